// nf_ladder.hip -- one replica-exchange sweep along the coupling ladders of nf_phi4_hmc_ladder / nf_phi4_hmc_tiled_ladder
// (MI355X-side extension, no counterpart in the reference).  C = K R chains, chain c in replica set c / K on rung rung[c];
// within a set the rungs are a permutation of 0 .. K - 1.  The phi^4 action is linear in a rung's (w0, w2, w4), with the
// coefficients Q = sum phi^2, P = sum phi^4 and Lam = the sum of the links: columns 1, 2 and 3 .. 6 of nf_lattice_measure's
// row.  A sweep of parity p tries the pairs of rungs (k, k + 1), k = p, p + 2, ..: the chains a (on k) and b (on k + 1)
// trade their RUNGS -- no configuration moves -- iff log u < Delta (ladder_delta, nf_sampler_core.h).
// One workgroup per replica set: the inverse map rung -> chain goes through LDS, then one lane per pair.  The pairs of a
// sweep are disjoint, so every entry of rung, action and swapped has one writer: no atomics, plain stores, the same inputs
// give the same bits.  A rung outside 0 .. K - 1 is left out of the inverse map and its pairs are not tried: nothing is
// read or written outside the arrays whatever `rung` holds.
#include "nf_sampler_core.h"

namespace nf {

constexpr int kLadderMaxK = 1024;
constexpr int kLadderLanes = 256;

struct LadderArgs {
  const double *rows;
  int64_t stride;
  const double *coef;
  int32_t *rung;
  double *action;
  uint8_t *swapped;
  int K, parity;
  PhiloxPos pos;
};

__global__ __launch_bounds__(kLadderLanes) void ladder_exchange_kernel(LadderArgs A) {
  __shared__ int inv[kLadderMaxK];
  const int tid = threadIdx.x, K = A.K;
  const int64_t set = blockIdx.x, c0 = set * K;
  for (int k = tid; k < K; k += kLadderLanes) inv[k] = -1;
  __syncthreads();
  for (int i = tid; i < K; i += kLadderLanes) {
    const int r = A.rung[c0 + i];
    if (r >= 0 && r < K) inv[r] = i;
  }
  __syncthreads();
  for (int k = tid; k + 1 < K; k += kLadderLanes) {
    bool ok = false;
    const int ia = inv[k], ib = inv[k + 1];
    if ((k & 1) == A.parity && ia >= 0 && ib >= 0) {
      const int64_t a = c0 + ia, b = c0 + ib;
      const double *ra = A.rows + a * A.stride, *rb = A.rows + b * A.stride;
      const double Qa = ra[1], Pa = ra[2], La = ra[3] + ra[4] + ra[5] + ra[6];
      const double Qb = rb[1], Pb = rb[2], Lb = rb[3] + rb[4] + rb[5] + rb[6];
      const double *wk = A.coef + 3 * k, *wn = wk + 3;
      const double delta = ladder_delta(wk[0] - wn[0], wk[1] - wn[1], wk[2] - wn[2], Qa - Qb, Pa - Pb, La - Lb);
      ok = philox_log_uniform(A.pos, uint64_t(c0) + uint64_t(k)) < delta;
      if (ok) {
        A.rung[a] = k + 1;
        A.rung[b] = k;
        if (A.action) {
          A.action[a] = wn[1] * Qa + wn[2] * Pa - wn[0] * La;
          A.action[b] = wk[1] * Qb + wk[2] * Pb - wk[0] * Lb;
        }
      }
    }
    A.swapped[set * (K - 1) + k] = uint8_t(ok);
  }
}

}  // namespace nf

using namespace nf;

extern "C" int nf_phi4_ladder_exchange(const double *rows, int64_t row_stride, const double *coef, int K, int32_t *rung,
                                       double *action, uint8_t *swapped, int64_t C, int parity, uint64_t seed,
                                       uint64_t offset, void *stream) {
  const char *what = "nf_phi4_ladder_exchange";
  NF_REQUIRE(rows && coef && rung, "%s: rows, coef or rung is NULL", what);
  NF_REQUIRE(K >= 1 && K <= kLadderMaxK, "%s: K (%d) must be in 1 .. %d", what, K, kLadderMaxK);
  NF_REQUIRE(C >= 1 && C % K == 0, "%s: C (%lld) must be a positive multiple of K (%d)", what, (long long)C, K);
  NF_REQUIRE(swapped != nullptr || K == 1, "%s: swapped is NULL", what);
  NF_REQUIRE(row_stride >= 7, "%s: row_stride (%lld) must be >= 7, the scalars of nf_lattice_measure's row", what,
             (long long)row_stride);
  NF_REQUIRE(parity == 0 || parity == 1, "%s: parity (%d) must be 0 or 1", what, parity);
  NF_REQUIRE(C / K <= (int64_t(1) << 31) - 1, "%s: %lld replica sets exceed one launch", what, (long long)(C / K));
  if (K == 1) return NF_OK;                        // no pair: nothing changes and nothing is written
  LadderArgs A{rows, row_stride, coef, rung, action, swapped, K, parity, philox_pos(seed, NF_PHILOX_EXCHANGE_DOMAIN, offset)};
  hipLaunchKernelGGL(ladder_exchange_kernel, dim3(unsigned(C / K)), dim3(kLadderLanes), 0, static_cast<hipStream_t>(stream), A);
  return check_launch(what);
}

// nf_mcmc.hip -- the two per-block kernels of the blocked Metropolis sampler (reference: src/mcmc/mcmc.py:132-220 with the
// block updater of src/prior/prior.py:106-112, 161-178), for C independent chains at once:
//   * nf_block_propose: save block k of every chain's prior-side field and redraw it from the normal prior (one launch
//     where the reference deep-copies the block and calls the chopped prior's sampler);
//   * nf_block_accept:  the Metropolis decision of every chain on the device, from the log q / log p the flow and the
//     action just produced, and the bitwise restore of the rejected chains' blocks (the reference does it per block on
//     the host: np.random, .item(), a bool test) -- no host round trip per block.
// Random numbers: Philox4x32-10 (nf_internal.h); the counter layouts are written out in include/normflow_hip.h.
#include "nf_internal.h"

namespace nf {

struct ProposeArgs {
  void *x;
  void *backup;
  const void *loc, *scale;     // (V) or null
  int64_t C, V, block_len, start, ngroups;
  uint32_t k0, k1, o0, o1;
};

// Grid-stride over (chain, Philox group): the group's normals are those nf_normal_sample draws for sample c of a
// (C, block_len) field, so the block equals normal_prior_sample(seed, offset, C, block_len, loc_blk, scale_blk).
template <typename T>
__global__ __launch_bounds__(kBlock) void block_propose_kernel(ProposeArgs A) {
  constexpr int PER = sizeof(T) == 4 ? 4 : 2;
  T *__restrict__ x = static_cast<T *>(A.x);
  T *__restrict__ bk = static_cast<T *>(A.backup);
  const T *loc = static_cast<const T *>(A.loc), *sc = static_cast<const T *>(A.scale);
  const int64_t total = A.C * A.ngroups;
  for (int64_t u = int64_t(blockIdx.x) * kBlock + threadIdx.x; u < total; u += int64_t(gridDim.x) * kBlock) {
    const int64_t c = u / A.ngroups, q = u - c * A.ngroups;
    const uint64_t g = uint64_t(u);                     // = c * ngroups + q
    uint32_t r[4] = {uint32_t(g), uint32_t(g >> 32), A.o0, A.o1};
    philox4x32_10(r, A.k0, A.k1);
    T z[PER];
    philox_normals<T>(r, z);
    T *xc = x + c * A.V + A.start;
    T *bc = bk + c * A.block_len;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int64_t i = q * PER + j;
      if (i < A.block_len) {
        const int64_t site = A.start + i;
        const T s = sc ? sc[site] : T(1);
        bc[i] = xc[i];
        xc[i] = (loc ? loc[site] : T(0)) + s * z[j];
      }
    }
  }
}

struct AcceptArgs {
  void *x;
  const void *backup, *logq, *logp;
  double *logqp_ref;
  uint8_t *accept;
  int64_t C, V, block_len, start;
  int force;
  uint32_t k0, k1, o0, o1;
};

// One workgroup per chain (grid-stride over chains): every lane draws the chain's uniform and takes the decision
// redundantly, then the lanes restore a rejected block together.
template <typename T>
__global__ __launch_bounds__(kBlock) void block_accept_kernel(AcceptArgs A) {
  T *__restrict__ x = static_cast<T *>(A.x);
  const T *__restrict__ bk = static_cast<const T *>(A.backup);
  const T *lq = static_cast<const T *>(A.logq), *lp = static_cast<const T *>(A.logp);
  for (int64_t c = blockIdx.x; c < A.C; c += gridDim.x) {
    uint32_t r[4] = {uint32_t(uint64_t(c)), uint32_t(uint64_t(c) >> 32), A.o0, A.o1};
    philox4x32_10(r, A.k0, A.k1);
    const double logu = ::log(philox_u53(r[0], r[1]));
    const double d = double(lq[c]) - double(lp[c]);
    const double ref = A.logqp_ref[c];
    const bool ok = A.force || logu < ref - d;
    __syncthreads();                                    // every lane has read logqp_ref[c] before it changes
    if (threadIdx.x == 0) {
      A.accept[c] = uint8_t(ok);
      if (ok) A.logqp_ref[c] = d;
    }
    if (!ok) {
      T *xc = x + c * A.V + A.start;
      const T *bc = bk + c * A.block_len;
      for (int64_t i = threadIdx.x; i < A.block_len; i += kBlock) xc[i] = bc[i];
    }
  }
}

static int block_checks(const char *what, int64_t C, int64_t V, int64_t block_len, int64_t block_ind, int dtype) {
  NF_REQUIRE(C >= 0 && V >= 1 && block_len >= 1 && block_ind >= 0 && block_len <= V && block_ind < V / block_len,
             "%s: block %lld of length %lld does not fit in %lld sites (C = %lld)", what, (long long)block_ind,
             (long long)block_len, (long long)V, (long long)C);
  NF_REQUIRE(dtype == NF_F32 || dtype == NF_F64, "%s: unsupported dtype %d", what, dtype);
  return NF_OK;
}

}  // namespace nf

using namespace nf;

extern "C" int nf_block_propose(void *x, void *backup, const void *loc, const void *scale, int64_t C, int64_t V,
                                int64_t block_len, int64_t block_ind, uint64_t seed, uint64_t offset, int dtype,
                                void *stream) {
  const int rc = block_checks("nf_block_propose", C, V, block_len, block_ind, dtype);
  if (rc) return rc;
  NF_REQUIRE(x && backup, "nf_block_propose: x or backup is NULL");
  if (C == 0) return NF_OK;
  ProposeArgs A{};
  A.x = x; A.backup = backup; A.loc = loc; A.scale = scale;
  A.C = C; A.V = V; A.block_len = block_len; A.start = block_ind * block_len;
  const int per = dtype == NF_F32 ? 4 : 2;
  A.ngroups = (block_len + per - 1) / per;
  // the key of nf_normal_sample: a draw here is a draw of that kernel on a (C, block_len) field
  A.k0 = uint32_t(seed); A.k1 = uint32_t(seed >> 32) ^ NF_PHILOX_KEY_DOMAIN; A.o0 = uint32_t(offset); A.o1 = uint32_t(offset >> 32);
  const int64_t total = C * A.ngroups;
  const int64_t blocks = (total + kBlock - 1) / kBlock;
  const unsigned grid = unsigned(blocks < 8192 ? blocks : 8192);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (dtype == NF_F32) hipLaunchKernelGGL((block_propose_kernel<float>), dim3(grid), dim3(kBlock), 0, s, A);
  else hipLaunchKernelGGL((block_propose_kernel<double>), dim3(grid), dim3(kBlock), 0, s, A);
  return check_launch("nf_block_propose");
}

extern "C" int nf_block_accept(void *x, const void *backup, const void *logq, const void *logp, double *logqp_ref,
                               uint8_t *accept_out, int64_t C, int64_t V, int64_t block_len, int64_t block_ind,
                               int force_accept, uint64_t seed, uint64_t offset, int dtype, void *stream) {
  const int rc = block_checks("nf_block_accept", C, V, block_len, block_ind, dtype);
  if (rc) return rc;
  NF_REQUIRE(x && backup && logq && logp && logqp_ref && accept_out, "nf_block_accept: NULL pointer argument");
  if (C == 0) return NF_OK;
  AcceptArgs A{};
  A.x = x; A.backup = backup; A.logq = logq; A.logp = logp; A.logqp_ref = logqp_ref; A.accept = accept_out;
  A.C = C; A.V = V; A.block_len = block_len; A.start = block_ind * block_len; A.force = force_accept != 0;
  A.k0 = uint32_t(seed); A.k1 = uint32_t(seed >> 32) ^ NF_PHILOX_ACCEPT_DOMAIN; A.o0 = uint32_t(offset); A.o1 = uint32_t(offset >> 32);
  const unsigned grid = unsigned(C < 65536 ? C : 65536);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (dtype == NF_F32) hipLaunchKernelGGL((block_accept_kernel<float>), dim3(grid), dim3(kBlock), 0, s, A);
  else hipLaunchKernelGGL((block_accept_kernel<double>), dim3(grid), dim3(kBlock), 0, s, A);
  return check_launch("nf_block_accept");
}

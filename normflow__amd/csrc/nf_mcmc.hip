// nf_mcmc.hip -- Metropolis accept/reject on the device.  First the two per-block kernels of the blocked Metropolis sampler (reference: src/mcmc/mcmc.py:132-220 with the
// block updater of src/prior/prior.py:106-112, 161-178), for C independent chains at once:
//   * nf_block_propose: save block k of every chain's prior-side field and redraw it from the normal prior (one launch
//     where the reference deep-copies the block and calls the chopped prior's sampler);
//   * nf_block_accept:  the Metropolis decision of every chain on the device, from the log q / log p the flow and the
//     action just produced, and the bitwise restore of the rejected chains' blocks (the reference does it per block on
//     the host: np.random, .item(), a bool test) -- no host round trip per block.
// Then the two kernels of the independence sampler with C chains (MCMCSampler(n_chains=C); reference: src/mcmc/mcmc.py:56-87
// and :304-328, two Python loops over the batch on the host, three index_select passes):
//   * nf_metropolis_chains: every decision of C chains over S steps in one launch, with the kept row's index and log q / log p;
//   * nf_metropolis_select: the rejected rows of the batch overwritten in place by the configuration their chain holds.
// Random numbers: Philox4x32-10 and the two draws (nf_sampler_core.h); the counter layouts: include/normflow_hip.h.
#include "nf_sampler_core.h"

namespace nf {

struct ProposeArgs {
  void *x;
  void *backup;
  const void *loc, *scale;     // (V) or null
  int64_t C, V, block_len, start, ngroups;
  PhiloxPos pos;
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
    T z[PER];
    philox_normal_group<T>(A.pos, uint64_t(u), z);      // u = c * ngroups + q
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
  PhiloxPos pos;
};

// One workgroup per chain (grid-stride over chains): every lane draws the chain's uniform and takes the decision
// redundantly, then the lanes restore a rejected block together.
template <typename T>
__global__ __launch_bounds__(kBlock) void block_accept_kernel(AcceptArgs A) {
  T *__restrict__ x = static_cast<T *>(A.x);
  const T *__restrict__ bk = static_cast<const T *>(A.backup);
  const T *lq = static_cast<const T *>(A.logq), *lp = static_cast<const T *>(A.logp);
  for (int64_t c = blockIdx.x; c < A.C; c += gridDim.x) {
    const double logu = philox_log_uniform(A.pos, uint64_t(c));
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


// ---------------------------------------------------------------- independence Metropolis, C chains x S steps
constexpr int kChainChunk = 1024;   // (step, chain) entries staged in LDS at a time: 8 KiB of log u + 2 x 1024 T

struct ChainsArgs {
  const void *logq, *logp;
  double *logqp_ref;
  void *ref_logq, *ref_logp;
  uint8_t *accept;
  int64_t *keep;
  void *logq_sel, *logp_sel;
  int64_t S, C;
  int fresh;
  PhiloxPos pos;
};

// Mapping: a workgroup owns a group of W <= 64 adjacent chains (grid-stride over the groups) and walks their steps in
// chunks of floor(1024 / W) steps.  Only logqp_ref carries a dependence from step to step, so a chunk is done in two phases:
//   1. all 256 threads: the Philox uniform and its log (the expensive part: a double log per row) and the loads of
//      log q / log p for the chunk's rows, into LDS.  Chains are adjacent in memory within a step, so the W-lane runs
//      read coalesced; nothing here waits on a decision;
//   2. lanes 0 .. W-1 of wave 0, one per chain: the scan over the chunk's steps, reading LDS at consecutive addresses
//      across lanes (no bank conflicts) -- per step a subtract, a compare and selects, no global load in the dependence
//      chain -- and storing the row's flag, kept row and selected log q / log p, coalesced across the chains.
// The chain state (logqp_ref, the kept row, its log q / log p) lives in the scan lane's registers across chunks.
// C >= 64: full waves scan, ceil(C / 64) workgroups.  C = 1: W = 1, phase 1 spreads 1024 steps over the workgroup and one
// lane scans them from LDS (~10 instructions per step); that serial scan is what an independence chain is.  A wider group
// than 64 would only idle more of phase 2; a narrower one would cut the coalesced runs.
template <typename T>
__global__ __launch_bounds__(kBlock) void metropolis_chains_kernel(ChainsArgs A) {
  __shared__ double s_logu[kChainChunk];
  __shared__ T s_lq[kChainChunk], s_lp[kChainChunk];
  const T *lq = static_cast<const T *>(A.logq), *lp = static_cast<const T *>(A.logp);
  T *rlq = static_cast<T *>(A.ref_logq), *rlp = static_cast<T *>(A.ref_logp);
  T *lq_sel = static_cast<T *>(A.logq_sel), *lp_sel = static_cast<T *>(A.logp_sel);
  const int tid = threadIdx.x;
  const int64_t ngroups = (A.C + kWave - 1) / kWave;
  for (int64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
    const int64_t c0 = g * kWave;
    const int W = int(A.C - c0 < kWave ? A.C - c0 : kWave);
    const int steps = kChainChunk / W;                  // steps per chunk, >= 16
    const bool scans = tid < W;
    const int64_t c = c0 + tid;
    double ref = 0.0;
    T cur_lq = T(0), cur_lp = T(0);
    int64_t cur_keep = c;                               // row c: where the select kernel puts the stored sample
    if (scans && !A.fresh) {
      ref = A.logqp_ref[c];
      cur_lq = rlq[c];
      cur_lp = rlp[c];
    }
    for (int64_t s0 = 0; s0 < A.S; s0 += steps) {
      const int ns = int(A.S - s0 < steps ? A.S - s0 : steps);
      const int n = ns * W;                             // <= kChainChunk
      for (int e = tid; e < n; e += kBlock) {
        const int sl = e / W, cl = e - sl * W;
        const uint64_t r = uint64_t((s0 + sl) * A.C + c0 + cl);
        s_logu[e] = philox_log_uniform(A.pos, r);
        s_lq[e] = lq[r];
        s_lp[e] = lp[r];
      }
      __syncthreads();
      if (scans) {
#pragma unroll 4
        for (int sl = 0; sl < ns; ++sl) {
          const int e = sl * W + tid;
          const T q = s_lq[e], p = s_lp[e];
          const double d = double(q) - double(p);
          const int64_t r = (s0 + sl) * A.C + c;
          const bool ok = (A.fresh && s0 + sl == 0) || s_logu[e] < ref - d;
          if (ok) {
            ref = d;
            cur_lq = q;
            cur_lp = p;
            cur_keep = r;
          }
          A.accept[r] = uint8_t(ok);
          A.keep[r] = cur_keep;
          lq_sel[r] = cur_lq;
          lp_sel[r] = cur_lp;
        }
      }
      __syncthreads();                                  // the chunk is consumed before the next one overwrites it
    }
    if (scans && A.S > 0) {
      A.logqp_ref[c] = ref;
      rlq[c] = cur_lq;
      rlp[c] = cur_lp;
    }
  }
}

struct SelectArgs {
  void *y;
  const void *ref_sample;
  const uint8_t *accept;
  const int64_t *keep;
  int64_t B, C, row_bytes;
};

// One wave per row (4 rows per workgroup, grid-stride): a wave that finds its row accepted has nothing to do; a rejected
// row is copied from its source in units of U (16 bytes where rows and bases are 16-byte aligned, else one element).
// Hazard-freedom within the launch: the rows WRITTEN are exactly the rows with accept == 0.  The rows READ are rows
// keep[r] with accept[keep[r]] != 0 -- accepted rows, which no wave writes -- and ref_sample, a separate buffer nobody
// writes.  The one row that is both a target of keep and written is a rejected step-0 row c (it receives the stored
// sample while later rows of chain c point at it): those later rows see accept[c] == 0 and read ref_sample[c] directly,
// never row c.  accept and keep are only read.  So no wave reads what another writes, in any order of execution.
template <typename U>
__global__ __launch_bounds__(kBlock) void metropolis_select_kernel(SelectArgs A) {
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
  constexpr int kRows = kBlock / kWave;
  const int64_t n = A.row_bytes / int64_t(sizeof(U));
  char *y = static_cast<char *>(A.y);
  for (int64_t r = int64_t(blockIdx.x) * kRows + w; r < A.B; r += int64_t(gridDim.x) * kRows) {
    if (A.accept[r]) continue;
    const int64_t k = A.keep[r];
    if (k < 0 || k >= A.B) continue;                    // never from this library's keep; no read out of bounds on a foreign one
    const char *from;
    if (A.accept[k]) {
      from = y + k * A.row_bytes;
    } else {
      if (!A.ref_sample) continue;
      from = static_cast<const char *>(A.ref_sample) + (r % A.C) * A.row_bytes;
    }
    const U *src = reinterpret_cast<const U *>(from);
    U *dst = reinterpret_cast<U *>(y + r * A.row_bytes);
    for (int64_t i = lane; i < n; i += kWave) dst[i] = src[i];
  }
}

template <typename U>
static void launch_select(const SelectArgs &A, unsigned grid, hipStream_t s) {
  hipLaunchKernelGGL((metropolis_select_kernel<U>), dim3(grid), dim3(kBlock), 0, s, A);
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
  A.pos = philox_pos(seed, NF_PHILOX_KEY_DOMAIN, offset);
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
  A.pos = philox_pos(seed, NF_PHILOX_ACCEPT_DOMAIN, offset);
  const unsigned grid = unsigned(C < 65536 ? C : 65536);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (dtype == NF_F32) hipLaunchKernelGGL((block_accept_kernel<float>), dim3(grid), dim3(kBlock), 0, s, A);
  else hipLaunchKernelGGL((block_accept_kernel<double>), dim3(grid), dim3(kBlock), 0, s, A);
  return check_launch("nf_block_accept");
}

extern "C" int nf_metropolis_chains(const void *logq, const void *logp, double *logqp_ref, void *ref_logq, void *ref_logp,
                                    uint8_t *accept, int64_t *keep, void *logq_sel, void *logp_sel, int64_t S, int64_t C,
                                    int fresh, uint64_t seed, uint64_t offset, int dtype, void *stream) {
  NF_REQUIRE(S >= 0 && C >= 0, "nf_metropolis_chains: S (%lld) and C (%lld) must not be negative", (long long)S, (long long)C);
  NF_REQUIRE(S == 0 || C <= INT64_MAX / S, "nf_metropolis_chains: S C overflows (S = %lld, C = %lld)", (long long)S, (long long)C);
  NF_REQUIRE(dtype == NF_F32 || dtype == NF_F64, "nf_metropolis_chains: unsupported dtype %d", dtype);
  NF_REQUIRE(logq && logp && logqp_ref && ref_logq && ref_logp && accept && keep && logq_sel && logp_sel,
             "nf_metropolis_chains: NULL pointer argument");
  if (S == 0 || C == 0) return NF_OK;
  ChainsArgs A{};
  A.logq = logq; A.logp = logp; A.logqp_ref = logqp_ref; A.ref_logq = ref_logq; A.ref_logp = ref_logp;
  A.accept = accept; A.keep = keep; A.logq_sel = logq_sel; A.logp_sel = logp_sel;
  A.S = S; A.C = C; A.fresh = fresh != 0;
  A.pos = philox_pos(seed, NF_PHILOX_CHAIN_DOMAIN, offset);
  const int64_t groups = (C + kWave - 1) / kWave;
  const unsigned grid = unsigned(groups < 65536 ? groups : 65536);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (dtype == NF_F32) hipLaunchKernelGGL((metropolis_chains_kernel<float>), dim3(grid), dim3(kBlock), 0, s, A);
  else hipLaunchKernelGGL((metropolis_chains_kernel<double>), dim3(grid), dim3(kBlock), 0, s, A);
  return check_launch("nf_metropolis_chains");
}

extern "C" int nf_metropolis_select(void *y, const void *ref_sample, const uint8_t *accept, const int64_t *keep, int64_t S,
                                    int64_t C, int64_t V, int elem_size, void *stream) {
  NF_REQUIRE(S >= 0 && C >= 0 && V >= 0, "nf_metropolis_select: S (%lld), C (%lld) and V (%lld) must not be negative",
             (long long)S, (long long)C, (long long)V);
  NF_REQUIRE(S == 0 || C <= INT64_MAX / S, "nf_metropolis_select: S C overflows (S = %lld, C = %lld)", (long long)S, (long long)C);
  NF_REQUIRE(elem_size == 1 || elem_size == 2 || elem_size == 4 || elem_size == 8,
             "nf_metropolis_select: unsupported element size %d", elem_size);
  NF_REQUIRE(S * C == 0 || V <= INT64_MAX / 8 / (S * C), "nf_metropolis_select: the field is too large (V = %lld)", (long long)V);
  NF_REQUIRE(y && accept && keep, "nf_metropolis_select: NULL pointer argument");
  if (S == 0 || C == 0 || V == 0) return NF_OK;
  SelectArgs A{};
  A.y = y; A.ref_sample = ref_sample; A.accept = accept; A.keep = keep;
  A.B = S * C; A.C = C; A.row_bytes = V * elem_size;
  const int64_t blocks = (A.B + kBlock / kWave - 1) / (kBlock / kWave);
  const unsigned grid = unsigned(blocks < 65536 ? blocks : 65536);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool wide = A.row_bytes % 16 == 0 && reinterpret_cast<uintptr_t>(y) % 16 == 0 &&
                    reinterpret_cast<uintptr_t>(ref_sample) % 16 == 0;
  if (wide) launch_select<uint4>(A, grid, s);
  else if (elem_size == 8) launch_select<uint64_t>(A, grid, s);
  else if (elem_size == 4) launch_select<uint32_t>(A, grid, s);
  else if (elem_size == 2) launch_select<uint16_t>(A, grid, s);
  else launch_select<uint8_t>(A, grid, s);
  return check_launch("nf_metropolis_select");
}

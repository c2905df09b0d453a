// nf_cluster_moments_tiled.hip -- the cluster-improved estimators for chains that live in HBM (MI355X-side extension, no
// counterpart in the reference): nf_cluster_moments' rule (include/normflow_hip.h, "cluster-improved estimators") for
// lattices beyond one CU's LDS, with the int64 slots in a workspace in HBM.
// A chain is cut into blocks of `block_sites` consecutive sites (and slots); the grid of the three site kernels is
// (blocks, C) with 256 lanes, lane tid of a block owns the sites first + tid + 256 k: coalesced loads.  On `stream`:
//   memset of the flags | CHECK: range and label test of every site, a refused chain's flag set (one atomicOr per block)
//   per pass of `per_pass` quantities:
//     memset of the pass's slot arrays
//     SCATTER: every site's q to the slot of its label, through the claim-add-flush table of nf_cluster_table.h in LDS
//     SQUARES: per block and quantity, lane l squares the slots first + l + 256 k (fma), wave shuffle tree, the 4 waves in
//              order -> the block's partial in the workspace; quantity 0 also writes moments_out
//   FINISH: one wave per (chain, column) adds the blocks' partials (lane l the blocks l, l + 64, ... in order, shuffle
//           tree), then the row, or NaNs, and status.
// Contention: adds to one HBM word from all over the chip go one after the other (nf_cluster_tiled.hip, phase 3), and at
// kappa = 0.67 one cluster holds 0.95 of the lattice.  A lane first sums its own consecutive sites that share a label in
// registers (a site is read ONCE per pass: all quantities of the pass are taken from it), then adds the run to the
// label's entry of the table with LDS integer adds; the table sends one global atomic per (label, quantity).  A run whose
// entry belongs to another label goes straight to HBM.  Everything is an integer sum: no grouping changes a bit.
// Everything that depends on the quantity is wave-uniform and picked with constant indices out of the kernel's
// arguments: nothing in registers is indexed dynamically, so there is no scratch.
#include "nf_internal.h"
#include "nf_cluster_table.h"

namespace nf {
namespace {

constexpr int kMtLanes = 256;
constexpr int kMtWaves = kMtLanes / kWave;
constexpr int kMtMaxQ = 9;                         // 1 + 2 x 4 axes
constexpr int kMtCols = kMtMaxQ + 1;               // sums of squares: a^2, a^4, then r^2 and i^2 of every axis
constexpr int kMtDefaultBlockSites = 4096;         // 16 sites per lane, as phases 3 and 4 of the tiled sweep
constexpr int kMtTable = 512;                      // H: entries of the table
constexpr size_t kMtAlign = 16;
static_assert((kMtTable & (kMtTable - 1)) == 0, "entry h = label & (H - 1)");
static_assert(size_t(kMtTable) * (4 + 8 * kMtMaxQ) <= 64 * 1024, "the table fits static LDS");

struct MtQuantity {
  int stride, extent, tw;        // of the quantity's axis: site stride, extent, the index of its first double in tw
};

struct MtPlan {
  int64_t V, blocks;
  int bs, nq, per_pass, passes;
  MtQuantity q[kMtMaxQ];         // q[0] is A (no twiddle)
  int col[4];                    // column of sum r^2 of axis mu among the sums of squares (i^2 is the next), -1: extent 1
  double limit;                  // 2^min(16, 30 - ceil(log2 V))
};

int mt_plan(const char *what, const int32_t *lattice, int dtype, int64_t block_sites, int per_pass, MtPlan &p) {
  NF_REQUIRE(lattice != nullptr, "%s: lattice is NULL", what);
  NF_REQUIRE(dtype == NF_F32 || dtype == NF_F64, "%s: unsupported dtype %d", what, dtype);
  p.V = 1;
  for (int mu = 0; mu < 4; ++mu) {
    NF_REQUIRE(lattice[mu] >= 1, "%s: lattice extents must be >= 1", what);
    p.V *= lattice[mu];
    NF_REQUIRE(p.V < (int64_t(1) << 31), "%s: the lattice (%d, %d, %d, %d) has 2^31 sites or more", what, lattice[0], lattice[1],
               lattice[2], lattice[3]);
  }
  NF_REQUIRE(block_sites >= 0, "%s: block_sites (%lld) must be 0 (the default, %d) or >= 1", what, (long long)block_sites,
             kMtDefaultBlockSites);
  const int64_t bs = block_sites ? block_sites : kMtDefaultBlockSites;
  p.bs = int(bs < p.V ? bs : p.V);
  p.blocks = (p.V + p.bs - 1) / p.bs;
  NF_REQUIRE(p.blocks * kMtLanes < (int64_t(1) << 32),
             "%s: %lld blocks of %d sites are more than one launch takes (blocks x lanes < 2^32)", what, (long long)p.blocks, p.bs);
  p.nq = 1;
  p.q[0] = MtQuantity{1, 1, 0};
  int stride = int(p.V), off = 0;
  for (int mu = 0; mu < 4; ++mu) {
    stride /= lattice[mu];
    p.col[mu] = -1;
    if (lattice[mu] > 1) {
      p.col[mu] = p.nq + 1;
      p.q[p.nq++] = MtQuantity{stride, lattice[mu], 2 * off};
      p.q[p.nq++] = MtQuantity{stride, lattice[mu], 2 * off + 1};
    }
    off += lattice[mu];
  }
  for (int k = p.nq; k < kMtMaxQ; ++k) p.q[k] = MtQuantity{1, 1, 0};
  NF_REQUIRE(per_pass >= 0 && per_pass <= p.nq, "%s: per_pass (%d) must be 0 (all) or 1 .. %d, the quantities of the lattice",
             what, per_pass, p.nq);
  p.per_pass = per_pass ? per_pass : p.nq;
  p.passes = (p.nq + p.per_pass - 1) / p.per_pass;
  int lg = 0;
  while ((int64_t(1) << lg) < p.V) ++lg;
  const int e = 30 - lg < 16 ? 30 - lg : 16;
  p.limit = e >= 0 ? double(int64_t(1) << e) : 1.0 / double(int64_t(1) << -e);
  return NF_OK;
}

size_t mt_flag_bytes(int64_t C) { return (size_t(C) * 4 + kMtAlign - 1) & ~(kMtAlign - 1); }
size_t mt_slot_bytes(int64_t C, const MtPlan &p) { return size_t(p.per_pass) * size_t(C) * size_t(p.V) * 8; }
size_t mt_workspace(int64_t C, const MtPlan &p) {
  return mt_flag_bytes(C) + mt_slot_bytes(C, p) + size_t(C) * size_t(p.blocks) * kMtCols * sizeof(double);
}

struct MtArgs {
  const void *phi;
  const int32_t *labels;
  double *out;
  int32_t *status;
  int64_t *moments;
  const double *tw;
  int *flags;                    // [C]: the chain is refused
  unsigned long long *slots;     // [per_pass][C][V]
  double *part;                  // [C][kMtCols][blocks]
  int V, bs, blocks, C, nq;
  int q0, nqp;                   // the pass: quantities q0 .. q0 + nqp - 1
  int col[4];
  MtQuantity q[kMtMaxQ];
  double limit;
};

struct DeviceTable {
  typedef int key;
  typedef unsigned long long sum;
  static __device__ __forceinline__ void init_key(key *p) { *p = -1; }
  static __device__ __forceinline__ void init_sum(sum *p) { *p = 0; }
  static __device__ __forceinline__ int claim(key *p, int label) { return atomicCAS(p, -1, label); }       // LDS
  static __device__ __forceinline__ int load(const key *p) { return *p; }
  static __device__ __forceinline__ void add_table(sum *p, unsigned long long v) { atomicAdd(p, v); }      // LDS
  static __device__ __forceinline__ unsigned long long read_table(const sum *p) { return *p; }
  static __device__ __forceinline__ void add_out(sum *p, unsigned long long v) { atomicAdd(p, v); }        // HBM, no return
};

// ---------------------------------------------------------------- check: before anything is indexed by a label
template <typename T>
__global__ __launch_bounds__(kMtLanes) void moments_tiled_check_kernel(MtArgs A) {
  const int V = A.V;
  const int64_t c = blockIdx.y;
  const int64_t first = int64_t(blockIdx.x) * A.bs;
  const int64_t last = first + A.bs < V ? first + A.bs : int64_t(V);
  const T *__restrict__ gphi = static_cast<const T *>(A.phi) + c * int64_t(V);
  const int32_t *__restrict__ glab = A.labels + c * int64_t(V);
  int bad = 0;
  for (int64_t x = first + threadIdx.x; x < last; x += kMtLanes) {
    const int l = glab[x];
    if (!(fabs(double(gphi[x])) < A.limit) || l < 0 || l >= V) bad = 1;
  }
  bad = __syncthreads_or(bad);
  if (bad && threadIdx.x == 0) atomicOr(&A.flags[c], 1);
}

// ---------------------------------------------------------------- scatter: every site's q to the slot of its label
template <typename T>
__global__ __launch_bounds__(kMtLanes) void moments_tiled_scatter_kernel(MtArgs A) {
  __shared__ int keys[kMtTable];
  __shared__ unsigned long long sums[kMtMaxQ * kMtTable];
  const int tid = threadIdx.x, V = A.V, H = kMtTable;
  const int64_t c = blockIdx.y;
  if (A.flags[c]) return;                                             // final since the check ended; the same in every lane
  const int64_t first = int64_t(blockIdx.x) * A.bs;
  const int64_t last = first + A.bs < V ? first + A.bs : int64_t(V);
  const T *__restrict__ gphi = static_cast<const T *>(A.phi) + c * int64_t(V);
  const int32_t *__restrict__ glab = A.labels + c * int64_t(V);
  const double *__restrict__ tw = A.tw;
  const int lo = A.q0, hi = A.q0 + A.nqp;
  const int64_t qstride = int64_t(A.C) * V;                           // between the slot arrays of two quantities
  unsigned long long *slots = A.slots + c * int64_t(V);               // of quantity lo

  table_clear<DeviceTable>(keys, sums, H, A.nqp, tid, kMtLanes);
  __syncthreads();

  int run = -1;                         // the label of the lane's current run of sites, and their sums
  long long sum[kMtMaxQ];
#pragma unroll
  for (int k = 0; k < kMtMaxQ; ++k) sum[k] = 0;
  auto commit = [&]() {
    const int h = table_claim<DeviceTable>(keys, H, run);
#pragma unroll
    for (int k = 0; k < kMtMaxQ; ++k)
      if (k >= lo && k < hi) table_add<DeviceTable>(sums, H, h, k - lo, slots + (k - lo) * qstride, run, sum[k]);
  };
  for (int64_t xx = first + tid; xx < last; xx += kMtLanes) {
    const int x = int(xx);
    const int l = glab[x];
    const double w = double(gphi[x]);
    if (l != run) {
      if (run >= 0) commit();
      run = l;
#pragma unroll
      for (int k = 0; k < kMtMaxQ; ++k) sum[k] = 0;
    }
    if (lo == 0) sum[0] += static_cast<long long>(rint(w * 4294967296.0));
#pragma unroll
    for (int k = 1; k < kMtMaxQ; k += 2) {                            // r and i of one axis
      const bool wr = k >= lo && k < hi, wi = k + 1 >= lo && k + 1 < hi;
      if (wr || wi) {
        const int t = 2 * int((unsigned(x) / unsigned(A.q[k].stride)) % unsigned(A.q[k].extent));
        if (wr) {
          const double v = w * tw[A.q[k].tw + t];
          sum[k] += static_cast<long long>(rint(v * 4294967296.0));
        }
        if (wi) {
          const double v = w * tw[A.q[k + 1].tw + t];
          sum[k + 1] += static_cast<long long>(rint(v * 4294967296.0));
        }
      }
    }
  }
  if (run >= 0) commit();
  __syncthreads();
  table_flush<DeviceTable>(keys, sums, H, A.nqp, slots, qstride, tid, kMtLanes);
}

// ---------------------------------------------------------------- squares: the blocks' partials
__global__ __launch_bounds__(kMtLanes) void moments_tiled_squares_kernel(MtArgs A) {
  __shared__ double red[kMtWaves][kMtCols];
  const int tid = threadIdx.x, V = A.V;
  const int lane = tid & (kWave - 1), wave = tid / kWave;
  const int64_t c = blockIdx.y;
  const int64_t first = int64_t(blockIdx.x) * A.bs;
  const int64_t last = first + A.bs < V ? first + A.bs : int64_t(V);
  if (A.flags[c]) {
    if (A.q0 == 0 && A.moments)
      for (int64_t s = first + tid; s < last; s += kMtLanes) A.moments[c * int64_t(V) + s] = 0;
    return;
  }
  const int64_t qstride = int64_t(A.C) * V;
#pragma unroll 1
  for (int j = 0; j < A.nqp; ++j) {
    const int qid = A.q0 + j;
    const unsigned long long *slot = A.slots + j * qstride + c * int64_t(V);
    double s2 = 0, s4 = 0;
    for (int64_t s = first + tid; s < last; s += kMtLanes) {
      const long long v = static_cast<long long>(slot[s]);
      const double a = double(v) * 0x1p-32, a2 = a * a;
      s2 = fma(a, a, s2);
      if (qid == 0) {
        s4 = fma(a2, a2, s4);
        if (A.moments) A.moments[c * int64_t(V) + s] = v;
      }
    }
    s2 = wave_sum(s2);
    if (qid == 0) s4 = wave_sum(s4);
    if (lane == 0) {
      red[wave][qid ? qid + 1 : 0] = s2;
      if (qid == 0) red[wave][1] = s4;
    }
  }
  __syncthreads();
  const int col0 = A.q0 ? A.q0 + 1 : 0, col1 = A.q0 + A.nqp + 1;      // the columns of the pass
  if (col0 + tid < col1) {
    const int col = col0 + tid;
    double r = 0;
#pragma unroll
    for (int w = 0; w < kMtWaves; ++w) r += red[w][col];
    A.part[(c * kMtCols + col) * int64_t(A.blocks) + blockIdx.x] = r;
  }
}

// ---------------------------------------------------------------- finish: the blocks in order, the row, status
__global__ __launch_bounds__(kMtCols *kWave) void moments_tiled_finish_kernel(MtArgs A) {
  __shared__ double res[kMtCols];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), col = tid / kWave;
  const int64_t c = blockIdx.x;
  if (A.flags[c]) {
    if (tid == 0) A.status[c] = 1;
    if (tid < 6) A.out[6 * c + tid] = __builtin_nan("");
    return;
  }
  if (col <= A.nq) {
    const double *part = A.part + (c * kMtCols + col) * int64_t(A.blocks);
    double r = 0;
    for (int b = lane; b < A.blocks; b += kWave) r += part[b];
    r = wave_sum(r);
    if (lane == 0) res[col] = r;
  }
  __syncthreads();
  if (tid == 0) {
    A.status[c] = 0;
    A.out[6 * c] = res[0];
    A.out[6 * c + 1] = res[1];
#pragma unroll
    for (int mu = 0; mu < 4; ++mu) A.out[6 * c + 2 + mu] = A.col[mu] < 0 ? res[0] : res[A.col[mu]] + res[A.col[mu] + 1];
  }
}

template <typename T>
int mt_launch(const char *what, MtArgs A, int64_t C, const MtPlan &p, hipStream_t s) {
  if (hipMemsetAsync(A.flags, 0, mt_flag_bytes(C), s) != hipSuccess) {
    (void)hipGetLastError();
    set_error("%s: cannot clear the flags of the workspace", what);
    return NF_ELAUNCH;
  }
  const dim3 grid(unsigned(p.blocks), unsigned(C)), lanes(kMtLanes);
  hipLaunchKernelGGL(moments_tiled_check_kernel<T>, grid, lanes, 0, s, A);
  int rc = check_launch(what);
  if (rc) return rc;
  for (int q0 = 0; q0 < p.nq; q0 += p.per_pass) {
    A.q0 = q0;
    A.nqp = p.nq - q0 < p.per_pass ? p.nq - q0 : p.per_pass;
    if (hipMemsetAsync(A.slots, 0, size_t(A.nqp) * size_t(C) * size_t(p.V) * 8, s) != hipSuccess) {
      (void)hipGetLastError();
      set_error("%s: cannot clear the slots of the workspace", what);
      return NF_ELAUNCH;
    }
    hipLaunchKernelGGL(moments_tiled_scatter_kernel<T>, grid, lanes, 0, s, A);
    if ((rc = check_launch(what))) return rc;
    hipLaunchKernelGGL(moments_tiled_squares_kernel, grid, lanes, 0, s, A);
    if ((rc = check_launch(what))) return rc;
  }
  hipLaunchKernelGGL(moments_tiled_finish_kernel, dim3(unsigned(C)), dim3(kMtCols * kWave), 0, s, A);
  return check_launch(what);
}

}  // namespace
}  // namespace nf

using namespace nf;

extern "C" int nf_cluster_moments_tiled_supported(const int32_t *lattice, int dtype, int64_t block_sites) {
  MtPlan p;
  return mt_plan("nf_cluster_moments_tiled_supported", lattice, dtype, block_sites, 0, p) == NF_OK ? 1 : 0;
}

extern "C" int nf_cluster_moments_tiled_plan(const int32_t *lattice, int dtype, int64_t block_sites, int per_pass,
                                             nf_moments_tiled_plan *out) {
  NF_REQUIRE(out != nullptr, "nf_cluster_moments_tiled_plan: out is NULL");
  MtPlan p;
  const int rc = mt_plan("nf_cluster_moments_tiled_plan", lattice, dtype, block_sites, per_pass, p);
  if (rc) return rc;
  out->blocks = p.blocks;
  out->block_sites = p.bs;
  out->quantities = p.nq;
  out->per_pass = p.per_pass;
  out->passes = p.passes;
  out->table_entries = kMtTable;
  out->launches = 2 + 2 * p.passes;
  out->lds_bytes = int64_t(kMtTable) * (4 + 8 * kMtMaxQ);
  return NF_OK;
}

extern "C" size_t nf_cluster_moments_tiled_workspace(int64_t C, const int32_t *lattice, int64_t block_sites, int per_pass) {
  MtPlan p;
  if (C < 1 || C > 65535 || mt_plan("nf_cluster_moments_tiled_workspace", lattice, NF_F32, block_sites, per_pass, p) != NF_OK)
    return 0;
  return mt_workspace(C, p);
}

extern "C" int nf_cluster_moments_tiled(const void *phi, const int32_t *labels, double *out, int32_t *status,
                                        int64_t *moments_out, int64_t C, const int32_t *lattice, const double *tw, int dtype,
                                        int64_t block_sites, int per_pass, void *workspace, size_t workspace_bytes,
                                        void *stream) {
  const char *what = "nf_cluster_moments_tiled";
  NF_REQUIRE(phi && labels && out && status, "%s: phi, labels, out or status is NULL", what);
  NF_REQUIRE(tw != nullptr, "%s: tw is NULL", what);
  NF_REQUIRE(C >= 1 && C <= 65535, "%s: C (%lld) must be in 1 .. 65535", what, (long long)C);
  MtPlan p;
  const int rc = mt_plan(what, lattice, dtype, block_sites, per_pass, p);
  if (rc) return rc;
  const size_t need = mt_workspace(C, p);
  NF_REQUIRE(workspace != nullptr, "%s: workspace is NULL (%zu B needed)", what, need);
  NF_REQUIRE(workspace_bytes >= need, "%s: workspace of %zu B is too small, %zu B needed", what, workspace_bytes, need);
  NF_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % kMtAlign == 0, "%s: workspace is not aligned to %zu B", what, kMtAlign);
  MtArgs A{};
  A.phi = phi; A.labels = labels; A.out = out; A.status = status; A.moments = moments_out; A.tw = tw;
  unsigned char *w = static_cast<unsigned char *>(workspace);
  A.flags = reinterpret_cast<int *>(w);
  A.slots = reinterpret_cast<unsigned long long *>(w + mt_flag_bytes(C));
  A.part = reinterpret_cast<double *>(w + mt_flag_bytes(C) + mt_slot_bytes(C, p));
  A.V = int(p.V); A.bs = p.bs; A.blocks = int(p.blocks); A.C = int(C); A.nq = p.nq;
  for (int mu = 0; mu < 4; ++mu) A.col[mu] = p.col[mu];
  for (int k = 0; k < kMtMaxQ; ++k) A.q[k] = p.q[k];
  A.limit = p.limit;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return dtype == NF_F32 ? mt_launch<float>(what, A, C, p, s) : mt_launch<double>(what, A, C, p, s);
}

// nf_cluster_modes_tiled.hip -- the cluster modes for chains that live in HBM (MI355X-side extension, no counterpart in
// the reference): nf_cluster_modes' rule (include/normflow_hip.h, "cluster modes") for lattices beyond one CU's LDS, with
// the int64 slots in a workspace in HBM and nf_cluster_moments_tiled's order of the sums of squares.
// The structure is nf_cluster_spectrum_tiled.hip's.  A chain is cut into blocks of `block_sites` consecutive sites (and
// slots); the grid of the three site kernels is (blocks, C) with 256 lanes, lane tid of a block owns the sites
// first + tid + 256 k.  On `stream`:
//   memset of the flags | CHECK: range and label test of every site, a refused chain's flag bit 0 set (one atomicOr per
//                         block); block 0 of a chain holds every row of desc to cm_row_ok, a failing table sets bit 1
//   per pass of up to `per_pass` <= 16 quantities:
//     memset of the pass's slot arrays
//     SCATTER: every site's q of every quantity of the pass to the slot of its label, through the claim-add-flush table of
//              nf_cluster_table.h in dynamic LDS (H = 512 entries, 512 (4 + 8 per_pass) bytes)
//     SQUARES: per block and quantity, lane l squares the slots first + l + 256 k (fma), wave shuffle tree, the 4 waves in
//              order -> the block's partial in the workspace
//   FINISH: one wave per (chain, sum) adds the blocks' partials (lane l the blocks l, l + 64, ... in order, shuffle tree),
//           then the row: columns 0 and 1, per momentum sum r^2 + sum i^2, sum r^2 alone for a self-conjugate one; or
//           NaNs; and status.  With a failing table: status 1 and nothing else.
// The quantities of a pass are consecutive indices q0 .. q0 + n - 1.  Their rows of desc (nf_cluster_modes_core.h) are
// read with wave-uniform loads in front of the site loop and kept packed: m_mu < N <= 2^16, two to a word.  A site is read
// ONCE per pass, its coordinates are taken once, and the phase j(x) (nf_cluster_modes_tiled_core.h: every product reduced
// mod N before the axes are added, no division) once per momentum of the pass: an I takes the phase of the R in front of
// it, an I that begins a pass forms it anew.  The scatter kernel is instantiated for every pass size NP = 1 .. 16: a pass
// of n quantities carries n descriptors and n run sums, picked with constant indices out of unrolled loops: nothing in
// registers is indexed dynamically, so there is no scratch.
#include <string>

#include "nf_internal.h"
#include "nf_cluster_modes_core.h"
#include "nf_cluster_modes_tiled_core.h"
#include "nf_cluster_table.h"

namespace nf {
namespace {

constexpr int kMtLanes = 256;
constexpr int kMtWaves = kMtLanes / kWave;
constexpr int kMtMaxPass = kCmtMaxPass;            // quantities per pass: nf_cluster_modes' cap, a lane's sums in registers
constexpr int kMtMaxQ = 1 + 2 * kCmMaxModes;       // 1025: bounds the launches (2 + 2 passes) and the partials
constexpr int kMtDefaultBlockSites = 4096;         // nf_cluster_moments_tiled's
constexpr int kMtTable = kCmtTable;                // H: entries of the table
constexpr int kMtFinishLanes = 1024;
constexpr size_t kMtAlign = 16;
enum { kMtBadChain = 1, kMtBadTable = 2 };         // bits of a chain's flag
static_assert((kMtTable & (kMtTable - 1)) == 0, "entry h = label & (H - 1)");
static_assert(size_t(kMtTable) * (4 + 8 * kMtMaxPass) <= 160 * 1024, "the table fits the LDS of a CU");

struct MtPlan {
  int64_t V, blocks;
  int bs, N, nq, per_pass, passes;
  int extent[4];
  size_t lds;
  double limit;                  // 2^min(16, 30 - ceil(log2 V))
};

int mt_plan(const char *what, const int32_t *lattice, int dtype, int Q, int64_t block_sites, int per_pass, MtPlan &p) {
  NF_REQUIRE(lattice != nullptr, "%s: lattice is NULL", what);
  NF_REQUIRE(dtype == NF_F32 || dtype == NF_F64, "%s: unsupported dtype %d", what, dtype);
  p.V = 1;
  for (int mu = 0; mu < 4; ++mu) {
    NF_REQUIRE(lattice[mu] >= 1, "%s: lattice extents must be >= 1, got (%d, %d, %d, %d)", what, lattice[0], lattice[1],
               lattice[2], lattice[3]);
    p.V *= lattice[mu];
    NF_REQUIRE(p.V < (int64_t(1) << 31), "%s: the lattice (%d, %d, %d, %d) has 2^31 sites or more", what, lattice[0], lattice[1],
               lattice[2], lattice[3]);
    p.extent[mu] = lattice[mu];
  }
  const long long lcm = cm_lcm(lattice);
  NF_REQUIRE(lcm > 1, "%s: every extent of the lattice (%d, %d, %d, %d) is 1 (N = 1): there is no momentum", what, lattice[0],
             lattice[1], lattice[2], lattice[3]);
  NF_REQUIRE(lcm <= kCmMaxN, "%s: N, the lcm of the extents of the lattice (%d, %d, %d, %d), is above %d", what, lattice[0],
             lattice[1], lattice[2], lattice[3], kCmMaxN);
  p.N = int(lcm);
  NF_REQUIRE(Q >= 2 && Q <= kMtMaxQ, "%s: Q (%d) must be in 2 .. %d", what, Q, kMtMaxQ);
  p.nq = Q;
  NF_REQUIRE(block_sites >= 0, "%s: block_sites (%lld) must be 0 (the default, %d) or >= 1", what, (long long)block_sites,
             kMtDefaultBlockSites);
  const int64_t bs = block_sites ? block_sites : kMtDefaultBlockSites;
  p.bs = int(bs < p.V ? bs : p.V);
  p.blocks = (p.V + p.bs - 1) / p.bs;
  NF_REQUIRE(p.blocks * kMtLanes < (int64_t(1) << 32),
             "%s: %lld blocks of %d sites are more than one launch takes (blocks x lanes < 2^32)", what, (long long)p.blocks, p.bs);
  const int cap = Q < kMtMaxPass ? Q : kMtMaxPass;
  NF_REQUIRE(per_pass >= 0 && per_pass <= cap,
             "%s: per_pass (%d) must be 0 (as many as fit) or 1 .. %d, the smaller of the quantities and %d", what, per_pass, cap,
             kMtMaxPass);
  p.per_pass = cmt_per_pass(Q, per_pass);
  p.passes = cmt_passes(Q, p.per_pass);
  p.lds = size_t(cmt_lds_bytes(p.per_pass));
  int lg = 0;
  while ((int64_t(1) << lg) < p.V) ++lg;
  const int e = 30 - lg < 16 ? 30 - lg : 16;
  p.limit = e >= 0 ? double(int64_t(1) << e) : 1.0 / double(int64_t(1) << -e);
  return NF_OK;
}

// Q and N of a host list, by nf_cluster_modes_describe; its refusal under this function's name
int mt_list(const char *what, const int32_t *lattice, const int32_t *modes, int P, int *Q, int *N) {
  int32_t q = 0, n = 0;
  const int rc = nf_cluster_modes_describe(lattice, modes, P, nullptr, &q, &n);
  if (rc) {
    const std::string why = nf_last_error_string();
    set_error("%s: %s", what, why.c_str());
    return rc;
  }
  *Q = q;
  *N = n;
  return NF_OK;
}

size_t mt_flag_bytes(int64_t C) { return (size_t(C) * 4 + kMtAlign - 1) & ~(kMtAlign - 1); }
size_t mt_slot_bytes(int64_t C, const MtPlan &p) { return size_t(p.per_pass) * size_t(C) * size_t(p.V) * 8; }
size_t mt_workspace(int64_t C, const MtPlan &p) {
  return mt_flag_bytes(C) + mt_slot_bytes(C, p) + size_t(C) * size_t(p.nq + 1) * size_t(p.blocks) * sizeof(double);
}

struct MtArgs {
  const void *phi;
  const int32_t *labels;
  double *out;
  int32_t *status;
  const double *tw;              // twN (N, 2)
  const int32_t *desc;           // (Q, 8)
  int *flags;                    // [C]: kMtBadChain | kMtBadTable
  unsigned long long *slots;     // [per_pass][C][V]
  double *part;                  // [C][Q + 1][blocks]: a^2, a^4, then one sum per further quantity
  int V, bs, blocks, C, nq, N;
  unsigned magic;                // cmt_magic(N)
  int q0, nqp;                   // the pass: quantities q0 .. q0 + nqp - 1
  int extent[4];
  double limit;
};

struct MtDeviceTable {
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

// ---------------------------------------------------------------- check: before anything is indexed by a label or a row
template <typename T>
__global__ __launch_bounds__(kMtLanes) void modes_tiled_check_kernel(MtArgs A) {
  const int V = A.V;
  const int64_t c = blockIdx.y;
  const int64_t first = int64_t(blockIdx.x) * A.bs;
  const int64_t last = first + A.bs < V ? first + A.bs : int64_t(V);
  const T *__restrict__ gphi = static_cast<const T *>(A.phi) + c * int64_t(V);
  const int32_t *__restrict__ glab = A.labels + c * int64_t(V);
  int bad = 0, bad_row = 0;
  for (int64_t x = first + threadIdx.x; x < last; x += kMtLanes) {
    const int l = glab[x];
    if (!(fabs(double(gphi[x])) < A.limit) || l < 0 || l >= V) bad = 1;
  }
  if (blockIdx.x == 0) {                                              // the table: once per chain, every row
    const int ncols = A.desc[kCmMode];                                // row 0: 2 + P
    for (int q = threadIdx.x; q < A.nq; q += kMtLanes)
      if (!cm_row_ok(A.desc, q, A.nq, A.N, ncols)) bad_row = 1;
  }
  bad = __syncthreads_or(bad);
  bad_row = __syncthreads_or(bad_row);
  if ((bad || bad_row) && threadIdx.x == 0) atomicOr(&A.flags[c], (bad ? kMtBadChain : 0) | (bad_row ? kMtBadTable : 0));
}

// ---------------------------------------------------------------- scatter: every site's q to the slot of its label
enum { kMtComp = 1, kMtFresh = 2, kMtTwiddle = 4 };                   // bits of how[j]: I | the phase anew | not A

// NP: the quantities of the pass, a compile-time number, so that a pass of n quantities carries n descriptors and n sums
template <typename T, int NP>
__global__ __launch_bounds__(kMtLanes) void modes_tiled_scatter_kernel(MtArgs A) {
  extern __shared__ __align__(16) unsigned char mt_lds[];
  const int tid = threadIdx.x, V = A.V, H = kMtTable;
  constexpr int nqp = NP;
  unsigned long long *sums = reinterpret_cast<unsigned long long *>(mt_lds);          // [nqp][H]
  int *keys = reinterpret_cast<int *>(mt_lds + size_t(nqp) * H * 8);                   // [H]
  const int64_t c = blockIdx.y;
  if (A.flags[c]) return;                                             // final since the check ended; the same in every lane
  const int64_t first = int64_t(blockIdx.x) * A.bs;
  const int64_t last = first + A.bs < V ? first + A.bs : int64_t(V);
  const T *__restrict__ gphi = static_cast<const T *>(A.phi) + c * int64_t(V);
  const int32_t *__restrict__ glab = A.labels + c * int64_t(V);
  const double *__restrict__ tw = A.tw;
  const int64_t qstride = int64_t(A.C) * V;                           // between the slot arrays of two quantities
  unsigned long long *slots = A.slots + c * int64_t(V);               // of quantity q0
  const unsigned N = unsigned(A.N), M = A.magic;
  const unsigned L1 = unsigned(A.extent[1]), L2 = unsigned(A.extent[2]), L3 = unsigned(A.extent[3]);

  table_clear<MtDeviceTable>(keys, sums, H, nqp, tid, kMtLanes);

  // ---- the pass's rows of desc, wave-uniform, in front of the site loop; the table passed cm_row_ok: m_mu < N <= 2^16
  unsigned m01[NP], m23[NP];                                          // m_0 | m_1 << 16, m_2 | m_3 << 16
  int how[NP];
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    m01[j] = m23[j] = 0;
    how[j] = 0;
    const int qid = A.q0 + j;
    if (qid > 0) {
      const int32_t *d = A.desc + size_t(qid) * kCmRow;
      m01[j] = unsigned(d[kCmM]) | unsigned(d[kCmM + 1]) << 16;
      m23[j] = unsigned(d[kCmM + 2]) | unsigned(d[kCmM + 3]) << 16;
      const int comp = d[kCmComp];
      how[j] = kMtTwiddle | (comp == 0 || j == 0 ? kMtFresh : 0) | (comp ? kMtComp : 0);      // an I that begins a pass: anew
    }
  }
  __syncthreads();

  int run = -1;                         // the label of the lane's current run of sites, and their sums
  long long sum[NP];
#pragma unroll
  for (int j = 0; j < NP; ++j) sum[j] = 0;
  auto commit = [&]() {
    const int h = table_claim<MtDeviceTable>(keys, H, run);
#pragma unroll
    for (int j = 0; j < NP; ++j)
      table_add<MtDeviceTable>(sums, H, h, j, slots + j * qstride, run, sum[j]);
  };
  for (int64_t xx = first + tid; xx < last; xx += kMtLanes) {
    const unsigned x = unsigned(xx);
    const int l = glab[x];
    const double w = double(gphi[x]);
    if (l != run) {
      if (run >= 0) commit();
      run = l;
#pragma unroll
      for (int j = 0; j < NP; ++j) sum[j] = 0;
    }
    // the coordinates, once per site: x = ((x_0 L_1 + x_1) L_2 + x_2) L_3 + x_3
    unsigned r = x;
    const unsigned x3 = r % L3; r /= L3;
    const unsigned x2 = r % L2; r /= L2;
    const unsigned x1 = r % L1;
    const unsigned x0 = r / L1;
    unsigned t = 0;                                                   // j(x) of the momentum in hand
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      double v = w;
      if (how[j] & kMtTwiddle) {
        if (how[j] & kMtFresh)
          t = cmt_phase(m01[j] & 0xffffu, m01[j] >> 16, m23[j] & 0xffffu, m23[j] >> 16, x0, x1, x2, x3, N, M);
        v = w * tw[2 * size_t(t) + size_t(how[j] & kMtComp)];
      }
      sum[j] += static_cast<long long>(rint(v * 4294967296.0));
    }
  }
  if (run >= 0) commit();
  __syncthreads();
  table_flush<MtDeviceTable>(keys, sums, H, nqp, slots, qstride, tid, kMtLanes);
}

// ---------------------------------------------------------------- squares: the blocks' partials
__global__ __launch_bounds__(kMtLanes) void modes_tiled_squares_kernel(MtArgs A) {
  __shared__ double red[kMtWaves][kMtMaxPass + 1];                    // the pass's sums, and a^4 of quantity 0 in the last
  const int tid = threadIdx.x, V = A.V;
  const int lane = tid & (kWave - 1), wave = tid / kWave;
  const int64_t c = blockIdx.y;
  const int64_t first = int64_t(blockIdx.x) * A.bs;
  const int64_t last = first + A.bs < V ? first + A.bs : int64_t(V);
  if (A.flags[c]) return;
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
      if (qid == 0) s4 = fma(a2, a2, s4);
    }
    s2 = wave_sum(s2);
    if (qid == 0) s4 = wave_sum(s4);
    if (lane == 0) {
      red[wave][j] = s2;
      if (qid == 0) red[wave][kMtMaxPass] = s4;
    }
  }
  __syncthreads();
  if (tid < A.nqp || (tid == kMtMaxPass && A.q0 == 0)) {
    double r = 0;
#pragma unroll
    for (int w = 0; w < kMtWaves; ++w) r += red[w][tid];
    const int at = tid == kMtMaxPass ? kCmtPartialA4 : cmt_partial_of(A.q0 + tid);
    A.part[(c * int64_t(A.nq + 1) + at) * int64_t(A.blocks) + blockIdx.x] = r;
  }
}

// ---------------------------------------------------------------- finish: the blocks in order, the row, status
__global__ __launch_bounds__(kMtFinishLanes) void modes_tiled_finish_kernel(MtArgs A) {
  __shared__ double res[kMtMaxQ + 1];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int64_t c = blockIdx.x;
  const int flag = A.flags[c];
  if (flag & kMtBadTable) {            // the row's length is the table's own word: out is left alone
    if (tid == 0) A.status[c] = 1;
    return;
  }
  const int ncols = A.desc[kCmMode];                                  // row 0, held to 3 .. 1 + Q by the check
  double *__restrict__ row = A.out + c * int64_t(ncols);
  if (flag) {
    if (tid == 0) A.status[c] = 1;
    for (int k = tid; k < ncols; k += kMtFinishLanes) row[k] = __builtin_nan("");
    return;
  }
  for (int at = wave; at <= A.nq; at += kMtFinishLanes / kWave) {     // one wave per (chain, sum)
    const double *part = A.part + (c * int64_t(A.nq + 1) + at) * int64_t(A.blocks);
    double r = 0;
    for (int b = lane; b < A.blocks; b += kWave) r += part[b];
    r = wave_sum(r);
    if (lane == 0) res[at] = r;
  }
  __syncthreads();
  for (int qid = tid; qid < A.nq; qid += kMtFinishLanes) {
    if (qid == 0) {
      A.status[c] = 0;
      row[0] = res[0];
      row[1] = res[kCmtPartialA4];
    } else {
      const int32_t *d = A.desc + size_t(qid) * kCmRow;
      if (d[kCmComp] == 0) row[d[kCmCol]] = d[kCmROnly] ? res[qid + 1] : res[qid + 1] + res[qid + 2];
    }
  }
}

template <typename T, int NP>
int mt_scatter(const char *what, const MtArgs &A, dim3 grid, hipStream_t s) {
  auto kern = modes_tiled_scatter_kernel<T, NP>;
  constexpr size_t lds = size_t(kMtTable) * (4 + 8 * size_t(NP));
  // per launch, as the one-CU kernels do: the attribute belongs to the current device
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)) != hipSuccess) {
    (void)hipGetLastError();
    set_error("%s: cannot raise the dynamic LDS limit to %zu B", what, lds);
    return NF_ELAUNCH;
  }
  hipLaunchKernelGGL(kern, grid, dim3(kMtLanes), lds, s, A);
  return check_launch(what);
}

template <typename T>
int mt_scatter_of(const char *what, const MtArgs &A, dim3 grid, hipStream_t s) {
  switch (A.nqp) {
#define NF_MT_CASE(n) case n: return mt_scatter<T, n>(what, A, grid, s);
    NF_MT_CASE(1) NF_MT_CASE(2) NF_MT_CASE(3) NF_MT_CASE(4) NF_MT_CASE(5) NF_MT_CASE(6) NF_MT_CASE(7) NF_MT_CASE(8)
    NF_MT_CASE(9) NF_MT_CASE(10) NF_MT_CASE(11) NF_MT_CASE(12) NF_MT_CASE(13) NF_MT_CASE(14) NF_MT_CASE(15) NF_MT_CASE(16)
#undef NF_MT_CASE
  }
  set_error("%s: no scatter kernel for a pass of %d quantities", what, A.nqp);
  return NF_EINVAL;
}

template <typename T>
int mt_launch(const char *what, MtArgs A, int64_t C, const MtPlan &p, hipStream_t s) {
  if (hipMemsetAsync(A.flags, 0, mt_flag_bytes(C), s) != hipSuccess) {
    (void)hipGetLastError();
    set_error("%s: cannot clear the flags of the workspace", what);
    return NF_ELAUNCH;
  }
  const dim3 grid(unsigned(p.blocks), unsigned(C)), lanes(kMtLanes);
  hipLaunchKernelGGL(modes_tiled_check_kernel<T>, grid, lanes, 0, s, A);
  int rc = check_launch(what);
  if (rc) return rc;
  for (int pass = 0; pass < p.passes; ++pass) {
    A.q0 = cmt_pass_first(pass, p.per_pass);
    A.nqp = cmt_pass_count(p.nq, pass, p.per_pass);
    if (hipMemsetAsync(A.slots, 0, size_t(A.nqp) * size_t(C) * size_t(p.V) * 8, s) != hipSuccess) {
      (void)hipGetLastError();
      set_error("%s: cannot clear the slots of the workspace", what);
      return NF_ELAUNCH;
    }
    if ((rc = mt_scatter_of<T>(what, A, grid, s))) return rc;
    hipLaunchKernelGGL(modes_tiled_squares_kernel, grid, lanes, 0, s, A);
    if ((rc = check_launch(what))) return rc;
  }
  hipLaunchKernelGGL(modes_tiled_finish_kernel, dim3(unsigned(C)), dim3(kMtFinishLanes), 0, s, A);
  return check_launch(what);
}

}  // namespace
}  // namespace nf

using namespace nf;

extern "C" int nf_cluster_modes_tiled_supported(const int32_t *lattice, int dtype, const int32_t *modes, int P,
                                                int64_t block_sites) {
  nf_modes_tiled_plan out;
  return nf_cluster_modes_tiled_plan(lattice, dtype, modes, P, block_sites, 0, &out) == NF_OK ? 1 : 0;
}

extern "C" int nf_cluster_modes_tiled_plan(const int32_t *lattice, int dtype, const int32_t *modes, int P, int64_t block_sites,
                                           int per_pass, nf_modes_tiled_plan *out) {
  const char *what = "nf_cluster_modes_tiled_plan";
  NF_REQUIRE(out != nullptr, "%s: out is NULL", what);
  int Q = 0, N = 0;
  int rc = mt_list(what, lattice, modes, P, &Q, &N);
  if (rc) return rc;
  MtPlan p;
  rc = mt_plan(what, lattice, dtype, Q, block_sites, per_pass, p);
  if (rc) return rc;
  out->blocks = p.blocks;
  out->block_sites = p.bs;
  out->N = p.N;
  out->columns = 2 + P;
  out->quantities = p.nq;
  out->per_pass = p.per_pass;
  out->passes = p.passes;
  out->table_entries = kMtTable;
  out->launches = 2 + 2 * p.passes;
  out->lds_bytes = int64_t(p.lds);
  return NF_OK;
}

extern "C" size_t nf_cluster_modes_tiled_workspace(int64_t C, const int32_t *lattice, int Q, int64_t block_sites, int per_pass) {
  MtPlan p;
  if (C < 1 || C > 65535 || mt_plan("nf_cluster_modes_tiled_workspace", lattice, NF_F32, Q, block_sites, per_pass, p) != NF_OK)
    return 0;
  return mt_workspace(C, p);
}

extern "C" int nf_cluster_modes_tiled(const void *phi, const int32_t *labels, double *out, int32_t *status, int64_t C,
                                      const int32_t *lattice, const int32_t *desc, int Q, const double *twN, int N, int dtype,
                                      int64_t block_sites, int per_pass, void *workspace, size_t workspace_bytes, void *stream) {
  const char *what = "nf_cluster_modes_tiled";
  NF_REQUIRE(phi && labels && out && status, "%s: phi, labels, out or status is NULL", what);
  NF_REQUIRE(desc != nullptr, "%s: desc is NULL", what);
  NF_REQUIRE(twN != nullptr, "%s: twN is NULL", what);
  NF_REQUIRE(C >= 1 && C <= 65535, "%s: C (%lld) must be in 1 .. 65535", what, (long long)C);
  MtPlan p;
  const int rc = mt_plan(what, lattice, dtype, Q, block_sites, per_pass, p);
  if (rc) return rc;
  NF_REQUIRE(N == p.N, "%s: N (%d) is not the lcm of the lattice's extents (%d)", what, N, p.N);
  const size_t need = mt_workspace(C, p);
  NF_REQUIRE(workspace != nullptr, "%s: workspace is NULL (%zu B needed)", what, need);
  NF_REQUIRE(workspace_bytes >= need, "%s: workspace of %zu B is too small, %zu B needed", what, workspace_bytes, need);
  NF_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % kMtAlign == 0, "%s: workspace is not aligned to %zu B", what, kMtAlign);
  MtArgs A{};
  A.phi = phi; A.labels = labels; A.out = out; A.status = status; A.tw = twN; A.desc = desc;
  unsigned char *w = static_cast<unsigned char *>(workspace);
  A.flags = reinterpret_cast<int *>(w);
  A.slots = reinterpret_cast<unsigned long long *>(w + mt_flag_bytes(C));
  A.part = reinterpret_cast<double *>(w + mt_flag_bytes(C) + mt_slot_bytes(C, p));
  A.V = int(p.V); A.bs = p.bs; A.blocks = int(p.blocks); A.C = int(C); A.nq = p.nq; A.N = p.N;
  A.magic = cmt_magic(uint32_t(p.N));
  for (int mu = 0; mu < 4; ++mu) A.extent[mu] = p.extent[mu];
  A.limit = p.limit;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return dtype == NF_F32 ? mt_launch<float>(what, A, C, p, s) : mt_launch<double>(what, A, C, p, s);
}

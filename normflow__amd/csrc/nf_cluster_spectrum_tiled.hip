// nf_cluster_spectrum_tiled.hip -- the cluster spectrum for chains that live in HBM (MI355X-side extension, no counterpart
// in the reference): nf_cluster_spectrum's rule (include/normflow_hip.h, "cluster spectrum") for lattices beyond one CU's
// LDS, with the int64 slots in a workspace in HBM and nf_cluster_moments_tiled's order of the sums of squares.
// The structure is nf_cluster_moments_tiled.hip's.  A chain is cut into blocks of `block_sites` consecutive sites (and
// slots); the grid of the three site kernels is (blocks, C) with 256 lanes, lane tid of a block owns the sites
// first + tid + 256 k.  On `stream`:
//   memset of the flags | CHECK: range and label test of every site, a refused chain's flag set (one atomicOr per block)
//   per pass of up to `per_pass` <= 16 quantities:
//     memset of the pass's slot arrays
//     SCATTER: every site's q of every quantity of the pass to the slot of its label, through the claim-add-flush table of
//              nf_cluster_table.h in dynamic LDS (H = 512 entries, 512 (4 + 8 per_pass) bytes)
//     SQUARES: per block and quantity, lane l squares the slots first + l + 256 k (fma), wave shuffle tree, the 4 waves in
//              order -> the block's partial in the workspace
//   FINISH: one wave per (chain, sum) adds the blocks' partials (lane l the blocks l, l + 64, ... in order, shuffle tree),
//           then the row: columns 0 and 1, per (mu, k) sum r^2 + sum i^2, at Nyquist sum r^2 alone; or NaNs; and status.
// The quantities of a pass are consecutive indices q0 .. q0 + n - 1.  Their descriptors (nf_cluster_spectrum_core.h) are
// wave-uniform and are worked out in front of the site loop; a site is read ONCE per pass, its coordinate x_mu is taken
// once per axis of the pass, and the twiddle index k x_mu mod L_mu of consecutive k of one axis follows by one add and one
// conditional subtract from the one before (a multiplication and a division only for the first quantity of a pass).
// The scatter kernel is instantiated for every pass size NP = 1 .. 16: a pass of n quantities carries n descriptors and n
// run sums, picked with constant indices out of unrolled loops: nothing in registers is indexed dynamically, so there
// is no scratch.
#include "nf_internal.h"
#include "nf_cluster_spectrum_core.h"
#include "nf_cluster_table.h"

namespace nf {
namespace {

constexpr int kStLanes = 256;
constexpr int kStWaves = kStLanes / kWave;
constexpr int kStMaxPass = 16;                     // quantities per pass: nf_cluster_spectrum's cap, a lane's sums in registers
constexpr int kStMaxQ = 1024;                      // bounds the launches (2 + 2 passes) and the partials
constexpr int kStDefaultBlockSites = 4096;         // nf_cluster_moments_tiled's
constexpr int kStTable = 512;                      // H: entries of the table
constexpr int kStFinishLanes = 1024;
constexpr size_t kStAlign = 16;
constexpr size_t kStLdsBudget = size_t(kStTable) * (4 + 8 * kStMaxPass);        // 66 KiB
static_assert((kStTable & (kStTable - 1)) == 0, "entry h = label & (H - 1)");
static_assert(kStLdsBudget <= 160 * 1024, "the table fits the LDS of a CU");

struct StPlan : CsLayout {
  int64_t V, blocks;
  int bs, per_pass, passes;
  size_t lds;
  double limit;                  // 2^min(16, 30 - ceil(log2 V))
};

int st_plan(const char *what, const int32_t *lattice, int dtype, int kmax, int64_t block_sites, int per_pass, StPlan &p) {
  NF_REQUIRE(lattice != nullptr, "%s: lattice is NULL", what);
  NF_REQUIRE(dtype == NF_F32 || dtype == NF_F64, "%s: unsupported dtype %d", what, dtype);
  NF_REQUIRE(kmax >= 0, "%s: kmax (%d) must be >= 0 (0: all momenta)", what, kmax);
  p.V = 1;
  for (int mu = 0; mu < 4; ++mu) {
    NF_REQUIRE(lattice[mu] >= 1, "%s: lattice extents must be >= 1", what);
    p.V *= lattice[mu];
    NF_REQUIRE(p.V < (int64_t(1) << 31), "%s: the lattice (%d, %d, %d, %d) has 2^31 sites or more", what, lattice[0], lattice[1],
               lattice[2], lattice[3]);
  }
  NF_REQUIRE(block_sites >= 0, "%s: block_sites (%lld) must be 0 (the default, %d) or >= 1", what, (long long)block_sites,
             kStDefaultBlockSites);
  const int64_t bs = block_sites ? block_sites : kStDefaultBlockSites;
  p.bs = int(bs < p.V ? bs : p.V);
  p.blocks = (p.V + p.bs - 1) / p.bs;
  NF_REQUIRE(p.blocks * kStLanes < (int64_t(1) << 32),
             "%s: %lld blocks of %d sites are more than one launch takes (blocks x lanes < 2^32)", what, (long long)p.blocks, p.bs);
  // Q before the layout's ints could overflow: an axis gives at most L quantities
  int64_t nq = 1;
  for (int mu = 0; mu < 4; ++mu) {
    const int64_t L = lattice[mu], K = L == 1 ? 0 : (kmax == 0 || kmax > L / 2 ? L / 2 : kmax);
    nq += 2 * K - (K > 0 && 2 * K == L ? 1 : 0);
  }
  NF_REQUIRE(nq <= kStMaxQ,
             "%s: the lattice (%d, %d, %d, %d) has %lld quantities at kmax = %d, more than %d: give a smaller kmax (> 0)", what,
             lattice[0], lattice[1], lattice[2], lattice[3], (long long)nq, kmax, kStMaxQ);
  cs_layout(lattice, kmax, p.V, p);
  const int cap = p.nq < kStMaxPass ? p.nq : kStMaxPass;
  NF_REQUIRE(per_pass >= 0 && per_pass <= cap,
             "%s: per_pass (%d) must be 0 (as many as fit) or 1 .. %d, the smaller of the quantities and %d", what, per_pass, cap,
             kStMaxPass);
  p.per_pass = per_pass ? per_pass : cap;
  p.passes = (p.nq + p.per_pass - 1) / p.per_pass;
  p.lds = size_t(kStTable) * (4 + 8 * size_t(p.per_pass));
  int lg = 0;
  while ((int64_t(1) << lg) < p.V) ++lg;
  const int e = 30 - lg < 16 ? 30 - lg : 16;
  p.limit = e >= 0 ? double(int64_t(1) << e) : 1.0 / double(int64_t(1) << -e);
  return NF_OK;
}

size_t st_flag_bytes(int64_t C) { return (size_t(C) * 4 + kStAlign - 1) & ~(kStAlign - 1); }
size_t st_slot_bytes(int64_t C, const StPlan &p) { return size_t(p.per_pass) * size_t(C) * size_t(p.V) * 8; }
size_t st_workspace(int64_t C, const StPlan &p) {
  return st_flag_bytes(C) + st_slot_bytes(C, p) + size_t(C) * size_t(p.nq + 1) * size_t(p.blocks) * sizeof(double);
}

struct StArgs {
  const void *phi;
  const int32_t *labels;
  double *out;
  int32_t *status;
  const double *tw;
  int *flags;                    // [C]: the chain is refused
  unsigned long long *slots;     // [per_pass][C][V]
  double *part;                  // [C][Q + 1][blocks]: a^2, a^4, then one sum per further quantity
  int V, bs, blocks, C, nq, ncols;
  int q0, nqp;                   // the pass: quantities q0 .. q0 + nqp - 1
  int stride[4], extent[4], off[4], qpre[4], cpre[4];
  double limit;
};

struct StDeviceTable {
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

// k x mod L for k <= kStMaxQ / 2 = 2^9 and x < L < 2^31: 32-bit where the product fits
__device__ __forceinline__ unsigned st_mulmod(unsigned k, unsigned x, unsigned L) {
  return L <= (1u << 22) ? (k * x) % L : unsigned((static_cast<unsigned long long>(k) * x) % L);
}

// ---------------------------------------------------------------- check: before anything is indexed by a label
template <typename T>
__global__ __launch_bounds__(kStLanes) void spectrum_tiled_check_kernel(StArgs A) {
  const int V = A.V;
  const int64_t c = blockIdx.y;
  const int64_t first = int64_t(blockIdx.x) * A.bs;
  const int64_t last = first + A.bs < V ? first + A.bs : int64_t(V);
  const T *__restrict__ gphi = static_cast<const T *>(A.phi) + c * int64_t(V);
  const int32_t *__restrict__ glab = A.labels + c * int64_t(V);
  int bad = 0;
  for (int64_t x = first + threadIdx.x; x < last; x += kStLanes) {
    const int l = glab[x];
    if (!(fabs(double(gphi[x])) < A.limit) || l < 0 || l >= V) bad = 1;
  }
  bad = __syncthreads_or(bad);
  if (bad && threadIdx.x == 0) atomicOr(&A.flags[c], 1);
}

// ---------------------------------------------------------------- scatter: every site's q to the slot of its label
// how quantity j of the pass gets its twiddle index from the one before it
enum { kStSame = 0, kStNext = 1, kStFresh = 2, kStPlain = 3 };      // the same k | k + 1 of the axis | anew | A: no twiddle

// NP: the quantities of the pass, a compile-time number, so that a pass of n quantities carries n descriptors and n sums
template <typename T, int NP>
__global__ __launch_bounds__(kStLanes) void spectrum_tiled_scatter_kernel(StArgs A) {
  extern __shared__ __align__(16) unsigned char st_lds[];
  const int tid = threadIdx.x, V = A.V, H = kStTable;
  constexpr int nqp = NP;
  unsigned long long *sums = reinterpret_cast<unsigned long long *>(st_lds);          // [nqp][H]
  int *keys = reinterpret_cast<int *>(st_lds + size_t(nqp) * H * 8);                   // [H]
  const int64_t c = blockIdx.y;
  if (A.flags[c]) return;                                             // final since the check ended; the same in every lane
  const int64_t first = int64_t(blockIdx.x) * A.bs;
  const int64_t last = first + A.bs < V ? first + A.bs : int64_t(V);
  const T *__restrict__ gphi = static_cast<const T *>(A.phi) + c * int64_t(V);
  const int32_t *__restrict__ glab = A.labels + c * int64_t(V);
  const double *__restrict__ tw = A.tw;
  const int64_t qstride = int64_t(A.C) * V;                           // between the slot arrays of two quantities
  unsigned long long *slots = A.slots + c * int64_t(V);               // of quantity q0

  table_clear<StDeviceTable>(keys, sums, H, nqp, tid, kStLanes);

  // ---- the pass's descriptors, wave-uniform, in front of the site loop
  int how[NP];                                                        // kSt... | the axis << 2
  unsigned two[NP];                                                   // its first double in tw: 2 off_mu + component
  int k0 = 0;                                                         // the k of the pass's first quantity with a twiddle
  int alo = 4, ahi = -1;                                              // the axes of the pass
  {
    int pa = -1, pk = 0;
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      how[j] = kStPlain; two[j] = 0;
      const int qid = A.q0 + j;
      if (qid > 0) {
        const CsQuantity d = cs_quantity(A, qid);
        two[j] = 2u * unsigned(d.off) + unsigned(d.comp);
        how[j] = (d.axis == pa && d.k == pk ? kStSame : d.axis == pa && d.k == pk + 1 ? kStNext : kStFresh) | d.axis << 2;
        if (pa < 0) { k0 = d.k; alo = d.axis; }                       // every later kStFresh is an axis' k = 1
        pa = d.axis; pk = d.k; ahi = d.axis;
      }
    }
  }
  __syncthreads();

  int run = -1;                         // the label of the lane's current run of sites, and their sums
  long long sum[NP];
#pragma unroll
  for (int j = 0; j < NP; ++j) sum[j] = 0;
  auto commit = [&]() {
    const int h = table_claim<StDeviceTable>(keys, H, run);
#pragma unroll
    for (int j = 0; j < NP; ++j)
      table_add<StDeviceTable>(sums, H, h, j, slots + j * qstride, run, sum[j]);
  };
  for (int64_t xx = first + tid; xx < last; xx += kStLanes) {
    const int x = int(xx);
    const int l = glab[x];
    const double w = double(gphi[x]);
    if (l != run) {
      if (run >= 0) commit();
      run = l;
#pragma unroll
      for (int j = 0; j < NP; ++j) sum[j] = 0;
    }
    unsigned xm[4];                                                   // x_mu, once per axis of the pass
#pragma unroll
    for (int mu = 0; mu < 4; ++mu)
      xm[mu] = mu >= alo && mu <= ahi ? (unsigned(x) / unsigned(A.stride[mu])) % unsigned(A.extent[mu]) : 0u;
    unsigned t = 0;                                                   // k x_mu mod L_mu of the quantity in hand
    bool seen = false;                                                // a quantity with a twiddle came before
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      double v = w;
      if (how[j] != kStPlain) {
        const int mu = how[j] >> 2, step = how[j] & 3;
        const unsigned xa = mu == 1 ? xm[1] : mu == 2 ? xm[2] : mu == 3 ? xm[3] : xm[0];
        const unsigned L = unsigned(mu == 1 ? A.extent[1] : mu == 2 ? A.extent[2] : mu == 3 ? A.extent[3] : A.extent[0]);
        if (step == kStFresh) {
          t = seen || k0 == 1 ? xa : st_mulmod(unsigned(k0), xa, L);
        } else if (step == kStNext) {
          t += xa;                                                    // both below L < 2^31
          if (t >= L) t -= L;
        }
        seen = true;
        v = w * tw[size_t(two[j]) + 2 * size_t(t)];
      }
      sum[j] += static_cast<long long>(rint(v * 4294967296.0));
    }
  }
  if (run >= 0) commit();
  __syncthreads();
  table_flush<StDeviceTable>(keys, sums, H, nqp, slots, qstride, tid, kStLanes);
}

// ---------------------------------------------------------------- squares: the blocks' partials
__global__ __launch_bounds__(kStLanes) void spectrum_tiled_squares_kernel(StArgs A) {
  __shared__ double red[kStWaves][kStMaxPass + 1];                    // the pass's sums, and a^4 of quantity 0 in the last
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
    for (int64_t s = first + tid; s < last; s += kStLanes) {
      const long long v = static_cast<long long>(slot[s]);
      const double a = double(v) * 0x1p-32, a2 = a * a;
      s2 = fma(a, a, s2);
      if (qid == 0) s4 = fma(a2, a2, s4);
    }
    s2 = wave_sum(s2);
    if (qid == 0) s4 = wave_sum(s4);
    if (lane == 0) {
      red[wave][j] = s2;
      if (qid == 0) red[wave][kStMaxPass] = s4;
    }
  }
  __syncthreads();
  if (tid < A.nqp || (tid == kStMaxPass && A.q0 == 0)) {
    double r = 0;
#pragma unroll
    for (int w = 0; w < kStWaves; ++w) r += red[w][tid];
    const int qid = A.q0 + tid;                                       // the sum's place: a^2, a^4, then quantity q at q + 1
    const int at = tid == kStMaxPass ? 1 : qid ? qid + 1 : 0;
    A.part[(c * int64_t(A.nq + 1) + at) * int64_t(A.blocks) + blockIdx.x] = r;
  }
}

// ---------------------------------------------------------------- finish: the blocks in order, the row, status
__global__ __launch_bounds__(kStFinishLanes) void spectrum_tiled_finish_kernel(StArgs A) {
  __shared__ double res[kStMaxQ + 1];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int64_t c = blockIdx.x;
  double *__restrict__ row = A.out + c * int64_t(A.ncols);
  if (A.flags[c]) {
    if (tid == 0) A.status[c] = 1;
    for (int k = tid; k < A.ncols; k += kStFinishLanes) row[k] = __builtin_nan("");
    return;
  }
  for (int at = wave; at <= A.nq; at += kStFinishLanes / kWave) {     // one wave per (chain, sum)
    const double *part = A.part + (c * int64_t(A.nq + 1) + at) * int64_t(A.blocks);
    double r = 0;
    for (int b = lane; b < A.blocks; b += kWave) r += part[b];
    r = wave_sum(r);
    if (lane == 0) res[at] = r;
  }
  __syncthreads();
  for (int qid = tid; qid < A.nq; qid += kStFinishLanes) {
    if (qid == 0) {
      A.status[c] = 0;
      row[0] = res[0];
      row[1] = res[1];
    } else {
      const CsQuantity d = cs_quantity(A, qid);
      if (d.comp == 0) row[d.col] = d.nyquist ? res[qid + 1] : res[qid + 1] + res[qid + 2];
    }
  }
}

template <typename T, int NP>
int st_scatter(const char *what, const StArgs &A, dim3 grid, hipStream_t s) {
  auto kern = spectrum_tiled_scatter_kernel<T, NP>;
  constexpr size_t lds = size_t(kStTable) * (4 + 8 * size_t(NP));
  // per launch, as the one-CU kernels do: the attribute belongs to the current device
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)) != hipSuccess) {
    (void)hipGetLastError();
    set_error("%s: cannot raise the dynamic LDS limit to %zu B", what, lds);
    return NF_ELAUNCH;
  }
  hipLaunchKernelGGL(kern, grid, dim3(kStLanes), lds, s, A);
  return check_launch(what);
}

template <typename T>
int st_scatter_of(const char *what, const StArgs &A, dim3 grid, hipStream_t s) {
  switch (A.nqp) {
#define NF_ST_CASE(n) case n: return st_scatter<T, n>(what, A, grid, s);
    NF_ST_CASE(1) NF_ST_CASE(2) NF_ST_CASE(3) NF_ST_CASE(4) NF_ST_CASE(5) NF_ST_CASE(6) NF_ST_CASE(7) NF_ST_CASE(8)
    NF_ST_CASE(9) NF_ST_CASE(10) NF_ST_CASE(11) NF_ST_CASE(12) NF_ST_CASE(13) NF_ST_CASE(14) NF_ST_CASE(15) NF_ST_CASE(16)
#undef NF_ST_CASE
  }
  set_error("%s: no scatter kernel for a pass of %d quantities", what, A.nqp);
  return NF_EINVAL;
}

template <typename T>
int st_launch(const char *what, StArgs A, int64_t C, const StPlan &p, hipStream_t s) {
  if (hipMemsetAsync(A.flags, 0, st_flag_bytes(C), s) != hipSuccess) {
    (void)hipGetLastError();
    set_error("%s: cannot clear the flags of the workspace", what);
    return NF_ELAUNCH;
  }
  const dim3 grid(unsigned(p.blocks), unsigned(C)), lanes(kStLanes);
  hipLaunchKernelGGL(spectrum_tiled_check_kernel<T>, grid, lanes, 0, s, A);
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
    if ((rc = st_scatter_of<T>(what, A, grid, s))) return rc;
    hipLaunchKernelGGL(spectrum_tiled_squares_kernel, grid, lanes, 0, s, A);
    if ((rc = check_launch(what))) return rc;
  }
  hipLaunchKernelGGL(spectrum_tiled_finish_kernel, dim3(unsigned(C)), dim3(kStFinishLanes), 0, s, A);
  return check_launch(what);
}

void st_fill_plan(const StPlan &p, nf_spectrum_tiled_plan *out) {
  out->blocks = p.blocks;
  out->block_sites = p.bs;
  for (int mu = 0; mu < 4; ++mu) out->kmax[mu] = p.K[mu];
  out->columns = p.ncols;
  out->quantities = p.nq;
  out->per_pass = p.per_pass;
  out->passes = p.passes;
  out->table_entries = kStTable;
  out->launches = 2 + 2 * p.passes;
  out->lds_bytes = int64_t(p.lds);
}

}  // namespace
}  // namespace nf

using namespace nf;

extern "C" int nf_cluster_spectrum_tiled_supported(const int32_t *lattice, int dtype, int kmax, int64_t block_sites) {
  StPlan p;
  return st_plan("nf_cluster_spectrum_tiled_supported", lattice, dtype, kmax, block_sites, 0, p) == NF_OK ? 1 : 0;
}

extern "C" int nf_cluster_spectrum_tiled_plan(const int32_t *lattice, int dtype, int kmax, int64_t block_sites, int per_pass,
                                              nf_spectrum_tiled_plan *out) {
  NF_REQUIRE(out != nullptr, "nf_cluster_spectrum_tiled_plan: out is NULL");
  StPlan p;
  const int rc = st_plan("nf_cluster_spectrum_tiled_plan", lattice, dtype, kmax, block_sites, per_pass, p);
  if (rc) return rc;
  st_fill_plan(p, out);
  return NF_OK;
}

extern "C" size_t nf_cluster_spectrum_tiled_workspace(int64_t C, const int32_t *lattice, int kmax, int64_t block_sites,
                                                      int per_pass) {
  StPlan p;
  if (C < 1 || C > 65535 ||
      st_plan("nf_cluster_spectrum_tiled_workspace", lattice, NF_F32, kmax, block_sites, per_pass, p) != NF_OK)
    return 0;
  return st_workspace(C, p);
}

extern "C" int nf_cluster_spectrum_tiled(const void *phi, const int32_t *labels, double *out, int32_t *status, int64_t C,
                                         const int32_t *lattice, int kmax, const double *tw, int dtype, int64_t block_sites,
                                         int per_pass, void *workspace, size_t workspace_bytes, void *stream) {
  const char *what = "nf_cluster_spectrum_tiled";
  NF_REQUIRE(phi && labels && out && status, "%s: phi, labels, out or status is NULL", what);
  NF_REQUIRE(tw != nullptr, "%s: tw is NULL", what);
  NF_REQUIRE(C >= 1 && C <= 65535, "%s: C (%lld) must be in 1 .. 65535", what, (long long)C);
  StPlan p;
  const int rc = st_plan(what, lattice, dtype, kmax, block_sites, per_pass, p);
  if (rc) return rc;
  const size_t need = st_workspace(C, p);
  NF_REQUIRE(workspace != nullptr, "%s: workspace is NULL (%zu B needed)", what, need);
  NF_REQUIRE(workspace_bytes >= need, "%s: workspace of %zu B is too small, %zu B needed", what, workspace_bytes, need);
  NF_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % kStAlign == 0, "%s: workspace is not aligned to %zu B", what, kStAlign);
  StArgs A{};
  A.phi = phi; A.labels = labels; A.out = out; A.status = status; A.tw = tw;
  unsigned char *w = static_cast<unsigned char *>(workspace);
  A.flags = reinterpret_cast<int *>(w);
  A.slots = reinterpret_cast<unsigned long long *>(w + st_flag_bytes(C));
  A.part = reinterpret_cast<double *>(w + st_flag_bytes(C) + st_slot_bytes(C, p));
  A.V = int(p.V); A.bs = p.bs; A.blocks = int(p.blocks); A.C = int(C); A.nq = p.nq; A.ncols = p.ncols;
  for (int mu = 0; mu < 4; ++mu) {
    A.stride[mu] = p.stride[mu]; A.extent[mu] = p.extent[mu]; A.off[mu] = p.off[mu];
    A.qpre[mu] = p.qpre[mu]; A.cpre[mu] = p.cpre[mu];
  }
  A.limit = p.limit;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return dtype == NF_F32 ? st_launch<float>(what, A, C, p, s) : st_launch<double>(what, A, C, p, s);
}

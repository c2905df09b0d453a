// nf_cluster_moments.hip -- the per-cluster sums behind the cluster-improved estimators (MI355X-side extension, no
// counterpart in the reference).  The rule -- the fixed point q, the range test, the sums A, R, I and the order of the
// sums of squares -- is stated once in include/normflow_hip.h, "cluster-improved estimators".
// One workgroup per chain, for the lattices of nf_phi4_cluster, with its lane map: lane `tid` of the NT lanes owns the
// sites tid + k NT (k < NS) and keeps their phi and labels in registers.  LDS holds 2 KiB of reduction slots and, behind
// them, `per_pass` arrays of V int64 slots.  A pass:
//   zero the arrays | barrier | for every quantity of the pass, for every site: q -> the slot of the site's label (64-bit
//   integer LDS add) | barrier | for every quantity: lane l squares the slots l, l + NT, ... (fma), wave shuffle tree, the
//   wave's sum into its own column of the reduction slots | barrier.
// After the last pass the waves' sums are added in wave order and thread 0 writes the row.  The quantity loop is a runtime
// loop and everything that depends on the quantity is wave-uniform (stride, extent and twiddle offset of its axis, picked
// by a chain of selects with constant indices): nothing in registers is indexed dynamically, so there is no scratch.
// Contention: in the ordered phase one cluster holds 0.95 of the lattice, so most adds of a wave go to one slot.  A lane
// therefore adds up the consecutive sites of its own that share a label in a register and issues one atomic per run:
// with the lane map's stride between a lane's sites, the sites of the giant cluster are almost always one run, NS times
// fewer atomics, while a lattice of small clusters pays a compare per site.  The sums are integers: every grouping gives
// the same bits.  The kernel has no static LDS, so that the dynamic limit of 160 KiB stays reachable.
// The label and range checks come first, for the whole chain, before any slot is touched: a refused chain gets status 1,
// a NaN row and a zero moments row, and its workgroup leaves.
#include "nf_internal.h"

namespace nf {
namespace {

constexpr int kCmMaxLanes = 1024;
constexpr int kCmMaxQ = 9;                         // 1 + 2 x 4 axes
constexpr int kCmCols = kCmMaxQ + 1;               // sums of squares: a^2, a^4, then r^2 and i^2 of every axis
constexpr int kCmWaves = kCmMaxLanes / kWave;
constexpr size_t kCmScratch = 2048;                // kCmWaves x kCmCols doubles of wave sums, kCmCols results, the flag
constexpr size_t kCmLdsBudget = 160 * 1024;
static_assert((kCmWaves * kCmCols + kCmCols + 1) * sizeof(double) <= kCmScratch, "reduction slots");

struct CmQuantity {
  int stride, extent, tw;        // of the quantity's axis: site stride, extent, the index of its first double in tw
};

struct CmPlan {
  int64_t V;
  int ns, nt, nq, per_pass, passes;
  CmQuantity q[kCmMaxQ];         // q[0] is A (no twiddle)
  int col[4];                    // column of sum r^2 of axis mu among the sums of squares (i^2 is the next), -1: extent 1
  size_t lds;
  double limit;                  // 2^min(16, 30 - ceil(log2 V))
};

int cm_plan(const char *what, const int32_t *lattice, int dtype, CmPlan &p) {
  NF_REQUIRE(lattice != nullptr, "%s: lattice is NULL", what);
  NF_REQUIRE(dtype == NF_F32 || dtype == NF_F64, "%s: unsupported dtype %d", what, dtype);
  for (int mu = 0; mu < 4; ++mu) NF_REQUIRE(lattice[mu] >= 1, "%s: lattice extents must be >= 1", what);
  nf_cluster_plan cp;
  if (nf_phi4_cluster_plan(lattice, dtype, &cp) != NF_OK) {
    set_error("%s: a chain of the lattice (%d, %d, %d, %d) is outside the class of nf_phi4_cluster (V sizeof <= 64 KiB)", what,
              lattice[0], lattice[1], lattice[2], lattice[3]);
    return NF_EINVAL;
  }
  p.V = int64_t(lattice[0]) * lattice[1] * lattice[2] * lattice[3];
  p.ns = cp.sites_per_lane;
  p.nt = cp.lanes;
  p.nq = 1;
  p.q[0] = CmQuantity{1, 1, 0};
  int stride = int(p.V), off = 0;
  for (int mu = 0; mu < 4; ++mu) {
    stride /= lattice[mu];
    p.col[mu] = -1;
    if (lattice[mu] > 1) {
      p.col[mu] = p.nq + 1;
      p.q[p.nq++] = CmQuantity{stride, lattice[mu], 2 * off};
      p.q[p.nq++] = CmQuantity{stride, lattice[mu], 2 * off + 1};
    }
    off += lattice[mu];
  }
  for (int k = p.nq; k < kCmMaxQ; ++k) p.q[k] = CmQuantity{1, 1, 0};
  const size_t fit = (kCmLdsBudget - kCmScratch) / (size_t(p.V) * 8);      // >= 1: V <= 16384
  p.per_pass = int(fit < size_t(p.nq) ? fit : size_t(p.nq));
  p.passes = (p.nq + p.per_pass - 1) / p.per_pass;
  p.lds = kCmScratch + size_t(p.per_pass) * size_t(p.V) * 8;
  int lg = 0;
  while ((int64_t(1) << lg) < p.V) ++lg;
  const int e = 30 - lg < 16 ? 30 - lg : 16;
  p.limit = e >= 0 ? double(int64_t(1) << e) : 1.0 / double(int64_t(1) << -e);
  return NF_OK;
}

struct CmArgs {
  const void *phi;
  const int32_t *labels;
  double *out;
  int32_t *status;
  int64_t *moments;
  const double *tw;
  int V, nq, per_pass;
  int col[4];
  CmQuantity q[kCmMaxQ];
  double limit;
};

template <typename T, int NS>
__global__ __launch_bounds__(kCmMaxLanes) void cluster_moments_kernel(CmArgs A) {
  extern __shared__ __align__(16) unsigned char cm_lds[];
  double *red = reinterpret_cast<double *>(cm_lds);                 // [wave][kCmCols]
  double *res = red + kCmWaves * kCmCols;                           // [kCmCols]
  volatile int *s_bad = reinterpret_cast<volatile int *>(res + kCmCols);      // the chain is refused
  unsigned long long *slots = reinterpret_cast<unsigned long long *>(cm_lds + kCmScratch);
  const int tid = threadIdx.x, NT = blockDim.x, V = A.V;
  const int lane = tid & (kWave - 1), wave = tid / kWave;
  const int64_t c = blockIdx.x;
  const T *__restrict__ gphi = static_cast<const T *>(A.phi) + c * int64_t(V);
  const int32_t *__restrict__ glab = A.labels + c * int64_t(V);
  const double *__restrict__ tw = A.tw;

  // ---- the chain into registers, and the two checks: before any indexed access
  T phi[NS];
  int lab[NS];
  int bad = 0;
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    const int x = tid + k * NT;
    phi[k] = T(0);
    lab[k] = 0;
    if (x < V) {
      phi[k] = gphi[x];
      lab[k] = glab[x];
      if (!(fabs(double(phi[k])) < A.limit) || lab[k] < 0 || lab[k] >= V) bad = 1;
    }
  }
  if (tid == 0) *s_bad = 0;
  __syncthreads();
  if (bad) *s_bad = 1;
  __syncthreads();
  if (*s_bad) {                                                      // the same in every lane
    if (A.moments)
      for (int s = tid; s < V; s += NT) A.moments[c * int64_t(V) + s] = 0;
    if (tid == 0) {
      A.status[c] = 1;
#pragma unroll
      for (int k = 0; k < 6; ++k) A.out[6 * c + k] = __builtin_nan("");
    }
    return;
  }

  for (int q0 = 0; q0 < A.nq; q0 += A.per_pass) {
    const int nqp = min(A.per_pass, A.nq - q0);
    for (int s = tid; s < nqp * V; s += NT) slots[s] = 0;
    __syncthreads();

    // ---- the sums: every site's term to the slot of its label
#pragma unroll 1
    for (int j = 0; j < nqp; ++j) {
      const int qid = q0 + j;
      int stride = 1, extent = 1, two = 0;
#pragma unroll
      for (int k = 0; k < kCmMaxQ; ++k)
        if (k == qid) { stride = A.q[k].stride; extent = A.q[k].extent; two = A.q[k].tw; }
      unsigned long long *slot = slots + size_t(j) * V;
      int run = -1;                     // the label of the lane's current run of sites, and their sum
      long long sum = 0;
#pragma unroll
      for (int k = 0; k < NS; ++k) {
        const int x = tid + k * NT;
        if (x < V) {
          double w = double(phi[k]);
          if (qid) w *= tw[two + 2 * int((unsigned(x) / unsigned(stride)) % unsigned(extent))];
          const long long q = static_cast<long long>(rint(w * 4294967296.0));
          if (lab[k] == run) {
            sum += q;
          } else {
            if (run >= 0) atomicAdd(&slot[run], static_cast<unsigned long long>(sum));
            run = lab[k];
            sum = q;
          }
        }
      }
      if (run >= 0) atomicAdd(&slot[run], static_cast<unsigned long long>(sum));
    }
    __syncthreads();

    // ---- the squares: lane l takes the slots l, l + NT, ...
#pragma unroll 1
    for (int j = 0; j < nqp; ++j) {
      const int qid = q0 + j;
      const unsigned long long *slot = slots + size_t(j) * V;
      double s2 = 0, s4 = 0;
      for (int s = tid; s < V; s += NT) {
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
        red[wave * kCmCols + (qid ? qid + 1 : 0)] = s2;
        if (qid == 0) red[wave * kCmCols + 1] = s4;
      }
    }
    __syncthreads();
  }

  // ---- the waves in order, then the row
  if (tid <= A.nq) {
    double r = 0;
    for (int w = 0; w < NT / kWave; ++w) r += red[w * kCmCols + tid];
    res[tid] = r;
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

template <typename T, int NS>
int cm_launch(const CmArgs &A, int64_t C, const CmPlan &p, hipStream_t s) {
  auto kern = cluster_moments_kernel<T, NS>;
  // per launch, as nf_phi4_cluster does: the attribute belongs to the current device, and always to the budget, so that no
  // call lowers what another raised
  if (p.lds > 64 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                          int(kCmLdsBudget)) != hipSuccess) {
    (void)hipGetLastError();
    set_error("nf_cluster_moments: cannot raise the dynamic LDS limit to %zu B", kCmLdsBudget);
    return NF_ELAUNCH;
  }
  hipLaunchKernelGGL(kern, dim3(unsigned(C)), dim3(unsigned(p.nt)), p.lds, s, A);
  return check_launch("nf_cluster_moments");
}

template <typename T>
int cm_dispatch(const CmArgs &A, int64_t C, const CmPlan &p, hipStream_t s) {
  switch (p.ns) {
    case 1: return cm_launch<T, 1>(A, C, p, s);
    case 2: return cm_launch<T, 2>(A, C, p, s);
    case 4: return cm_launch<T, 4>(A, C, p, s);
    case 8: return cm_launch<T, 8>(A, C, p, s);
    case 16:
      if constexpr (sizeof(T) == 4) return cm_launch<T, 16>(A, C, p, s);     // 8-byte fields end at 8 sites per lane
  }
  set_error("nf_cluster_moments: no kernel for %d sites per lane", p.ns);
  return NF_EINVAL;
}

}  // namespace
}  // namespace nf

using namespace nf;

extern "C" int nf_cluster_moments_supported(const int32_t *lattice, int dtype) {
  CmPlan p;
  return cm_plan("nf_cluster_moments_supported", lattice, dtype, p) == NF_OK ? 1 : 0;
}

extern "C" int nf_cluster_moments_plan(const int32_t *lattice, int dtype, nf_moments_plan *out) {
  NF_REQUIRE(out != nullptr, "nf_cluster_moments_plan: out is NULL");
  CmPlan p;
  const int rc = cm_plan("nf_cluster_moments_plan", lattice, dtype, p);
  if (rc) return rc;
  out->sites_per_lane = p.ns;
  out->lanes = p.nt;
  out->quantities = p.nq;
  out->passes = p.passes;
  out->per_pass = p.per_pass;
  out->lds_bytes = int64_t(p.lds);
  return NF_OK;
}

extern "C" int nf_cluster_moments(const void *phi, const int32_t *labels, double *out, int32_t *status, int64_t *moments_out,
                                  int64_t C, const int32_t *lattice, const double *tw, int dtype, void *stream) {
  const char *what = "nf_cluster_moments";
  NF_REQUIRE(phi && labels && out && status, "%s: phi, labels, out or status is NULL", what);
  NF_REQUIRE(tw != nullptr, "%s: tw is NULL", what);
  NF_REQUIRE(C >= 1 && C <= 65535, "%s: C (%lld) must be in 1 .. 65535", what, (long long)C);
  CmPlan p;
  const int rc = cm_plan(what, lattice, dtype, p);
  if (rc) return rc;
  CmArgs A{};
  A.phi = phi; A.labels = labels; A.out = out; A.status = status; A.moments = moments_out; A.tw = tw;
  A.V = int(p.V); A.nq = p.nq; A.per_pass = p.per_pass;
  for (int mu = 0; mu < 4; ++mu) A.col[mu] = p.col[mu];
  for (int k = 0; k < kCmMaxQ; ++k) A.q[k] = p.q[k];
  A.limit = p.limit;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return dtype == NF_F32 ? cm_dispatch<float>(A, C, p, s) : cm_dispatch<double>(A, C, p, s);
}

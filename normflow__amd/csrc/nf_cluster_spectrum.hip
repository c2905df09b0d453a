// nf_cluster_spectrum.hip -- the per-cluster sums of nf_cluster_moments at every on-axis momentum k = 1 .. K_mu, behind the
// cluster-improved propagator and time-slice correlator (MI355X-side extension, no counterpart in the reference).  The rule
// is stated once in include/normflow_hip.h, "cluster spectrum", which extends "cluster-improved estimators".
// The structure is nf_cluster_moments': one workgroup per chain with nf_phi4_cluster's lane map, phi and the labels in
// registers, the checks before any indexed access, `per_pass` arrays of V int64 slots in dynamic LDS behind the reduction
// region, a lane's run of same-label sites added in a register and issued as one 64-bit integer LDS add.  Two differences:
//   - the quantities (up to 255) are too many for a table picked by selects with constant indices, so the descriptor of
//     quantity `qid` -- axis, k, component -- follows from wave-uniform integer arithmetic on qid and the per-axis prefix
//     counts of the argument struct; the axis' stride, extent and table offset are then picked by selects on the axis
//     number (0 .. 3, constant indices).  Nothing in registers is indexed dynamically: no scratch.
//   - the reduction region is 4 KiB whatever Q: a pass holds at most 16 quantities, its wave sums are added in wave order
//     at the end of the pass and its columns are written then.  A column is (sum r^2) + (sum i^2): thread j of the pass
//     owns quantity j, an R writes its column with the I that follows it in the pass, and an R that ends a pass leaves its
//     sum in the carry slot for thread 0 of the next pass.
#include "nf_internal.h"
#include "nf_cluster_spectrum_core.h"

namespace nf {
namespace {

constexpr int kCsMaxLanes = 1024;
constexpr int kCsMaxPass = 16;                      // quantities per pass
constexpr int kCsCols = kCsMaxPass + 1;             // their sums of squares, and a^4 of quantity 0 in the last
constexpr int kCsWaves = kCsMaxLanes / kWave;
constexpr size_t kCsScratch = 4096;                 // kCsWaves x kCsCols doubles of wave sums, kCsCols results, carry, flag
constexpr size_t kCsLdsBudget = 160 * 1024;
static_assert((kCsWaves * kCsCols + kCsCols + 2) * sizeof(double) <= kCsScratch, "reduction region");

struct CsPlan : CsLayout {        // K, stride, extent, off, the prefix counts, nq, ncols: nf_cluster_spectrum_core.h
  int64_t V;
  int ns, nt, per_pass, passes;
  size_t lds;
  double limit;                  // 2^min(16, 30 - ceil(log2 V))
};

int cs_plan(const char *what, const int32_t *lattice, int dtype, int kmax, CsPlan &p) {
  NF_REQUIRE(lattice != nullptr, "%s: lattice is NULL", what);
  NF_REQUIRE(dtype == NF_F32 || dtype == NF_F64, "%s: unsupported dtype %d", what, dtype);
  NF_REQUIRE(kmax >= 0, "%s: kmax (%d) must be >= 0 (0: all momenta)", what, kmax);
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
  cs_layout(lattice, kmax, p.V, p);
  size_t fit = (kCsLdsBudget - kCsScratch) / (size_t(p.V) * 8);      // >= 1: V <= 16384
  if (fit > size_t(kCsMaxPass)) fit = kCsMaxPass;
  p.per_pass = int(fit < size_t(p.nq) ? fit : size_t(p.nq));
  p.passes = (p.nq + p.per_pass - 1) / p.per_pass;
  p.lds = kCsScratch + size_t(p.per_pass) * size_t(p.V) * 8;
  int lg = 0;
  while ((int64_t(1) << lg) < p.V) ++lg;
  const int e = 30 - lg < 16 ? 30 - lg : 16;
  p.limit = e >= 0 ? double(int64_t(1) << e) : 1.0 / double(int64_t(1) << -e);
  return NF_OK;
}

struct CsArgs {
  const void *phi;
  const int32_t *labels;
  double *out;
  int32_t *status;
  const double *tw;
  int V, nq, ncols, per_pass;
  int stride[4], extent[4], off[4], qpre[4], cpre[4];
  double limit;
};

template <typename T, int NS>
__global__ __launch_bounds__(kCsMaxLanes) void cluster_spectrum_kernel(CsArgs A) {
  extern __shared__ __align__(16) unsigned char cs_lds[];
  double *red = reinterpret_cast<double *>(cs_lds);                 // [wave][kCsCols]
  double *res = red + kCsWaves * kCsCols;                           // [kCsCols]
  double *carry = res + kCsCols;                                    // sum r^2 of the R that ended the last pass
  volatile int *s_bad = reinterpret_cast<volatile int *>(carry + 1);           // the chain is refused
  unsigned long long *slots = reinterpret_cast<unsigned long long *>(cs_lds + kCsScratch);
  const int tid = threadIdx.x, NT = blockDim.x, V = A.V;
  const int lane = tid & (kWave - 1), wave = tid / kWave;
  const int64_t c = blockIdx.x;
  const T *__restrict__ gphi = static_cast<const T *>(A.phi) + c * int64_t(V);
  const int32_t *__restrict__ glab = A.labels + c * int64_t(V);
  const double *__restrict__ tw = A.tw;
  double *__restrict__ row = A.out + c * int64_t(A.ncols);

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
    for (int k = tid; k < A.ncols; k += NT) row[k] = __builtin_nan("");
    if (tid == 0) A.status[c] = 1;
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
      int stride = 1, extent = 1, two = 0, kq = 0;
      if (qid) {
        const CsQuantity d = cs_quantity(A, qid);
        stride = d.stride; extent = d.extent; two = 2 * d.off + d.comp; kq = d.k;
      }
      unsigned long long *slot = slots + size_t(j) * V;
      int run = -1;                     // the label of the lane's current run of sites, and their sum
      long long sum = 0;
#pragma unroll
      for (int k = 0; k < NS; ++k) {
        const int x = tid + k * NT;
        if (x < V) {
          double w = double(phi[k]);
          if (qid) {
            const unsigned xm = (unsigned(x) / unsigned(stride)) % unsigned(extent);
            w *= tw[two + 2 * int((unsigned(kq) * xm) % unsigned(extent))];
          }
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
        if (qid == 0) s4 = fma(a2, a2, s4);
      }
      s2 = wave_sum(s2);
      if (qid == 0) s4 = wave_sum(s4);
      if (lane == 0) {
        red[wave * kCsCols + j] = s2;
        if (qid == 0) red[wave * kCsCols + kCsMaxPass] = s4;
      }
    }
    __syncthreads();

    // ---- the waves in order, then the pass's columns
    if (tid < nqp || (tid == kCsMaxPass && q0 == 0)) {
      double r = 0;
      for (int w = 0; w < NT / kWave; ++w) r += red[w * kCsCols + tid];
      res[tid] = r;
    }
    __syncthreads();
    const double carried = *carry;                                   // read before this pass's last R overwrites it
    __syncthreads();
    if (tid < nqp) {
      const int qid = q0 + tid;
      if (qid == 0) {
        row[0] = res[0];
        row[1] = res[kCsMaxPass];
      } else {
        const CsQuantity d = cs_quantity(A, qid);
        if (d.comp == 0) {
          if (2 * d.k == d.extent) row[d.col] = res[tid];            // Nyquist: no I
          else if (tid + 1 < nqp) row[d.col] = res[tid] + res[tid + 1];
          else *carry = res[tid];
        } else if (tid == 0) {
          row[d.col] = carried + res[0];
        }
      }
    }
    // the next pass's barriers (after the zeroing, after the sums) come before res, red and carry are touched again
  }
  if (tid == 0) A.status[c] = 0;
}

template <typename T, int NS>
int cs_launch(const CsArgs &A, int64_t C, const CsPlan &p, hipStream_t s) {
  auto kern = cluster_spectrum_kernel<T, NS>;
  // per launch, as nf_cluster_moments does: the attribute belongs to the current device, and always to the budget, so that
  // no call lowers what another raised
  if (p.lds > 64 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                          int(kCsLdsBudget)) != hipSuccess) {
    (void)hipGetLastError();
    set_error("nf_cluster_spectrum: cannot raise the dynamic LDS limit to %zu B", kCsLdsBudget);
    return NF_ELAUNCH;
  }
  hipLaunchKernelGGL(kern, dim3(unsigned(C)), dim3(unsigned(p.nt)), p.lds, s, A);
  return check_launch("nf_cluster_spectrum");
}

template <typename T>
int cs_dispatch(const CsArgs &A, int64_t C, const CsPlan &p, hipStream_t s) {
  switch (p.ns) {
    case 1: return cs_launch<T, 1>(A, C, p, s);
    case 2: return cs_launch<T, 2>(A, C, p, s);
    case 4: return cs_launch<T, 4>(A, C, p, s);
    case 8: return cs_launch<T, 8>(A, C, p, s);
    case 16:
      if constexpr (sizeof(T) == 4) return cs_launch<T, 16>(A, C, p, s);     // 8-byte fields end at 8 sites per lane
  }
  set_error("nf_cluster_spectrum: no kernel for %d sites per lane", p.ns);
  return NF_EINVAL;
}

}  // namespace
}  // namespace nf

using namespace nf;

extern "C" int nf_cluster_spectrum_supported(const int32_t *lattice, int dtype, int kmax) {
  CsPlan p;
  return cs_plan("nf_cluster_spectrum_supported", lattice, dtype, kmax, p) == NF_OK ? 1 : 0;
}

extern "C" int nf_cluster_spectrum_plan(const int32_t *lattice, int dtype, int kmax, nf_spectrum_plan *out) {
  NF_REQUIRE(out != nullptr, "nf_cluster_spectrum_plan: out is NULL");
  CsPlan p;
  const int rc = cs_plan("nf_cluster_spectrum_plan", lattice, dtype, kmax, p);
  if (rc) return rc;
  out->sites_per_lane = p.ns;
  out->lanes = p.nt;
  for (int mu = 0; mu < 4; ++mu) out->kmax[mu] = p.K[mu];
  out->columns = p.ncols;
  out->quantities = p.nq;
  out->passes = p.passes;
  out->per_pass = p.per_pass;
  out->lds_bytes = int64_t(p.lds);
  return NF_OK;
}

extern "C" int nf_cluster_spectrum(const void *phi, const int32_t *labels, double *out, int32_t *status, int64_t C,
                                   const int32_t *lattice, int kmax, const double *tw, int dtype, void *stream) {
  const char *what = "nf_cluster_spectrum";
  NF_REQUIRE(phi && labels && out && status, "%s: phi, labels, out or status is NULL", what);
  NF_REQUIRE(tw != nullptr, "%s: tw is NULL", what);
  NF_REQUIRE(C >= 1 && C <= 65535, "%s: C (%lld) must be in 1 .. 65535", what, (long long)C);
  CsPlan p;
  const int rc = cs_plan(what, lattice, dtype, kmax, p);
  if (rc) return rc;
  CsArgs A{};
  A.phi = phi; A.labels = labels; A.out = out; A.status = status; A.tw = tw;
  A.V = int(p.V); A.nq = p.nq; A.ncols = p.ncols; A.per_pass = p.per_pass;
  for (int mu = 0; mu < 4; ++mu) {
    A.stride[mu] = p.stride[mu]; A.extent[mu] = p.extent[mu]; A.off[mu] = p.off[mu];
    A.qpre[mu] = p.qpre[mu]; A.cpre[mu] = p.cpre[mu];
  }
  A.limit = p.limit;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return dtype == NF_F32 ? cs_dispatch<float>(A, C, p, s) : cs_dispatch<double>(A, C, p, s);
}

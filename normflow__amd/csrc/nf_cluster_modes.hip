// nf_cluster_modes.hip -- the per-cluster sums of nf_cluster_moments at a LIST of momentum vectors n = (n_0 .. n_3), on or
// off the axes, behind the cluster-improved propagator at general momenta and the time-slice correlator at non-zero
// spatial momentum (MI355X-side extension, no counterpart in the reference).  The rule is stated once in
// include/normflow_hip.h, "cluster modes", which extends "cluster-improved estimators".
// The structure is nf_cluster_spectrum's: one workgroup per chain with nf_phi4_cluster's lane map, phi and the labels in
// registers, the checks before any indexed access, `per_pass` arrays of V int64 slots in dynamic LDS behind the 4 KiB
// reduction region, a lane's run of same-label sites added in a register and issued as one 64-bit integer LDS add, the
// wave sums added in wave order at the end of a pass, the carry slot for an R that ends a pass.  The one difference is the
// descriptor: quantity `qid` >= 1 reads row qid of the caller's device table `desc` (nf_cluster_modes_core.h) with
// wave-uniform loads -- m_0 .. m_3, the component -- and a site's phase index is (sum_mu m_mu x_mu) mod N into ONE table of
// N twiddles.  The coordinates of a lane's first site are taken once and its further sites, `lanes` apart, follow by
// mixed-radix addition of that step; nothing in registers is indexed
// dynamically: no scratch.  The table is held to cm_row_ok before a field of it is used: a table that fails refuses the
// chain, it never reaches an index.
#include "nf_internal.h"
#include "nf_cluster_modes_core.h"

namespace nf {
namespace {

constexpr int kCmMaxLanes = 1024;
constexpr int kCmMaxPass = 16;                      // quantities per pass
constexpr int kCmCols = kCmMaxPass + 1;             // their sums of squares, and a^4 of quantity 0 in the last
constexpr int kCmWaves = kCmMaxLanes / kWave;
constexpr size_t kCmScratch = 4096;                 // kCmWaves x kCmCols doubles of wave sums, kCmCols results, carry, flag
constexpr size_t kCmLdsBudget = 160 * 1024;
static_assert((kCmWaves * kCmCols + kCmCols + 2) * sizeof(double) <= kCmScratch, "reduction region");

struct CmPlan {
  int64_t V;
  int ns, nt, N, nq, per_pass, passes;
  int stride[4], extent[4], step[4];
  size_t lds;
  double limit;                  // 2^min(16, 30 - ceil(log2 V))
};

const char *cm_reason(int e) {
  switch (e) {
    case kCmNoAxis: return "every extent is 1 (N = 1): there is no momentum";
    case kCmLargeN: return "N, the lcm of the extents, must be the lattice's and at most 65536";
    case kCmCount: return "P must be in 1 .. 512";
    case kCmUnitAxis: return "a non-zero component on an axis of extent 1";
    case kCmQuantities: return "Q must be in 2 .. 1025 and the table's";
    case kCmRowZero: return "row 0 of desc is not (0, 0, 0, 0, 0, 0, 0, 2 + P) of its P momenta";
    case kCmM_: return "an m outside 0 .. N - 1 or no multiple of N / L";
    case kCmComponent: return "a component outside {0, 1}, or an I that does not follow its R";
    case kCmColumn: return "a column outside 2 .. 1 + P or out of order";
    case kCmConjugate: return "the R-without-I flag is not the momentum's";
  }
  return "";
}

// the lattice's part of the plan: the class of nf_phi4_cluster, N, the lane map, the range; Q comes from the caller
int cm_plan(const char *what, const int32_t *lattice, int dtype, int Q, CmPlan &p) {
  NF_REQUIRE(lattice != nullptr, "%s: lattice is NULL", what);
  NF_REQUIRE(dtype == NF_F32 || dtype == NF_F64, "%s: unsupported dtype %d", what, dtype);
  for (int mu = 0; mu < 4; ++mu) NF_REQUIRE(lattice[mu] >= 1, "%s: lattice extents must be >= 1", what);
  nf_cluster_plan cp;
  if (nf_phi4_cluster_plan(lattice, dtype, &cp) != NF_OK) {
    set_error("%s: a chain of the lattice (%d, %d, %d, %d) is outside the class of nf_phi4_cluster (V sizeof <= 64 KiB)", what,
              lattice[0], lattice[1], lattice[2], lattice[3]);
    return NF_EINVAL;
  }
  const long long lcm = cm_lcm(lattice);
  NF_REQUIRE(lcm > 1, "%s: %s", what, cm_reason(kCmNoAxis));
  NF_REQUIRE(lcm <= kCmMaxN, "%s: %s (lattice (%d, %d, %d, %d))", what, cm_reason(kCmLargeN), lattice[0], lattice[1], lattice[2],
             lattice[3]);
  NF_REQUIRE(Q >= 2 && Q <= 1 + 2 * kCmMaxModes, "%s: Q (%d): %s", what, Q, cm_reason(kCmQuantities));
  p.V = int64_t(lattice[0]) * lattice[1] * lattice[2] * lattice[3];
  p.ns = cp.sites_per_lane;
  p.nt = cp.lanes;
  p.N = int(lcm);
  p.nq = Q;
  int stride = int(p.V);
  for (int mu = 0; mu < 4; ++mu) {
    stride /= lattice[mu];
    p.stride[mu] = stride;
    p.extent[mu] = lattice[mu];
  }
  // a lane's sites are `lanes` apart: the coordinates of that step (0 where the lanes hold the chain: one site per lane)
  for (int mu = 0; mu < 4; ++mu) p.step[mu] = int((int64_t(p.nt) % p.V) / p.stride[mu] % lattice[mu]);
  size_t fit = (kCmLdsBudget - kCmScratch) / (size_t(p.V) * 8);      // >= 1: V <= 16384
  if (fit > size_t(kCmMaxPass)) fit = kCmMaxPass;
  p.per_pass = int(fit < size_t(p.nq) ? fit : size_t(p.nq));
  p.passes = (p.nq + p.per_pass - 1) / p.per_pass;
  p.lds = kCmScratch + size_t(p.per_pass) * size_t(p.V) * 8;
  int lg = 0;
  while ((int64_t(1) << lg) < p.V) ++lg;
  const int e = 30 - lg < 16 ? 30 - lg : 16;
  p.limit = e >= 0 ? double(int64_t(1) << e) : 1.0 / double(int64_t(1) << -e);
  return NF_OK;
}

// the momenta's part: Q of the list (and the table where desc is not NULL)
int cm_list(const char *what, const int32_t *lattice, const int32_t *modes, int P, int32_t *desc, int *Q, int *N) {
  NF_REQUIRE(lattice != nullptr, "%s: lattice is NULL", what);
  NF_REQUIRE(modes != nullptr, "%s: modes is NULL", what);
  for (int mu = 0; mu < 4; ++mu) NF_REQUIRE(lattice[mu] >= 1, "%s: lattice extents must be >= 1", what);
  int bad = 0;
  const int e = cm_describe(lattice, modes, P, desc, Q, N, &bad);
  if (e == kCmCount) {
    set_error("%s: P (%d) must be in 1 .. %d", what, P, kCmMaxModes);
    return NF_EINVAL;
  }
  if (e == kCmUnitAxis) {
    set_error("%s: momentum %d (%d, %d, %d, %d): %s of the lattice (%d, %d, %d, %d)", what, bad, modes[4 * bad],
              modes[4 * bad + 1], modes[4 * bad + 2], modes[4 * bad + 3], cm_reason(e), lattice[0], lattice[1], lattice[2],
              lattice[3]);
    return NF_EINVAL;
  }
  NF_REQUIRE(e == kCmOk, "%s: %s (lattice (%d, %d, %d, %d))", what, cm_reason(e), lattice[0], lattice[1], lattice[2], lattice[3]);
  return NF_OK;
}

struct CmArgs {
  const void *phi;
  const int32_t *labels;
  double *out;
  int32_t *status;
  const double *tw;
  const int32_t *desc;
  int V, nq, per_pass, N;
  int stride[4], extent[4], step[4];
  double limit;
};

template <typename T, int NS>
__global__ __launch_bounds__(kCmMaxLanes) void cluster_modes_kernel(CmArgs A) {
  extern __shared__ __align__(16) unsigned char cm_lds[];
  double *red = reinterpret_cast<double *>(cm_lds);                 // [wave][kCmCols]
  double *res = red + kCmWaves * kCmCols;                           // [kCmCols]
  double *carry = res + kCmCols;                                    // sum r^2 of the R that ended the last pass
  volatile int *s_bad = reinterpret_cast<volatile int *>(carry + 1);           // 1: the chain is refused, 2: the table
  unsigned long long *slots = reinterpret_cast<unsigned long long *>(cm_lds + kCmScratch);
  const int tid = threadIdx.x, NT = blockDim.x, V = A.V;
  const int lane = tid & (kWave - 1), wave = tid / kWave;
  const int64_t c = blockIdx.x;
  const T *__restrict__ gphi = static_cast<const T *>(A.phi) + c * int64_t(V);
  const int32_t *__restrict__ glab = A.labels + c * int64_t(V);
  const double *__restrict__ tw = A.tw;
  const int32_t *__restrict__ desc = A.desc;
  const unsigned N = unsigned(A.N);

  // ---- the chain into registers with its coordinates, and the checks: before any indexed access
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
  // the coordinates of the lane's first site; its further sites are NT apart and follow by mixed-radix addition
  const unsigned ut = unsigned(tid) % unsigned(V);
  const unsigned b0 = (ut / unsigned(A.stride[0])) % unsigned(A.extent[0]), b1 = (ut / unsigned(A.stride[1])) % unsigned(A.extent[1]);
  const unsigned b2 = (ut / unsigned(A.stride[2])) % unsigned(A.extent[2]), b3 = (ut / unsigned(A.stride[3])) % unsigned(A.extent[3]);
  const unsigned L0 = unsigned(A.extent[0]), L1 = unsigned(A.extent[1]), L2 = unsigned(A.extent[2]), L3 = unsigned(A.extent[3]);
  const unsigned d0 = unsigned(A.step[0]), d1 = unsigned(A.step[1]), d2 = unsigned(A.step[2]), d3 = unsigned(A.step[3]);
  const int ncols = desc[kCmMode];                                   // row 0: 2 + P
  int bad_row = 0;
  if (!cm_row_ok(desc, 0, A.nq, A.N, ncols)) bad_row = 1;
  for (int q = 1 + tid; q < A.nq; q += NT)
    if (!cm_row_ok(desc, q, A.nq, A.N, ncols)) bad_row = 1;
  if (tid == 0) *s_bad = 0;
  __syncthreads();
  if (bad_row) *s_bad = 2;
  __syncthreads();
  if (bad && *s_bad == 0) *s_bad = 1;
  __syncthreads();
  const int refused = *s_bad;                                        // the same in every lane
  if (refused == 2) {                  // the row's length is the table's own word: out is left alone
    if (tid == 0) A.status[c] = 1;
    return;
  }
  double *__restrict__ row = A.out + c * int64_t(ncols);
  if (refused) {
    for (int k = tid; k < ncols; k += NT) row[k] = __builtin_nan("");
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
      const int32_t *d = desc + size_t(qid) * kCmRow;                // wave-uniform loads
      const unsigned m0 = unsigned(d[kCmM]), m1 = unsigned(d[kCmM + 1]), m2 = unsigned(d[kCmM + 2]), m3 = unsigned(d[kCmM + 3]);
      const int comp = d[kCmComp];
      unsigned long long *slot = slots + size_t(j) * V;
      int run = -1;                     // the label of the lane's current run of sites, and their sum
      long long sum = 0;
      unsigned x0 = b0, x1 = b1, x2 = b2, x3 = b3;                   // the coordinates of the lane's site k
#pragma unroll
      for (int k = 0; k < NS; ++k) {
        const int x = tid + k * NT;
        if (x < V) {
          // 16 sites per lane: an empty statement the compiler cannot see through, so that the sixteen conversions to
          // double are made here, one at a time, and not once in front of the loop over the quantities, where they
          // cost 32 registers more than a workgroup of 1024 lanes has
          if constexpr (NS == 16) asm volatile("" : "+v"(phi[k]));
          double w = double(phi[k]);
          if (qid) {
            const unsigned t = m0 * x0 + m1 * x1 + m2 * x2 + m3 * x3;                  // < 2^32: m < 2^16, x < 2^14
            w *= tw[2 * (t % N) + unsigned(comp)];
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
        if (k + 1 < NS) {               // site k + 1 = site k + NT: add the step's coordinates, the carries upwards
          unsigned cy;
          x3 += d3; cy = x3 >= L3 ? 1u : 0u; x3 -= cy ? L3 : 0u;
          x2 += d2 + cy; cy = x2 >= L2 ? 1u : 0u; x2 -= cy ? L2 : 0u;
          x1 += d1 + cy; cy = x1 >= L1 ? 1u : 0u; x1 -= cy ? L1 : 0u;
          x0 += d0 + cy; x0 -= x0 >= L0 ? L0 : 0u;
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
        red[wave * kCmCols + j] = s2;
        if (qid == 0) red[wave * kCmCols + kCmMaxPass] = s4;
      }
    }
    __syncthreads();

    // ---- the waves in order, then the pass's columns
    if (tid < nqp || (tid == kCmMaxPass && q0 == 0)) {
      double r = 0;
      for (int w = 0; w < NT / kWave; ++w) r += red[w * kCmCols + tid];
      res[tid] = r;
    }
    __syncthreads();
    const double carried = *carry;                                   // read before this pass's last R overwrites it
    __syncthreads();
    if (tid < nqp) {
      const int qid = q0 + tid;
      if (qid == 0) {
        row[0] = res[0];
        row[1] = res[kCmMaxPass];
      } else {
        const int32_t *d = desc + size_t(qid) * kCmRow;
        const int col = d[kCmCol];
        if (d[kCmComp] == 0) {
          if (d[kCmROnly]) row[col] = res[tid];                      // self-conjugate: no I
          else if (tid + 1 < nqp) row[col] = res[tid] + res[tid + 1];
          else *carry = res[tid];
        } else if (tid == 0) {
          row[col] = carried + res[0];
        }
      }
    }
    // the next pass's barriers (after the zeroing, after the sums) come before res, red and carry are touched again
  }
  if (tid == 0) A.status[c] = 0;
}

template <typename T, int NS>
int cm_launch(const CmArgs &A, int64_t C, const CmPlan &p, hipStream_t s) {
  auto kern = cluster_modes_kernel<T, NS>;
  // per launch, as nf_cluster_moments does: the attribute belongs to the current device, and always to the budget, so that
  // no call lowers what another raised
  if (p.lds > 64 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                          int(kCmLdsBudget)) != hipSuccess) {
    (void)hipGetLastError();
    set_error("nf_cluster_modes: cannot raise the dynamic LDS limit to %zu B", kCmLdsBudget);
    return NF_ELAUNCH;
  }
  hipLaunchKernelGGL(kern, dim3(unsigned(C)), dim3(unsigned(p.nt)), p.lds, s, A);
  return check_launch("nf_cluster_modes");
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
  set_error("nf_cluster_modes: no kernel for %d sites per lane", p.ns);
  return NF_EINVAL;
}

}  // namespace
}  // namespace nf

using namespace nf;

extern "C" int nf_cluster_modes_describe(const int32_t *lattice, const int32_t *modes, int P, int32_t *desc, int32_t *Q,
                                         int32_t *N) {
  const char *what = "nf_cluster_modes_describe";
  NF_REQUIRE(Q != nullptr && N != nullptr, "%s: Q or N is NULL", what);
  int q = 0, n = 0;
  const int rc = cm_list(what, lattice, modes, P, desc, &q, &n);
  *Q = q;
  *N = n;
  return rc;
}

extern "C" int nf_cluster_modes_check(const int32_t *lattice, const int32_t *desc, int Q, int N) {
  const char *what = "nf_cluster_modes_check";
  NF_REQUIRE(lattice != nullptr, "%s: lattice is NULL", what);
  NF_REQUIRE(desc != nullptr, "%s: desc is NULL", what);
  for (int mu = 0; mu < 4; ++mu) NF_REQUIRE(lattice[mu] >= 1, "%s: lattice extents must be >= 1", what);
  int bad = 0;
  const int e = cm_check(lattice, desc, Q, N, &bad);
  NF_REQUIRE(e == kCmOk, "%s: desc row %d (Q = %d, N = %d): %s", what, bad, Q, N, cm_reason(e));
  return NF_OK;
}

extern "C" int nf_cluster_modes_plan(const int32_t *lattice, int dtype, const int32_t *modes, int P, nf_modes_plan *out) {
  const char *what = "nf_cluster_modes_plan";
  NF_REQUIRE(out != nullptr, "%s: out is NULL", what);
  int Q = 0, N = 0;
  int rc = cm_list(what, lattice, modes, P, nullptr, &Q, &N);
  if (rc) return rc;
  CmPlan p;
  rc = cm_plan(what, lattice, dtype, Q, p);
  if (rc) return rc;
  out->sites_per_lane = p.ns;
  out->lanes = p.nt;
  out->N = p.N;
  out->columns = 2 + P;
  out->quantities = p.nq;
  out->per_pass = p.per_pass;
  out->passes = p.passes;
  out->lds_bytes = int64_t(p.lds);
  return NF_OK;
}

extern "C" int nf_cluster_modes_supported(const int32_t *lattice, int dtype, const int32_t *modes, int P) {
  nf_modes_plan out;
  return nf_cluster_modes_plan(lattice, dtype, modes, P, &out) == NF_OK ? 1 : 0;
}

extern "C" int nf_cluster_modes(const void *phi, const int32_t *labels, double *out, int32_t *status, int64_t C,
                                const int32_t *lattice, const int32_t *desc, int Q, const double *twN, int N, int dtype,
                                void *stream) {
  const char *what = "nf_cluster_modes";
  NF_REQUIRE(phi && labels && out && status, "%s: phi, labels, out or status is NULL", what);
  NF_REQUIRE(desc != nullptr, "%s: desc is NULL", what);
  NF_REQUIRE(twN != nullptr, "%s: twN is NULL", what);
  NF_REQUIRE(C >= 1 && C <= 65535, "%s: C (%lld) must be in 1 .. 65535", what, (long long)C);
  CmPlan p;
  const int rc = cm_plan(what, lattice, dtype, Q, p);
  if (rc) return rc;
  NF_REQUIRE(N == p.N, "%s: N (%d) is not the lcm of the lattice's extents (%d)", what, N, p.N);
  CmArgs A{};
  A.phi = phi; A.labels = labels; A.out = out; A.status = status; A.tw = twN; A.desc = desc;
  A.V = int(p.V); A.nq = p.nq; A.per_pass = p.per_pass; A.N = p.N;
  for (int mu = 0; mu < 4; ++mu) {
    A.stride[mu] = p.stride[mu]; A.extent[mu] = p.extent[mu]; A.step[mu] = p.step[mu];
  }
  A.limit = p.limit;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return dtype == NF_F32 ? cm_dispatch<float>(A, C, p, s) : cm_dispatch<double>(A, C, p, s);
}

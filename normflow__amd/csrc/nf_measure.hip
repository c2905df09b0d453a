// nf_measure.hip -- the sufficient statistics of lattice configurations in one pass (MI355X-side extension, no
// counterpart in the reference): per row of (N, V) the power sums, the d nearest-neighbour link sums and the slice sums of
// every axis, all in double (include/normflow_hip.h, nf_lattice_measure).
//
// A team of lanes stages an IMAGE of the row -- the whole row, or a segment of planes of the slowest axis of extent > 1,
// the marched axis -- in LDS once (16-byte loads where the plan and the pointer allow) and every sum is read from that
// image by measure_image (nf_measure_core.h, shared with nf_measure_tiled.hip), a device routine that knows nothing of
// where the image came from (an LDS image of the HMC kernels would do):
//   power sums, links   lane l of the team takes the sites l, l + lanes, ... in index order, its coordinates carried
//                       along in mixed radix (no division per site); lane partials -> wave shuffle tree -> waves in order
//   slice sums          per axis, fixed (slice t, stripe j) pairs on fixed lanes: stripe j adds the sites j, j + J, ... of
//                       its slice in index order, then the J stripes of a slice are added in stripe order
// All in double with explicit fma, no atomics: the bits of a row depend on the row's values and on the plan (lattice and
// dtype) alone -- not on N, the row's position, its neighbours in the batch, or the pointer's alignment (the wide and the
// narrow staging fill the same image).
// Regimes (nf_lattice_measure_plan):
//   packed      V <= 256 sites: four rows per workgroup, one wave each
//   resident    V sizeof <= 64 KiB: one workgroup per row
//   segmented   beyond: the marched axis is cut into `segments` runs of seg_len planes, one workgroup each, which reads
//               the one plane before its run from HBM for the backward link; the (7 + sum of image extents) partials of
//               a segment go to the workspace and measure_finish adds them in segment order.  A plane must fit the LDS.
#include "nf_measure_core.h"

namespace nf {
namespace {

constexpr int kMsPackedRows = kBlock / kWave;
constexpr size_t kMsResident = 64 * 1024;         // a row up to this size is one image
constexpr size_t kMsSegmentImage = 32 * 1024;     // a segment's image: four workgroups per CU

struct MsPlan {
  int64_t V, plane;    // sites of a row, of a plane of the marched axis
  int L[4];
  int a0;              // the marched axis: the slowest of extent > 1 (3 when V = 1)
  int regime, rpg, segments, seg_len, lanes, team, vec, n_out, n_part;
  int goff[4], poff[4];   // the slice sums' offsets behind the 7 scalars: in a row of out, in a segment's partials
  size_t img_bytes, lds;
};

// The one planner: nf_lattice_measure_supported, _plan and _workspace answer from it and nf_lattice_measure launches by it.
int ms_plan(const char *what, const int32_t *lattice, int dtype, MsPlan &p) {
  NF_REQUIRE(lattice != nullptr, "%s: lattice is NULL", what);
  NF_REQUIRE(dtype == NF_F32 || dtype == NF_F64, "%s: unsupported dtype %d", what, dtype);
  const size_t elem = dtype == NF_F32 ? 4 : 8;
  p.V = 1;
  p.a0 = -1;
  int64_t n_out = 7;
  for (int mu = 0; mu < 4; ++mu) {
    NF_REQUIRE(lattice[mu] >= 1, "%s: lattice extents must be >= 1", what);
    p.V *= lattice[mu];
    NF_REQUIRE(p.V < (int64_t(1) << 31), "%s: a row of the lattice (%d, %d, %d, %d) has 2^31 sites or more", what,
               lattice[0], lattice[1], lattice[2], lattice[3]);
    p.L[mu] = lattice[mu];
    if (p.a0 < 0 && lattice[mu] > 1) p.a0 = mu;
    p.goff[mu] = int(n_out - 7);
    n_out += lattice[mu];
  }
  if (p.a0 < 0) p.a0 = 3;
  NF_REQUIRE(n_out < (int64_t(1) << 31), "%s: a row of out has n_out = %lld entries, 2^31 or more", what, (long long)n_out);
  p.n_out = int(n_out);
  p.plane = p.V / p.L[p.a0];
  const int per = int(16 / elem);
  p.vec = p.L[3] % per == 0 ? per : 1;
  p.rpg = 1;
  p.segments = 1;
  p.seg_len = p.L[p.a0];
  if (p.V <= kMsPackedSites) {
    p.regime = NF_MEASURE_PACKED;
    p.rpg = kMsPackedRows;
    p.lanes = kBlock;
    p.team = ms_row_team(p.V);
  } else if (size_t(p.V) * elem <= kMsResident) {
    p.regime = NF_MEASURE_RESIDENT;
    p.lanes = p.team = ms_row_team(p.V);
  } else {
    p.regime = NF_MEASURE_SEGMENTED;
    const size_t plane_bytes = size_t(p.plane) * elem;
    NF_REQUIRE(plane_bytes <= kMsLdsBudget - kMsScratch,
               "%s: a plane of the lattice (%d, %d, %d, %d) (%zu B) does not fit the LDS (%zu B)", what, lattice[0],
               lattice[1], lattice[2], lattice[3], plane_bytes, kMsLdsBudget - kMsScratch);
    int len = int(kMsSegmentImage / plane_bytes);
    len = len < 1 ? 1 : len > p.L[p.a0] ? p.L[p.a0] : len;
    p.segments = (p.L[p.a0] - 1) / len + 1;
    p.seg_len = (p.L[p.a0] - 1) / p.segments + 1;       // the segments as even as they get
    // every image is whole 16-byte units and starts on one: a plane is (it holds whole rows of the fastest axis) unless
    // the marched axis IS the fastest one; then the segments are cut at multiples of vec (L[3] is one, so the last fits)
    if (p.plane % p.vec) p.seg_len = (p.seg_len + p.vec - 1) / p.vec * p.vec;
    p.segments = (p.L[p.a0] - 1) / p.seg_len + 1;
    p.lanes = p.team = ms_image_team(int64_t(p.seg_len) * p.plane);
  }
  const size_t img = size_t(p.seg_len) * size_t(p.plane) * elem;
  p.img_bytes = (img + 15) & ~size_t(15);
  p.lds = kMsScratch + size_t(p.rpg) * p.img_bytes;
  int np = 7;
  for (int mu = 0; mu < 4; ++mu) {
    p.poff[mu] = np - 7;
    np += mu == p.a0 ? p.seg_len : p.L[mu];
  }
  p.n_part = np;
  return NF_OK;
}

size_t ms_workspace(int64_t N, const MsPlan &p) {
  if (p.segments == 1 || N < 1) return 0;
  return (size_t(N) * size_t(p.segments) * size_t(p.n_part) * sizeof(double) + 255) & ~size_t(255);
}

struct MsArgs {
  const void *cfgs;
  double *dst;          // (N, n_out), or the partials (N, segments, n_part)
  int64_t N, V, plane;
  int L[4], off[4];     // off: the slice sums' offsets in a row of dst
  int a0, La0, rpg, segments, seg_len, team, n_dst;
  unsigned img_bytes;
};

template <typename T, int VEC>
__global__ __launch_bounds__(kMsMaxLanes) void measure_rows(MsArgs A) {
  extern __shared__ __align__(16) unsigned char ms_lds[];
  double *red = reinterpret_cast<double *>(ms_lds), *sp = red + kMsRed;
  const int team = threadIdx.x / A.team, tl = threadIdx.x % A.team;
  T *img = reinterpret_cast<T *>(ms_lds + kMsScratch + size_t(team) * A.img_bytes);
  const int seg = int(blockIdx.x % unsigned(A.segments));
  int64_t row = int64_t(blockIdx.x / unsigned(A.segments)) * A.rpg + team;
  const bool live = row < A.N;
  if (!live) row = A.N - 1;                              // a team past the batch measures the last row and writes nothing
  const int p0 = seg * A.seg_len;
  int E[4], Lext[4], off[4];
#pragma unroll
  for (int mu = 0; mu < 4; ++mu) {
    Lext[mu] = A.L[mu];
    off[mu] = A.off[mu];
    E[mu] = A.L[mu];
    if (A.segments > 1 && mu == A.a0) E[mu] = A.seg_len < A.La0 - p0 ? A.seg_len : A.La0 - p0;
  }
  const T *rowp = static_cast<const T *>(A.cfgs) + row * A.V;
  const T *src = rowp + int64_t(p0) * A.plane;
  const T *halo = A.segments > 1 ? rowp + int64_t(p0 > 0 ? p0 - 1 : A.La0 - 1) * A.plane : nullptr;
  const int n = E[0] * E[1] * E[2] * E[3];
  for (int u = tl; u < n / VEC; u += A.team) stage_w<T, VEC>(src + u * VEC, img + u * VEC);
  __syncthreads();
  double *dst = A.dst + (row * A.segments + seg) * A.n_dst;
  measure_image<T, false>(img, halo, nullptr, E, Lext, off, A.a0, -1, tl, A.team, team * (A.team / kWave), team * A.team,
                          red, sp, dst, live);
}

struct MsFinish {
  const double *part;
  double *out;
  int64_t N;
  int L[4], goff[4], poff[4];
  int a0, segments, seg_len, n_out, n_part;
};

// out[row, q] = the partials of q over the segments, in segment order; a slice of the marched axis has one segment
__global__ __launch_bounds__(kBlock) void measure_finish(MsFinish F) {
  const int64_t idx = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (idx >= F.N * F.n_out) return;
  const int64_t row = idx / F.n_out;
  const int q = int(idx % F.n_out);
  int pq = q, one = -1;
  if (q >= 7) {
#pragma unroll
    for (int mu = 0; mu < 4; ++mu) {
      const int t = q - 7 - F.goff[mu];
      if (t >= 0 && t < F.L[mu]) {
        if (mu == F.a0) { one = t / F.seg_len; pq = 7 + F.poff[mu] + t % F.seg_len; }
        else pq = 7 + F.poff[mu] + t;
      }
    }
  }
  const double *p = F.part + row * F.segments * F.n_part + pq;
  double r = 0;
  if (one >= 0) r = p[int64_t(one) * F.n_part];
  else
    for (int s = 0; s < F.segments; ++s) r += p[int64_t(s) * F.n_part];
  F.out[idx] = r;
}

template <typename T, int VEC>
int ms_run(const MsArgs &A, const MsPlan &p, int64_t groups, hipStream_t s) {
  auto kern = measure_rows<T, VEC>;
  if (p.lds > 64 * 1024) {
    // once per instantiation, to the budget: no later call lowers it again
    static const hipError_t raised = hipFuncSetAttribute(
        reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, int(kMsLdsBudget));
    if (raised != hipSuccess) {
      (void)hipGetLastError();
      set_error("nf_lattice_measure: cannot raise the dynamic LDS limit to %zu B", kMsLdsBudget);
      return NF_ELAUNCH;
    }
  }
  hipLaunchKernelGGL(kern, dim3(unsigned(groups)), dim3(unsigned(p.lanes)), p.lds, s, A);
  return check_launch("nf_lattice_measure");
}

}  // namespace
}  // namespace nf

using namespace nf;

extern "C" int nf_lattice_measure_supported(const int32_t *lattice, int dtype) {
  MsPlan p;
  return ms_plan("nf_lattice_measure_supported", lattice, dtype, p) == NF_OK ? 1 : 0;
}

extern "C" int nf_lattice_measure_plan(const int32_t *lattice, int dtype, nf_measure_plan *out) {
  NF_REQUIRE(out != nullptr, "nf_lattice_measure_plan: out is NULL");
  MsPlan p;
  const int rc = ms_plan("nf_lattice_measure_plan", lattice, dtype, p);
  if (rc) return rc;
  out->regime = p.regime;
  out->rows_per_group = p.rpg;
  out->segments = p.segments;
  out->seg_len = p.seg_len;
  out->stage_planes = p.seg_len;
  out->lanes = p.team;
  out->vec = p.vec;
  out->n_out = p.n_out;
  out->lds_bytes = int64_t(p.lds);
  out->lds_budget = int64_t(kMsLdsBudget);
  return NF_OK;
}

extern "C" size_t nf_lattice_measure_workspace(int64_t N, const int32_t *lattice, int dtype) {
  MsPlan p;
  if (ms_plan("nf_lattice_measure_workspace", lattice, dtype, p) != NF_OK) return 0;
  return ms_workspace(N, p);
}

extern "C" int nf_lattice_measure(const void *cfgs, double *out, int64_t N, const int32_t *lattice, void *workspace,
                                  size_t workspace_bytes, int dtype, void *stream) {
  NF_REQUIRE(cfgs && out, "nf_lattice_measure: NULL pointer argument");
  NF_REQUIRE(N >= 0, "nf_lattice_measure: N (%lld) is negative", (long long)N);
  MsPlan p;
  const int rc = ms_plan("nf_lattice_measure", lattice, dtype, p);
  if (rc) return rc;
  if (N == 0) return NF_OK;
  const int64_t groups = (N + p.rpg - 1) / p.rpg * p.segments;
  NF_REQUIRE(groups <= kMsMaxGroups && (N * p.n_out + kBlock - 1) / kBlock <= kMsMaxGroups,
             "nf_lattice_measure: %lld rows need more than the %lld workgroups of one launch: measure them in several calls",
             (long long)N, (long long)kMsMaxGroups);
  const size_t need = ms_workspace(N, p);
  NF_REQUIRE(need == 0 || (workspace != nullptr && workspace_bytes >= need),
             "nf_lattice_measure: workspace %zu B < %zu B needed", workspace ? workspace_bytes : size_t(0), need);
  NF_REQUIRE(need == 0 || (reinterpret_cast<uintptr_t>(workspace) & 7) == 0,
             "nf_lattice_measure: the workspace must be 8-byte aligned");
  MsArgs A{};
  A.cfgs = cfgs;
  A.dst = need ? static_cast<double *>(workspace) : out;
  A.N = N; A.V = p.V; A.plane = p.plane;
  for (int mu = 0; mu < 4; ++mu) {
    A.L[mu] = p.L[mu];
    A.off[mu] = need ? p.poff[mu] : p.goff[mu];
  }
  A.a0 = p.a0; A.La0 = p.L[p.a0]; A.rpg = p.rpg; A.segments = p.segments; A.seg_len = p.seg_len; A.team = p.team;
  A.n_dst = need ? p.n_part : p.n_out;
  A.img_bytes = unsigned(p.img_bytes);
  hipStream_t s = static_cast<hipStream_t>(stream);
  // 16-byte loads need every image to start on 16 bytes: the fastest extent a multiple of 16 / sizeof (the plan's vec) and
  // the caller's pointer aligned; either way the image, and with it every sum, is the same
  const bool wide = p.vec > 1 && (reinterpret_cast<uintptr_t>(cfgs) & 15) == 0;
  int rc2;
  if (dtype == NF_F32) rc2 = wide ? ms_run<float, 4>(A, p, groups, s) : ms_run<float, 1>(A, p, groups, s);
  else rc2 = wide ? ms_run<double, 2>(A, p, groups, s) : ms_run<double, 1>(A, p, groups, s);
  if (rc2 || !need) return rc2;
  MsFinish F{};
  F.part = static_cast<const double *>(workspace);
  F.out = out;
  F.N = N;
  for (int mu = 0; mu < 4; ++mu) {
    F.L[mu] = p.L[mu];
    F.goff[mu] = p.goff[mu];
    F.poff[mu] = p.poff[mu];
  }
  F.a0 = p.a0; F.segments = p.segments; F.seg_len = p.seg_len; F.n_out = p.n_out; F.n_part = p.n_part;
  hipLaunchKernelGGL(measure_finish, dim3(unsigned((N * p.n_out + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, F);
  return check_launch("nf_lattice_measure (finish)");
}

// nf_measure_tiled.hip -- nf_lattice_measure's statistics for rows of which not even a plane of the slowest axis fits the
// LDS (include/normflow_hip.h, nf_lattice_measure_tiled): the row is cut into BRICKS along its first two axes of extent
// > 1, a0 and a1, one workgroup per brick.  The measure pass reads every site once and needs the backward neighbour alone,
// so there is nothing a ring of planes could reuse.
//   brick     e0 planes of a0 x e1 sub-planes of a1 x all of the axes behind (a sub-plane is `sub` sites).  The planner
//             fills a1 first and takes more than one plane only with whole planes, so a brick is ONE run of consecutive
//             sites of the row: it is staged into LDS once, 16 bytes at a time where the plan's vec and the pointer allow
//   sums      measure_image (nf_measure_core.h) reads every sum from the image; the plane before the brick (over the same
//             sub-planes) and the sub-plane before it (a brick cut along a1 is part of one plane) are read from HBM for
//             the backward links
//   partials  a brick writes its 7 + (e0 + e1 + the uncut extents) sums to the workspace (row, brick, n_part), bricks in
//             the order b0 n1 + b1; measure_tiled_finish adds them, one wave per (row, output): lane l adds the bricks l,
//             l + 64, ... of the output's list in order, then the shuffle tree.  A slice of a0 (a1) lists the n1 (n0)
//             bricks that hold it in b1 (b0) order, everything else all bricks.
// All in double with explicit fma, no atomics: a row's bits depend on the row, the lattice, the dtype and the cap alone.
#include "nf_measure_core.h"

namespace nf {
namespace {

// the default cap of a brick.  Measured on 48^4 fp64 x 4 rows (tools/measure_bench.py): 15.7 k rows/s with 32 KiB (bricks of
// one 18 KiB sub-plane), 10.4 k rows/s with 64 KiB (54 KiB bricks)
constexpr size_t kMtBrick = 32 * 1024;
constexpr int kMtFinishTeams = kBlock / kWave;    // (row, output) pairs per workgroup of the finish

struct MtPlan {
  int64_t V, plane;    // sites of a row, of a plane of a0
  int L[4];
  int a0, a1;          // the cut axes: the first two of extent > 1 (a0 = 3 when V = 1; a1 = -1 when there is no second)
  int sub;             // sites of one (x_a0, x_a1) sub-plane
  int e0, e1, n0, n1, bricks, lanes, vec, n_out, n_part;
  int goff[4], poff[4];   // the slice sums' offsets behind the 7 scalars: in a row of out, in a brick's partials
  size_t img_bytes, lds;
};

// ceil(L / e) pieces of an axis of L sites (units of `unit` sites: L is a multiple), at most `cap` sites each and as even
// as they get; a cap below one unit gives pieces of one unit
int even_cut(int L, int64_t cap, int unit) {
  const int Lu = L / unit;
  int64_t eu = cap / unit;
  eu = eu < 1 ? 1 : eu > Lu ? Lu : eu;
  const int n = (Lu - 1) / int(eu) + 1;
  return ((Lu - 1) / n + 1) * unit;
}

// The one planner: nf_lattice_measure_tiled_supported, _plan and _workspace answer from it and nf_lattice_measure_tiled
// launches by it.
int mt_plan(const char *what, const int32_t *lattice, size_t brick_bytes, int dtype, MtPlan &p) {
  NF_REQUIRE(lattice != nullptr, "%s: lattice is NULL", what);
  NF_REQUIRE(dtype == NF_F32 || dtype == NF_F64, "%s: unsupported dtype %d", what, dtype);
  const size_t elem = dtype == NF_F32 ? 4 : 8;
  p.V = 1;
  p.a0 = p.a1 = -1;
  int64_t n_out = 7;
  for (int mu = 0; mu < 4; ++mu) {
    NF_REQUIRE(lattice[mu] >= 1, "%s: lattice extents must be >= 1", what);
    p.V *= lattice[mu];
    NF_REQUIRE(p.V < (int64_t(1) << 31), "%s: a row of the lattice (%d, %d, %d, %d) has 2^31 sites or more", what,
               lattice[0], lattice[1], lattice[2], lattice[3]);
    p.L[mu] = lattice[mu];
    if (lattice[mu] > 1) {
      if (p.a0 < 0) p.a0 = mu;
      else if (p.a1 < 0) p.a1 = mu;
    }
    p.goff[mu] = int(n_out - 7);
    n_out += lattice[mu];
  }
  if (p.a0 < 0) p.a0 = 3;
  NF_REQUIRE(n_out < (int64_t(1) << 31), "%s: a row of out has n_out = %lld entries, 2^31 or more", what, (long long)n_out);
  p.n_out = int(n_out);
  const size_t avail = kMsLdsBudget - kMsScratch;
  if (brick_bytes == 0) brick_bytes = kMtBrick;
  NF_REQUIRE(brick_bytes >= elem && brick_bytes <= kMsLdsBudget,
             "%s: brick_bytes = %zu is below one element (%zu B) or above the LDS budget (%zu B)", what, brick_bytes, elem,
             kMsLdsBudget);
  const int64_t cap = int64_t((brick_bytes < avail ? brick_bytes : avail) / elem);      // sites
  p.plane = p.V / p.L[p.a0];
  const int per = int(16 / elem);
  p.vec = p.L[3] % per == 0 ? per : 1;
  p.e1 = p.n1 = 1;
  if (p.a1 >= 0) {
    p.sub = int(p.plane / p.L[p.a1]);
    // a piece of the fastest axis is whole 16-byte units; behind any other axis lie whole rows of the fastest one
    p.e1 = even_cut(p.L[p.a1], cap / p.sub, p.sub % p.vec ? p.vec : 1);
    p.n1 = (p.L[p.a1] - 1) / p.e1 + 1;
    p.e0 = p.n1 == 1 ? even_cut(p.L[p.a0], cap / p.plane, 1) : 1;
  } else {
    p.sub = 1;
    p.e0 = even_cut(p.L[p.a0], cap, p.vec);            // a chain: plane = 1, and its one axis of extent > 1 is cut
  }
  p.n0 = (p.L[p.a0] - 1) / p.e0 + 1;
  p.bricks = p.n0 * p.n1;
  const size_t img = size_t(p.e0) * size_t(p.e1) * size_t(p.sub) * elem;
  NF_REQUIRE(img <= avail, "%s: the smallest brick of the lattice (%d, %d, %d, %d), %d x %d x %d sites (%zu B), does not fit "
             "the LDS (%zu B)", what, lattice[0], lattice[1], lattice[2], lattice[3], p.e0, p.e1, p.sub, img, avail);
  p.img_bytes = (img + 15) & ~size_t(15);
  p.lds = kMsScratch + p.img_bytes;
  p.lanes = ms_image_team(int64_t(p.e0) * p.e1 * p.sub);
  int np = 7;
  for (int mu = 0; mu < 4; ++mu) {
    p.poff[mu] = np - 7;
    np += mu == p.a0 ? p.e0 : mu == p.a1 ? p.e1 : p.L[mu];
  }
  p.n_part = np;
  return NF_OK;
}

size_t mt_workspace(int64_t N, const MtPlan &p) {
  if (N < 1) return 0;
  return (size_t(N) * size_t(p.bricks) * size_t(p.n_part) * sizeof(double) + 255) & ~size_t(255);
}

struct MtArgs {
  const void *cfgs;
  double *part;         // (N, bricks, n_part)
  int64_t V, plane;
  int L[4], off[4];     // off: the slice sums' offsets in a brick's partials
  int a0, a1, La0, La1, sub, e0, e1, n0, n1, lanes, n_part;
};

template <typename T, int VEC>
__global__ __launch_bounds__(kMsMaxLanes) void measure_bricks(MtArgs A) {
  extern __shared__ __align__(16) unsigned char mt_lds[];
  double *red = reinterpret_cast<double *>(mt_lds), *sp = red + kMsRed;
  T *img = reinterpret_cast<T *>(mt_lds + kMsScratch);
  const int tl = threadIdx.x;
  const unsigned bricks = unsigned(A.n0) * unsigned(A.n1);
  const int b = int(blockIdx.x % bricks);
  const int64_t row = blockIdx.x / bricks;
  const int p0 = b / A.n1 * A.e0, q0 = b % A.n1 * A.e1;               // the brick's first plane and first sub-plane
  const int E0 = A.e0 < A.La0 - p0 ? A.e0 : A.La0 - p0, E1 = A.e1 < A.La1 - q0 ? A.e1 : A.La1 - q0;   // the last may be short
  int E[4], Lext[4], off[4];
#pragma unroll
  for (int mu = 0; mu < 4; ++mu) {
    Lext[mu] = A.L[mu];
    off[mu] = A.off[mu];
    E[mu] = mu == A.a0 ? E0 : mu == A.a1 ? E1 : A.L[mu];
  }
  const T *rowp = static_cast<const T *>(A.cfgs) + row * A.V;
  const int64_t at1 = int64_t(q0) * A.sub;
  const T *src = rowp + int64_t(p0) * A.plane + at1;                 // n1 > 1 only with e0 = 1: the brick is one run
  const T *halo = A.n0 > 1 ? rowp + int64_t(p0 > 0 ? p0 - 1 : A.La0 - 1) * A.plane + at1 : nullptr;
  const T *halo1 = A.n1 > 1 ? rowp + int64_t(p0) * A.plane + int64_t(q0 > 0 ? q0 - 1 : A.La1 - 1) * A.sub : nullptr;
  const int n = E0 * E1 * A.sub;
  for (int u = tl; u < n / VEC; u += A.lanes) stage_w<T, VEC>(src + u * VEC, img + u * VEC);
  __syncthreads();
  double *dst = A.part + int64_t(blockIdx.x) * A.n_part;
  measure_image<T, true>(img, halo, halo1, E, Lext, off, A.a0, A.a1, tl, A.lanes, 0, 0, red, sp, dst, true);
}

struct MtFinish {
  const double *part;
  double *out;
  int64_t N;
  int L[4], goff[4], poff[4];
  int a0, a1, e0, e1, n0, n1, n_out, n_part;
};

// out[row, q] = the partials of q over the bricks that hold it, by one wave: lane l adds the bricks l, l + 64, ... of the
// list in order, then the shuffle tree
__global__ __launch_bounds__(kBlock) void measure_tiled_finish(MtFinish F) {
  const int64_t idx = int64_t(blockIdx.x) * kMtFinishTeams + threadIdx.x / kWave;     // the same for a whole wave
  if (idx >= F.N * F.n_out) return;
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t row = idx / F.n_out;
  const int q = int(idx % F.n_out);
  int pq = q, first = 0, step = 1, cnt = F.n0 * F.n1;
  if (q >= 7) {
#pragma unroll
    for (int mu = 0; mu < 4; ++mu) {
      const int t = q - 7 - F.goff[mu];
      if (t >= 0 && t < F.L[mu]) {
        if (mu == F.a0) { first = t / F.e0 * F.n1; cnt = F.n1; pq = 7 + F.poff[mu] + t % F.e0; }
        else if (mu == F.a1) { first = t / F.e1; step = F.n1; cnt = F.n0; pq = 7 + F.poff[mu] + t % F.e1; }
        else pq = 7 + F.poff[mu] + t;
      }
    }
  }
  const double *p = F.part + (row * (F.n0 * F.n1) + first) * F.n_part + pq;
  double r = 0;
  for (int j = lane; j < cnt; j += kWave) r += p[int64_t(j) * step * F.n_part];
  r = wave_sum(r);
  if (lane == 0) F.out[idx] = r;
}

template <typename T, int VEC>
int mt_run(const MtArgs &A, const MtPlan &p, int64_t groups, hipStream_t s) {
  auto kern = measure_bricks<T, VEC>;
  if (p.lds > 64 * 1024) {
    // once per instantiation, to the budget: no later call lowers it again
    static const hipError_t raised = hipFuncSetAttribute(
        reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, int(kMsLdsBudget));
    if (raised != hipSuccess) {
      (void)hipGetLastError();
      set_error("nf_lattice_measure_tiled: cannot raise the dynamic LDS limit to %zu B", kMsLdsBudget);
      return NF_ELAUNCH;
    }
  }
  hipLaunchKernelGGL(kern, dim3(unsigned(groups)), dim3(unsigned(p.lanes)), p.lds, s, A);
  return check_launch("nf_lattice_measure_tiled");
}

}  // namespace
}  // namespace nf

using namespace nf;

extern "C" int nf_lattice_measure_tiled_supported(const int32_t *lattice, size_t brick_bytes, int dtype) {
  MtPlan p;
  return mt_plan("nf_lattice_measure_tiled_supported", lattice, brick_bytes, dtype, p) == NF_OK ? 1 : 0;
}

extern "C" int nf_lattice_measure_tiled_plan(const int32_t *lattice, size_t brick_bytes, int dtype,
                                             nf_measure_tiled_plan *out) {
  NF_REQUIRE(out != nullptr, "nf_lattice_measure_tiled_plan: out is NULL");
  MtPlan p;
  const int rc = mt_plan("nf_lattice_measure_tiled_plan", lattice, brick_bytes, dtype, p);
  if (rc) return rc;
  out->axis0 = p.a0;
  out->axis1 = p.a1;
  out->e0 = p.e0;
  out->e1 = p.e1;
  out->n0 = p.n0;
  out->n1 = p.n1;
  out->bricks = p.bricks;
  out->lanes = p.lanes;
  out->vec = p.vec;
  out->n_out = p.n_out;
  out->n_part = p.n_part;
  out->reserved = 0;
  out->lds_bytes = int64_t(p.lds);
  out->lds_budget = int64_t(kMsLdsBudget);
  return NF_OK;
}

extern "C" size_t nf_lattice_measure_tiled_workspace(int64_t N, const int32_t *lattice, size_t brick_bytes, int dtype) {
  MtPlan p;
  if (mt_plan("nf_lattice_measure_tiled_workspace", lattice, brick_bytes, dtype, p) != NF_OK) return 0;
  return mt_workspace(N, p);
}

extern "C" int nf_lattice_measure_tiled(const void *cfgs, double *out, int64_t N, const int32_t *lattice, size_t brick_bytes,
                                        void *workspace, size_t workspace_bytes, int dtype, void *stream) {
  NF_REQUIRE(cfgs && out, "nf_lattice_measure_tiled: NULL pointer argument");
  NF_REQUIRE(N >= 0, "nf_lattice_measure_tiled: N (%lld) is negative", (long long)N);
  MtPlan p;
  const int rc = mt_plan("nf_lattice_measure_tiled", lattice, brick_bytes, dtype, p);
  if (rc) return rc;
  if (N == 0) return NF_OK;
  NF_REQUIRE(N <= kMsMaxGroups / p.bricks && (N * p.n_out + kMtFinishTeams - 1) / kMtFinishTeams <= kMsMaxGroups,
             "nf_lattice_measure_tiled: %lld rows need more than the %lld workgroups of one launch: measure them in several "
             "calls", (long long)N, (long long)kMsMaxGroups);
  const size_t need = mt_workspace(N, p);
  NF_REQUIRE(workspace != nullptr && workspace_bytes >= need, "nf_lattice_measure_tiled: workspace %zu B < %zu B needed",
             workspace ? workspace_bytes : size_t(0), need);
  NF_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0,
             "nf_lattice_measure_tiled: the workspace must be 8-byte aligned");
  MtArgs A{};
  A.cfgs = cfgs;
  A.part = static_cast<double *>(workspace);
  A.V = p.V; A.plane = p.plane;
  for (int mu = 0; mu < 4; ++mu) {
    A.L[mu] = p.L[mu];
    A.off[mu] = p.poff[mu];
  }
  A.a0 = p.a0; A.a1 = p.a1; A.La0 = p.L[p.a0]; A.La1 = p.a1 >= 0 ? p.L[p.a1] : 1; A.sub = p.sub;
  A.e0 = p.e0; A.e1 = p.e1; A.n0 = p.n0; A.n1 = p.n1; A.lanes = p.lanes; A.n_part = p.n_part;
  hipStream_t s = static_cast<hipStream_t>(stream);
  // 16-byte loads need every brick to start on 16 bytes: the plan's vec (whole units per brick) and the caller's pointer
  // aligned; either way the image, and with it every sum, is the same
  const bool wide = p.vec > 1 && (reinterpret_cast<uintptr_t>(cfgs) & 15) == 0;
  const int64_t groups = N * p.bricks;
  int rc2;
  if (dtype == NF_F32) rc2 = wide ? mt_run<float, 4>(A, p, groups, s) : mt_run<float, 1>(A, p, groups, s);
  else rc2 = wide ? mt_run<double, 2>(A, p, groups, s) : mt_run<double, 1>(A, p, groups, s);
  if (rc2) return rc2;
  MtFinish F{};
  F.part = A.part;
  F.out = out;
  F.N = N;
  for (int mu = 0; mu < 4; ++mu) {
    F.L[mu] = p.L[mu];
    F.goff[mu] = p.goff[mu];
    F.poff[mu] = p.poff[mu];
  }
  F.a0 = p.a0; F.a1 = p.a1; F.e0 = p.e0; F.e1 = p.e1; F.n0 = p.n0; F.n1 = p.n1; F.n_out = p.n_out; F.n_part = p.n_part;
  hipLaunchKernelGGL(measure_tiled_finish, dim3(unsigned((N * p.n_out + kMtFinishTeams - 1) / kMtFinishTeams)), dim3(kBlock),
                     0, s, F);
  return check_launch("nf_lattice_measure_tiled (finish)");
}

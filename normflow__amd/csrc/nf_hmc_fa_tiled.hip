// nf_hmc_fa_tiled.hip -- Fourier-accelerated hybrid Monte Carlo for the lattice phi^4 action with the chains in HBM and many
// workgroups per chain (MI355X-side extension; the rule is include/normflow_hip.h, "Fourier-accelerated hybrid Monte
// Carlo", and the entry is described there under "the same with the chains in HBM").  nf_phi4_hmc_fa's trajectory for the
// lattices beyond one CU's LDS, from two building blocks:
//   * the filter x <- T diag(d) T x over HBM (hmc_fa_pass, below), T = H_{L_0} x .. x H_{L_3} by the axis pass of
//     nf_spectral_core.h on panels staged in LDS;
//   * the marched drift-and-kick step of nf_hmc_tiled_core.h with the velocity v = A pi as a separate operand (VEL).
// The filter.  The four axes are cut into g groups of adjacent axes.  A pass of group [lo, hi] gives every workgroup one
// panel: the full extents of the group's axes times a run of the remaining sites -- `ri` sites along the sites behind the
// group (contiguous in memory), or, where the run covers all of them, `ro` values of the index in front of the group (the
// panel is then one contiguous stretch).  The panel is the row-major array (ro, L_lo, .., L_hi, ri) in LDS; the axis pass
// runs on it with the stride of the axis in that array; the panel goes back to where it came from (or into another
// buffer: the first pass of a filter reads pi and writes v).  A filter is 2 g - 1 passes: the groups from the fastest to
// the slowest forward, diag(d) inside the slowest group's pass between its forward and its backward transform (that
// group holds axis 0, so the panel index gives the momentum index), the other groups back.  The single axes are always
// transformed in the order 3, 2, 1, 0 | multiply | 0, 1, 2, 3, and a line's arithmetic depends on the line and its matrix
// alone (a column of the matrix-core product), so phi and pi do not depend on the cut, bit for bit.
// A trajectory is a fixed line of launches on the caller's stream:
//   draw (eta, as nf_normal_sample) | refresh filter a^(-1/2): pi        (both skipped with pi_in)
//   H0 filter a: v | begin: the partials of sum pi v / 2 and S(phi), pi -= (b_s / 2) dt F(phi)
//   per stage: filter a: v | step: phi' = phi + a_j dt v, pi' = pi - b_j dt F(phi')
//   H1 filter a: v | the partials of the end | commit (nf_hmc_tiled_core.h: decision, copy of the accepted chains, record)
// that is (n_md s + 3) (2 g - 1) + n_md s + 4 launches.  Energies: per-workgroup partials in double, added in a fixed order
// by commit, no atomics.  The plan depends on the lattice, the dtype and the cut alone.
#include <cstddef>

#include "nf_hmc_tiled_core.h"
#include "nf_spectral_core.h"

namespace nf {

constexpr int kFaTiledLanes = 512;                      // of a pass: 2 waves per SIMD, 256 registers for the transform's tiles
constexpr size_t kFaTiledLdsMax = 160 * 1024;           // LDS of a CU: what a pass may take at all
constexpr size_t kFaTiledLdsTarget = 80 * 1024;         // two workgroups per CU: what the planner aims for
constexpr size_t kFaTiledPanel = 32 * 1024;             // bytes of a panel the planner aims for
constexpr size_t kFaTiledRunBytes = 64;                 // a run along the remaining sites should be this long at least
constexpr int kFaTiledMaxTable = 4 * kSpecMaxAxis;
enum { kFaFwd = 1, kFaMul = 2, kFaBwd = 4 };

struct FaGroup {
  int lo, hi;            // the axes of lattice[4]
  int G, O, I;           // sites of the group's axes, in front of them, behind them
  int Ro, Ri, nro, nri;  // the run (Ro > 1 only where Ri == I) and the runs per chain
  int lanes, hm_off;     // of a workgroup; element offset of the matrices in LDS
  size_t lds, hbytes, stretch;   // stretch: contiguous bytes of a panel row
  bool eligible;         // the run reaches kFaTiledRunBytes inside kFaTiledLdsTarget
  HartleyAxes ax;
};

struct FaTiledPlan {
  int64_t V;
  int L[4];
  int cut, g;
  FaGroup grp[4];        // the slowest group first
  TiledPlan step;
};

static bool fa_size_group(FaGroup &q, const int L[4], size_t elem) {
  int n[4] = {1, 1, 1, 1};
  q.G = q.O = q.I = 1;
  for (int a = 0; a < 4; ++a) {
    if (a < q.lo) q.O *= L[a];
    else if (a > q.hi) q.I *= L[a];
    else { q.G *= L[a]; n[a] = L[a]; }
  }
  spectral_axes(q.ax, n);
  q.hbytes = size_t(q.ax.hsize) * elem;
  const size_t unit = size_t(q.G) * elem;
  if (unit + q.hbytes > kFaTiledLdsMax) return false;
  const size_t budget = (unit + q.hbytes <= kFaTiledLdsTarget ? kFaTiledLdsTarget : kFaTiledLdsMax) - q.hbytes;
  const int vec = int(16 / elem);
  const size_t rmin = q.I > 1 ? (size_t(q.I) < kFaTiledRunBytes / elem ? size_t(q.I) : kFaTiledRunBytes / elem) : 1;
  q.eligible = unit * rmin + q.hbytes <= kFaTiledLdsTarget;
  size_t want = kFaTiledPanel > unit * rmin ? kFaTiledPanel : unit * rmin;
  if (want > budget) want = budget;
  const int64_t cap = int64_t(want / unit);            // sites of the run, >= 1
  q.Ri = 1;
  if (q.I > 1) {
    const int rmax = int(cap < q.I ? cap : q.I);
    const int nr = (q.I - 1) / rmax + 1;
    q.Ri = (q.I - 1) / nr + 1;
    const int up = (q.Ri + vec - 1) / vec * vec;
    if (up <= rmax) q.Ri = up;
  }
  q.Ro = 1;
  if (q.Ri == q.I) {
    int64_t omax = cap / q.I;
    omax = omax < 1 ? 1 : omax > q.O ? q.O : omax;
    const int no = int((q.O - 1) / omax + 1);
    q.Ro = (q.O - 1) / no + 1;
  }
  q.nri = (q.I - 1) / q.Ri + 1;
  q.nro = (q.O - 1) / q.Ro + 1;
  const int64_t sites = int64_t(q.Ro) * q.G * q.Ri;
  q.hm_off = int((sites + vec - 1) / vec * vec);
  q.lds = size_t(q.hm_off) * elem + q.hbytes;
  q.stretch = (q.Ri == q.I ? size_t(sites) : size_t(q.Ri)) * elem;
  const int64_t lanes = ((sites + 7) / 8 + kWave - 1) / kWave * kWave;
  q.lanes = int(lanes > kFaTiledLanes ? kFaTiledLanes : lanes);
  return q.lds <= kFaTiledLdsMax;
}

// the groups of the cut `mask` (bit mu: a boundary between axis mu and mu + 1), sized; false where a group does not fit
static bool fa_cut(FaTiledPlan &p, int mask, size_t elem, int *bad) {
  p.cut = mask;
  p.g = 0;
  for (int a = 0, lo = 0; a < 4; ++a)
    if (a == 3 || (mask >> a & 1)) {
      FaGroup &q = p.grp[p.g];
      q.lo = lo;
      q.hi = a;
      if (!fa_size_group(q, p.L, elem)) {
        if (bad) *bad = p.g;
        return false;
      }
      ++p.g;
      lo = a + 1;
    }
  return true;
}

// The one planner: _supported, _plan and _workspace answer from it and nf_phi4_hmc_fa_tiled launches by it.  cut = -1:
// among the legal cuts, those whose every run reaches 64 bytes inside 80 KiB of LDS before the others, then the fewest
// groups, then the longest shortest contiguous stretch, then the smallest mask.
static int fa_tiled_plan(const char *what, const int32_t *lattice, int dtype, int cut, FaTiledPlan &p) {
  NF_REQUIRE(lattice != nullptr, "%s: lattice is NULL", what);
  NF_REQUIRE(dtype == NF_F32 || dtype == NF_F64, "%s: unsupported dtype %d (float32 and float64 fields)", what, dtype);
  const size_t elem = dtype == NF_F32 ? 4 : 8;
  p = FaTiledPlan{};
  for (int mu = 0; mu < 4; ++mu) {
    NF_REQUIRE(lattice[mu] >= 1, "%s: lattice extents must be >= 1", what);
    NF_REQUIRE(lattice[mu] <= kSpecMaxAxis, "%s: axis of %d sites (1 to %d fit the transform of a panel)", what, lattice[mu],
               kSpecMaxAxis);
    p.L[mu] = lattice[mu];
  }
  const int rc = tiled_plan(what, lattice, dtype, p.step);       // V < 2^31, and the step's tiles
  if (rc) return rc;
  p.V = p.step.V;
  NF_REQUIRE(cut >= -1 && cut <= 7, "%s: cut (%d) must be -1 (the planner's choice) or a mask of the 3 boundaries, 0 .. 7", what,
             cut);
  auto legal = [&](int mask, int *at) {
    for (int mu = 0; mu < 3; ++mu)
      if ((mask >> mu & 1) && (p.L[mu] == 1 || p.L[mu + 1] == 1)) {
        if (at) *at = mu;
        return false;
      }
    return true;
  };
  if (cut >= 0) {
    int at = 0, bad = 0;
    NF_REQUIRE(legal(cut, &at), "%s: cut %d puts a boundary between the axes %d and %d of the lattice (%d, %d, %d, %d), next "
               "to an axis of extent 1", what, cut, at, at + 1, p.L[0], p.L[1], p.L[2], p.L[3]);
    if (!fa_cut(p, cut, elem, &bad)) {
      const FaGroup &q = p.grp[bad];
      set_error("%s: cut %d: the group of the axes %d .. %d (%d sites, %zu B, and %zu B of Hartley matrices) does not fit the "
                "%zu B of LDS", what, cut, q.lo, q.hi, q.G, size_t(q.G) * elem, q.hbytes, kFaTiledLdsMax);
      return NF_EINVAL;
    }
    return NF_OK;
  }
  int best = -1, best_g = 0;
  bool best_ok = false;
  size_t best_stretch = 0;
  for (int mask = 0; mask < 8; ++mask) {
    FaTiledPlan t = p;
    if (!legal(mask, nullptr) || !fa_cut(t, mask, elem, nullptr)) continue;
    bool ok = true;
    size_t stretch = size_t(-1);
    for (int i = 0; i < t.g; ++i) {
      ok = ok && t.grp[i].eligible;
      stretch = t.grp[i].stretch < stretch ? t.grp[i].stretch : stretch;
    }
    const bool better = best < 0 || (ok != best_ok ? ok : t.g != best_g ? t.g < best_g : stretch > best_stretch);
    if (better) {
      best = mask; best_ok = ok; best_g = t.g; best_stretch = stretch;
    }
  }
  NF_REQUIRE(best >= 0, "%s: no cut of the lattice (%d, %d, %d, %d) into groups of adjacent axes fits the %zu B of LDS", what,
             p.L[0], p.L[1], p.L[2], p.L[3], kFaTiledLdsMax);
  fa_cut(p, best, elem, nullptr);
  return NF_OK;
}

struct FaPassArgs {
  const void *src;
  void *dst;
  int64_t V;
  int L[4];
  int lo, hi, G, O, I;
  int Ro, Ri, nri;
  int mode, refresh, hm_off;
  int toff[4];
  double w0, m2;
  HartleyAxes ax;
  double table[kFaTiledMaxTable];   // shat of the four extents (nf_phi4_hmc_fa_table)
};

// One pass of a filter: blockIdx.x the panel of chain blockIdx.y.  VEC sites per global access (the host has checked
// that every row of every panel starts and ends on 16 bytes).  src and dst may be the same buffer: a workgroup reads its
// panel whole before it writes it, and panels do not overlap.  Every barrier is in uniform control flow.
template <typename T, int VEC>
__global__ __launch_bounds__(kFaTiledLanes) void hmc_fa_pass(FaPassArgs A) {
  extern __shared__ __align__(16) unsigned char fa_tiled_lds[];
  T *buf = reinterpret_cast<T *>(fa_tiled_lds);
  T *hm = buf + A.hm_off;
  const int tid = threadIdx.x, NT = blockDim.x;
  const int64_t c = blockIdx.y;
  const int bo = blockIdx.x / A.nri, bi = blockIdx.x - bo * A.nri;
  const int o0 = bo * A.Ro, ro = min(A.Ro, A.O - o0);
  const int r0 = bi * A.Ri, ri = min(A.Ri, A.I - r0);
  const bool contig = ri == A.I;                         // then r0 = 0 and the panel is one stretch of memory
  const int rows = contig ? 1 : A.G;                     // ro = 1 unless contig
  const int rowlen = contig ? ro * A.G * A.I : ri;
  const int P = ro * A.G * ri;                           // sites of the panel, <= Ro G Ri = what the host sized the LDS for
  const T *gsrc = static_cast<const T *>(A.src) + c * A.V + (int64_t(o0) * A.G * A.I + r0);
  T *gdst = static_cast<T *>(A.dst) + c * A.V + (int64_t(o0) * A.G * A.I + r0);
  const int upr = rowlen / VEC, units = rows * upr;

  build_hartley(hm, A.ax, NT);
  for (int u = tid; u < units; u += NT) {
    const int row = u / upr, r = (u - row * upr) * VEC;
    T v[VEC];
    load_w<T, VEC>(gsrc + (int64_t(row) * A.I + r), v);
    store_w<T, VEC>(buf + u * VEC, v);
  }
  __syncthreads();

  // the kernel's argument segment in the constant address space: the table is read at variable indices (nf_hmc_fa.hip)
  using KernArgByte = const __attribute__((address_space(4))) unsigned char;
  using KernArgDouble = const __attribute__((address_space(4))) double;
  KernArgByte *seg = (KernArgByte *)__builtin_amdgcn_kernarg_segment_ptr();
  KernArgDouble *table = reinterpret_cast<KernArgDouble *>(seg + offsetof(FaPassArgs, table));

  // steps 0 .. 3: the axes 3, 2, 1, 0 forward; step 4: the multiply; steps 5 .. 8: the axes 0, 1, 2, 3 back -- of which
  // this pass does the ones of its group and its mode.  One loop, so that the axis pass is in the code once.
#pragma unroll 1
  for (int s = 0; s < 9; ++s) {
    if (s == 4) {
      if (!(A.mode & kFaMul)) continue;
      // the slowest group holds axis 0: O = 1, and site gi ri + r of the panel is momentum index gi I + r0 + r
      for (int idx = tid; idx < P; idx += NT) {
        const int gi = idx / ri, r = idx - gi * ri;
        int i = gi * A.I + r0 + r;
        const int x3 = i % A.L[3]; i /= A.L[3];
        const int x2 = i % A.L[2]; i /= A.L[2];
        const int x1 = i % A.L[1];
        const int x0 = i / A.L[1];
        double den;
        {
#pragma clang fp contract(off)
          const double sh = ((table[A.toff[0] + x0] + table[A.toff[1] + x1]) + table[A.toff[2] + x2]) + table[A.toff[3] + x3];
          const double hop = A.w0 * sh;
          den = hop + A.m2;
        }
        buf[idx] *= A.refresh ? T(::sqrt(den)) : T(1.0 / den);
      }
      __syncthreads();
      continue;
    }
    const bool fwd = s < 4;
    if (!(A.mode & (fwd ? kFaFwd : kFaBwd))) continue;
    const int a = fwd ? 3 - s : s - 5;
    if (a < A.lo || a > A.hi) continue;
    const int N = A.L[a];
    if (N <= 1) continue;
    int S = ri;
    for (int b = a + 1; b <= A.hi; ++b) S *= A.L[b];
    const T *h = hm + A.ax.hoff[a];
    const int ldh = A.ax.ldh[a], lines = P / N;
    if (N <= 16) axis_pass<T, 1>(buf, h, ldh, N, S, lines, NT);
    else if (N <= 32) axis_pass<T, 2>(buf, h, ldh, N, S, lines, NT);
    else if (N <= 48) axis_pass<T, 3>(buf, h, ldh, N, S, lines, NT);
    else axis_pass<T, 4>(buf, h, ldh, N, S, lines, NT);
  }

  for (int u = tid; u < units; u += NT) {
    const int row = u / upr, r = (u - row * upr) * VEC;
    T v[VEC];
    load_w<T, VEC>(buf + u * VEC, v);
    store_w<T, VEC>(gdst + (int64_t(row) * A.I + r), v);
  }
}

// eta (C, V) as nf_normal_sample lays it out: Philox group q of chain c holds the sites q PER + j
template <typename T>
__global__ __launch_bounds__(kTiledLanes) void hmc_fa_draw(T *eta, int64_t V, PhiloxPos pos) {
  constexpr int PER = sizeof(T) == 4 ? 4 : 2;
  const int64_t ngroups = (V + PER - 1) / PER, c = blockIdx.y;
  T *out = eta + c * V;
  for (int64_t q = int64_t(blockIdx.x) * kTiledLanes + threadIdx.x; q < ngroups; q += int64_t(gridDim.x) * kTiledLanes) {
    T z[PER];
    philox_normal_group<T>(pos, uint64_t(c) * uint64_t(ngroups) + uint64_t(q), z);
#pragma unroll
    for (int j = 0; j < PER; ++j)
      if (q * PER + j < V) out[q * PER + j] = z[j];
  }
}

static int64_t fa_tiled_launches(const FaTiledPlan &p, int64_t evals) {
  const int64_t passes = 2 * p.g - 1;
  return (evals + 3) * passes + evals + 4;
}

static size_t fa_tiled_workspace(int64_t C, const FaTiledPlan &p, size_t elem) {
  return round256(size_t(C) * size_t(p.step.tiles) * 4 * sizeof(double)) + 5 * round256(size_t(C) * size_t(p.V) * elem);
}

static int fa_raise(const void *kern, size_t lds, const char *what) {
  if (lds <= 64 * 1024) return NF_OK;
  if (hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)) != hipSuccess) {
    (void)hipGetLastError();
    set_error("%s: cannot raise the dynamic LDS limit to %zu B", what, lds);
    return NF_ELAUNCH;
  }
  return NF_OK;
}

struct FaTiledCall {
  double w0, w2, w4, m2;
  bool wide;               // the caller's fields and the workspace are 16-byte aligned
  const double *table;
};

template <typename T>
struct FaTiledRun {
  static constexpr int W = int(16 / sizeof(T));
  const char *what;
  const FaTiledPlan &p;
  const FaTiledCall &F;
  int64_t C;
  hipStream_t s;

  // one pass of group i
  int pass(int i, int mode, bool refresh, const void *src, void *dst) const {
    const FaGroup &q = p.grp[i];
    FaPassArgs A{};
    A.src = src; A.dst = dst; A.V = p.V;
    for (int a = 0, at = 0; a < 4; ++a) {
      A.L[a] = p.L[a];
      A.toff[a] = at;
      at += p.L[a];
    }
    for (int k = 0; k < A.toff[3] + p.L[3]; ++k) A.table[k] = F.table[k];
    A.lo = q.lo; A.hi = q.hi; A.G = q.G; A.O = q.O; A.I = q.I;
    A.Ro = q.Ro; A.Ri = q.Ri; A.nri = q.nri;
    A.mode = mode; A.refresh = refresh; A.hm_off = q.hm_off;
    A.w0 = F.w0; A.m2 = F.m2; A.ax = q.ax;
    // 16-byte accesses: every row of every panel starts and ends on 16 bytes
    const bool wide = F.wide && W > 1 && (int64_t(q.G) * q.I) % W == 0 && (q.I == 1 || q.Ri == q.I || (q.I % W == 0 && q.Ri % W == 0));
    auto kw = hmc_fa_pass<T, W>;
    auto k1 = hmc_fa_pass<T, 1>;
    auto kern = wide ? kw : k1;
    int rc = fa_raise(reinterpret_cast<const void *>(kern), q.lds, what);
    if (rc) return rc;
    hipLaunchKernelGGL(kern, dim3(unsigned(q.nro * q.nri), unsigned(C)), dim3(unsigned(q.lanes)), q.lds, s, A);
    return check_launch(what);
  }

  // dst <- T diag(d) T src, d = a^(-1/2) (refresh) or a; src is left alone
  int filter(bool refresh, const void *src, void *dst) const {
    int rc;
    const void *from = src;
    for (int i = p.g - 1; i >= 1; --i) {
      if ((rc = pass(i, kFaFwd, refresh, from, dst))) return rc;
      from = dst;
    }
    if ((rc = pass(0, kFaFwd | kFaMul | kFaBwd, refresh, from, dst))) return rc;
    for (int i = 1; i < p.g; ++i)
      if ((rc = pass(i, kFaBwd, refresh, dst, dst))) return rc;
    return NF_OK;
  }

  template <int VEC>
  int step(int mode, const TiledVelArgs &A) const {
    auto k0 = hmc_tiled_step<T, VEC, 0, false, true>;
    auto k1 = hmc_tiled_step<T, VEC, 1, false, true>;
    auto k3 = hmc_tiled_step<T, VEC, 3, false, true>;
    auto kern = mode == 0 ? k0 : mode == 1 ? k1 : k3;
    int rc = fa_raise(reinterpret_cast<const void *>(kern), p.step.lds, what);
    if (rc) return rc;
    hipLaunchKernelGGL(kern, dim3(unsigned(p.step.tiles), unsigned(C)), dim3(kTiledLanes), p.step.lds, s, A);
    return check_launch(what);
  }

  template <int VEC>
  int run(const HmcCall &K, const HmcSteps &st, unsigned char *ws) const {
    const TiledPlan &tp = p.step;
    const size_t field = round256(size_t(C) * size_t(p.V) * sizeof(T));
    double *part = reinterpret_cast<double *>(ws);
    unsigned char *base = ws + round256(size_t(C) * size_t(tp.tiles) * 4 * sizeof(double));
    void *fphi[2] = {base, base + field}, *fpi[2] = {base + 2 * field, base + 3 * field}, *vel = base + 4 * field;
    TiledVelArgs A{};
    A.V = p.V;
    for (int a = 0; a < 4; ++a) {
      A.L[a] = tp.L[a];
      A.T[a] = tp.T[a];
      A.n[a] = tp.n[a];
    }
    A.ring = tp.ring; A.tiles = tp.tiles;
    A.w0 = F.w0; A.w2 = F.w2; A.w4 = F.w4;
    A.vel_src = vel;
    const int evals = K.n_md * st.stages;
    const int64_t ngroups = (p.V + W - 1) / W;
    const int64_t dblocks = (ngroups + kTiledLanes - 1) / kTiledLanes;
    int rc;
    for (int t = 0; t < K.n_traj; ++t) {
      const void *pisrc = K.pi_in;
      int nxt = 0;                                       // the momentum buffer the next launch writes
      if (!pisrc) {
        // eta into the velocity buffer, pi = A^(-1/2) eta into the first momentum buffer
        const PhiloxPos pos = philox_pos(K.seed, NF_PHILOX_KEY_DOMAIN, K.offset + 2 * uint64_t(t));
        hipLaunchKernelGGL(hmc_fa_draw<T>, dim3(unsigned(dblocks < 4096 ? dblocks : 4096), unsigned(C)), dim3(kTiledLanes), 0, s,
                           static_cast<T *>(vel), p.V, pos);
        if ((rc = check_launch(what))) return rc;
        if ((rc = filter(true, vel, fpi[0]))) return rc;
        pisrc = fpi[0];
        nxt = 1;
      }
      if ((rc = filter(false, pisrc, vel))) return rc;
      A.part = part;
      A.phi_src = K.phi; A.pi_src = pisrc; A.phi_dst = nullptr; A.pi_dst = fpi[nxt];
      A.dt = 0.0;
      A.eps = st.kick_half;
      if ((rc = step<VEC>(0, A))) return rc;
      pisrc = fpi[nxt];
      nxt ^= 1;
      const void *src = K.phi;
      for (int k = 1, j = 0; k <= evals; ++k, j = j + 1 == st.stages ? 0 : j + 1) {
        if ((rc = filter(false, pisrc, vel))) return rc;
        A.phi_src = src; A.pi_src = pisrc; A.phi_dst = fphi[k & 1]; A.pi_dst = fpi[nxt];
        A.dt = st.drift[j];
        A.eps = k == evals ? st.kick_half : st.kick[j];
        if ((rc = step<VEC>(1, A))) return rc;
        src = A.phi_dst;
        pisrc = fpi[nxt];
        nxt ^= 1;
      }
      if ((rc = filter(false, pisrc, vel))) return rc;
      A.phi_src = src; A.pi_src = pisrc; A.phi_dst = nullptr; A.pi_dst = nullptr;
      A.dt = 0.0;
      A.eps = 0.0;
      if ((rc = step<VEC>(3, A))) return rc;
      CommitArgs Q{};
      Q.phi = K.phi; Q.prop = src; Q.pi_fin = pisrc;
      const bool due = K.record && (t + 1) % K.record_every == 0;
      Q.record = due ? static_cast<T *>(K.record) + int64_t((t + 1) / K.record_every - 1) * C * p.V : nullptr;
      Q.pi_out = t + 1 == K.n_traj ? K.pi_out : nullptr;
      Q.part = part;
      Q.dh_out = K.dh_out + int64_t(t) * C;
      Q.accept_out = K.accept_out + int64_t(t) * C;
      Q.action_out = K.action_out;
      Q.V = p.V; Q.tiles = tp.tiles; Q.force = K.force;
      Q.pos = philox_pos(K.seed, NF_PHILOX_ACCEPT_DOMAIN, K.offset + 2 * uint64_t(t) + 1);
      hipLaunchKernelGGL((hmc_tiled_commit<T, false>), dim3(tiled_commit_blocks(p.V), unsigned(C)), dim3(kTiledLanes), 0, s, Q);
      if ((rc = check_launch(what))) return rc;
    }
    return NF_OK;
  }
};

}  // namespace nf

using namespace nf;

extern "C" int nf_phi4_hmc_fa_tiled_supported(const int32_t *lattice, int dtype) {
  FaTiledPlan p;
  return fa_tiled_plan("nf_phi4_hmc_fa_tiled_supported", lattice, dtype, -1, p) == NF_OK ? 1 : 0;
}

extern "C" int nf_phi4_hmc_fa_tiled_plan(const int32_t *lattice, int dtype, int cut, int n_md, int stages,
                                         nf_hmc_fa_tiled_plan *out) {
  const char *what = "nf_phi4_hmc_fa_tiled_plan";
  NF_REQUIRE(out != nullptr, "%s: out is NULL", what);
  NF_REQUIRE(n_md >= 1 && stages >= 1 && stages <= NF_HMC_MAX_STAGES, "%s: n_md (%d) must be >= 1 and stages (%d) in 1 .. %d",
             what, n_md, stages, NF_HMC_MAX_STAGES);
  FaTiledPlan p;
  const int rc = fa_tiled_plan(what, lattice, dtype, cut, p);
  if (rc) return rc;
  *out = nf_hmc_fa_tiled_plan{};
  out->cut = p.cut;
  out->groups = p.g;
  out->passes = 2 * p.g - 1;
  for (int i = 0; i < p.g; ++i) {
    const FaGroup &q = p.grp[i];
    out->first[i] = q.lo;
    out->last[i] = q.hi;
    out->run[i] = q.Ro * q.Ri;
    out->run_inner[i] = q.Ri;
    out->panels[i] = q.nro * q.nri;
    out->lanes[i] = q.lanes;
    out->panel_sites[i] = int64_t(q.Ro) * q.G * q.Ri;
    out->lds_bytes[i] = int64_t(q.lds);
    out->matrix_bytes[i] = int64_t(q.hbytes);
  }
  out->filters = int64_t(n_md) * stages + 3;
  out->launches = fa_tiled_launches(p, int64_t(n_md) * stages);
  tiled_plan_out(p.step, &out->step);
  return NF_OK;
}

extern "C" size_t nf_phi4_hmc_fa_tiled_workspace(int64_t C, const int32_t *lattice, int dtype) {
  FaTiledPlan p;
  if (C < 1 || fa_tiled_plan("nf_phi4_hmc_fa_tiled_workspace", lattice, dtype, -1, p) != NF_OK) return 0;
  return fa_tiled_workspace(C, p, dtype == NF_F32 ? 4 : 8);
}

extern "C" int nf_phi4_hmc_fa_tiled(void *phi, double *action_out, const void *pi_in, void *pi_out, double *dh_out,
                                    uint8_t *accept_out, void *record, int record_every, int64_t C, const int32_t *lattice,
                                    double w0, double w2, double w4, int n_md, double dt, int n_traj, int force_accept,
                                    uint64_t seed, uint64_t offset, void *workspace, size_t workspace_bytes, int dtype,
                                    void *stream, const nf_hmc_scheme *scheme, double fa_mass_sq, int cut) {
  const char *what = "nf_phi4_hmc_fa_tiled";
  HmcSteps st;
  int rc = hmc_steps(what, scheme, dt, st);              // the scheme first, as the other launchers do
  if (rc) return rc;
  const HmcCall K{phi, action_out, pi_in, pi_out, dh_out, accept_out, record, record_every, C, n_md, n_traj,
                  force_accept != 0, seed, offset};
  rc = hmc_call_checks(what, K);
  FaTiledPlan p;
  if (!rc) rc = fa_tiled_plan(what, lattice, dtype, cut, p);
  if (rc) return rc;
  int64_t groups = p.step.tiles;
  for (int i = 0; i < p.g; ++i) groups = groups > int64_t(p.grp[i].nro) * p.grp[i].nri ? groups : int64_t(p.grp[i].nro) * p.grp[i].nri;
  NF_REQUIRE(groups * C <= kTiledMaxGroups, "%s: %lld workgroups per chain x %lld chains exceed the %lld workgroups of one "
             "launch: run the chains in several calls", what, (long long)groups, (long long)C, (long long)kTiledMaxGroups);
  const int64_t evals = int64_t(n_md) * st.stages;
  const int64_t launches = fa_tiled_launches(p, evals) * int64_t(n_traj);
  NF_REQUIRE(launches <= NF_HMC_TILED_MAX_LAUNCHES,
             "%s: ((n_md s + 3) (2 g - 1) + n_md s + 4) n_traj = %lld launches (s = %d stages, g = %d groups) exceed "
             "NF_HMC_TILED_MAX_LAUNCHES (%d): split the run into several calls", what, (long long)launches, st.stages, p.g,
             NF_HMC_TILED_MAX_LAUNCHES);
  const size_t elem = dtype == NF_F32 ? 4 : 8;
  const size_t need = fa_tiled_workspace(C, p, elem);
  NF_REQUIRE(workspace != nullptr && workspace_bytes >= need, "%s: workspace %zu B < %zu B needed", what,
             workspace ? workspace_bytes : size_t(0), need);
  NF_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "%s: the workspace must be 8-byte aligned", what);
  // the operator last, so that every refusal above can be met without a launch behind it
  NF_REQUIRE(std::isfinite(fa_mass_sq), "%s: fa_mass_sq (%g) is not finite", what, fa_mass_sq);
  NF_REQUIRE(fa_mass_sq > 0.0, "%s: fa_mass_sq (%g) must be > 0: a(k) = 1 / (w0 khat^2 + M^2) at k = 0", what, fa_mass_sq);
  NF_REQUIRE(w0 >= 0.0, "%s: w0 (%g) must be >= 0: a(k) = 1 / (w0 khat^2 + M^2) must stay positive", what, w0);
  double table[kFaTiledMaxTable];
  rc = nf_phi4_hmc_fa_table(lattice, table);
  if (rc) return rc;
  const uintptr_t bits = reinterpret_cast<uintptr_t>(phi) | reinterpret_cast<uintptr_t>(pi_in) |
                         reinterpret_cast<uintptr_t>(workspace);
  const FaTiledCall F{w0, w2, w4, fa_mass_sq, (bits & 15) == 0, table};
  hipStream_t s = static_cast<hipStream_t>(stream);
  unsigned char *ws = static_cast<unsigned char *>(workspace);
  const bool wide = p.step.vec > 1 && F.wide;
  if (dtype == NF_F32) {
    const FaTiledRun<float> R{what, p, F, C, s};
    return wide ? R.run<4>(K, st, ws) : R.run<1>(K, st, ws);
  }
  const FaTiledRun<double> R{what, p, F, C, s};
  return wide ? R.run<2>(K, st, ws) : R.run<1>(K, st, ws);
}

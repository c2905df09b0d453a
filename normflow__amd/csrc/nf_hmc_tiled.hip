// nf_hmc_tiled.hip -- hybrid Monte Carlo for the lattice phi^4 action with the chains in HBM and many workgroups per chain
// (MI355X-side extension, no counterpart in the reference).  The third implementation of the one definition of
// normflow__amd/mcmc/hmc.py, for the lattices whose chain does not fit the LDS image of nf_phi4_hmc (nf_hmc.hip): the same
// leapfrog, the same energies in double, the same accept rule, the same two Philox draws per trajectory -- the draws, the
// rule and the site terms of F and S through nf_sampler_core.h, which both kernels call.
//
// A trajectory is n_md + 2 launches on the caller's stream:
//   begin    pi <- the draw of nf_normal_sample at (seed, offset + 2 t), or pi_in;  per-tile partials of sum pi^2 / 2 and S(phi);
//            pi <- pi - (dt / 2) F(phi)
//   step     n_md times: phi' = phi + dt pi and pi' = pi - eps F(phi') in ONE pass from one pair of buffers into the other
//            (eps = dt, dt / 2 on the last step, which also writes the partials of sum pi'^2 / 2 and S(phi'))
//   commit   every workgroup of a chain adds the chain's tile partials in tile order, draws u as nf_block_accept does at
//            (seed, offset + 2 t + 1) and decides; accepted chains get the proposal copied into phi, rejected chains are not
//            written at all; the record row is written when due
// begin and step are one kernel template.  The lattice's axes of extent 1 are dropped (no site moves); the slowest of
// three or four remaining axes is MARCHED: a workgroup owns a tile of the other axes and walks a segment of the marched
// axis plane by plane with a ring of four planes of phi' in LDS.  Loading plane p computes phi' = phi + dt pi ONCE for the
// tile's sites of that plane and for its one-site halo on the tiled axes (faces only, no corners), then one barrier, then
// the force on plane p - 1 from the ring (planes p - 2, p - 1, p) and the stores of phi' and pi' of plane p - 1.  Ring depth
// four makes the one barrier enough: the slot loaded in iteration p + 1 was last read in iteration p - 1.  A segment of t
// planes loads t + 2, so the redundant reads are the halo of a (d - 1)-dimensional tile plus 2 / t, where a plain box tile
// in four dimensions pays a halo on every axis.  Lattices of one or two axes have no marched axis: one plane, one slot.
// An axis that one tile covers has no halo: the neighbours wrap inside the tile.  The momenta of a tile's own sites wait
// in LDS (lane-private entries, two planes) between the load of their plane and the force one iteration later.
// Energies: lane partial over the lane's sites in plane order, wave shuffle tree, waves in order, tiles in order -- all in
// double, no atomics, the same inputs give the same bits; the plan does not depend on C, so a chain's result does not
// depend on the chains it shares a launch with.
// nf_phi4_hmc_tiled_ladder: the same kernels compiled with LADDER.  begin and step take the coefficients of the chain
// their workgroup works on from row rung[c] of a table; commit writes dH, the accept flag and the record row at the
// rung-ordered column (c / K) K + rung[c].  The same launches, the same workspace, the same plan.
// Integration schemes (the _scheme entry points; include/normflow_hip.h): the step kernel always took its drift length
// (dt) and its kick length (eps) per launch, so a scheme of s stages is n_md s step launches with the lengths a_j dt and
// b_j dt of HmcSteps (nf_sampler_core.h), begin kicking by (b_s / 2) dt and the last launch likewise; leapfrog is s = 1.
#include <type_traits>

#include "nf_sampler_core.h"

namespace nf {

constexpr int kTiledLanes = 256;
constexpr int kTiledRing = 4;                     // planes of phi' in LDS along a marched axis
constexpr int kTiledUnits = 8;                    // units (1 site, or 16 bytes of sites) of a plane tile per lane, at most
constexpr int kTiledPlaneSites = kTiledLanes * kTiledUnits;   // sites of a plane tile, at most
constexpr int kTiledSegment = 8;                  // planes of a marched segment, at most: 10 planes loaded for 8 updated
constexpr size_t kTiledScratch = 256;             // the reduction slots, in front of the ring
constexpr size_t kTiledLdsBudget = 80 * 1024;     // two workgroups per CU (160 KiB)
constexpr int64_t kTiledMaxGroups = (int64_t(1) << 24) - 1;   // workgroups of a launch: 256 lanes each, below 2^32 lanes

struct TiledPlan {
  int64_t V;
  int L[4];       // slot 0: the marched axis (extent 1 = none); slots 1 .. 3: the axes of a plane, the fastest last
  int ax[4];      // the caller's axis behind each slot, -1 for a filler of extent 1
  int T[4];       // tile extents (the last tile of an axis may be narrower)
  int n[4];       // tiles per axis
  int vec;        // sites per 16-byte access along the fastest axis (4 / 2), or 1
  int ring;       // kTiledRing when an axis is marched, else 1
  int tiles;      // per chain
  size_t lds;
};

static size_t tiled_lds(const TiledPlan &p, size_t elem) {
  size_t plane = 1, own = 1;
  for (int a = 1; a < 4; ++a) {
    plane *= size_t(p.T[a] + (p.T[a] < p.L[a] ? 2 : 0));
    own *= size_t(p.T[a]);
  }
  return kTiledScratch + (size_t(p.ring) * plane + (p.ring > 1 ? 2 : 1) * own) * elem;
}

// The one planner: nf_phi4_hmc_tiled_supported, _plan and _workspace answer from it and nf_phi4_hmc_tiled launches by it.
static int tiled_plan(const char *what, const int32_t *lattice, int dtype, TiledPlan &p) {
  NF_REQUIRE(lattice != nullptr, "%s: lattice is NULL", what);
  NF_REQUIRE(dtype == NF_F32 || dtype == NF_F64, "%s: unsupported dtype %d", what, dtype);
  const size_t elem = dtype == NF_F32 ? 4 : 8;
  int ext[4], axs[4], nd = 0;
  p.V = 1;
  for (int mu = 0; mu < 4; ++mu) {
    NF_REQUIRE(lattice[mu] >= 1, "%s: lattice extents must be >= 1", what);
    p.V *= lattice[mu];
    NF_REQUIRE(p.V < (int64_t(1) << 31), "%s: a chain of the lattice (%d, %d, %d, %d) has 2^31 sites or more", what,
               lattice[0], lattice[1], lattice[2], lattice[3]);
    if (lattice[mu] > 1) {
      ext[nd] = lattice[mu];
      axs[nd++] = mu;
    }
  }
  for (int s = 0; s < 4; ++s) {
    p.L[s] = 1;
    p.ax[s] = -1;
  }
  const int back = nd >= 3 ? nd - 1 : nd;            // the axes of a plane
  for (int i = 0; i < back; ++i) {
    p.L[4 - back + i] = ext[nd - back + i];
    p.ax[4 - back + i] = axs[nd - back + i];
  }
  if (nd >= 3) {
    p.L[0] = ext[0];
    p.ax[0] = axs[0];
  }
  p.ring = p.L[0] > 1 ? kTiledRing : 1;
  const int per = int(16 / elem);
  p.vec = p.L[3] % per == 0 ? per : 1;
  const int nseg = (p.L[0] - 1) / kTiledSegment + 1;
  p.T[0] = (p.L[0] - 1) / nseg + 1;
  for (int a = 1; a < 4; ++a) p.T[a] = p.L[a];
  // halve the longest axis of the plane tile (the fastest axis counts a quarter: rows stay long) until the tile has at
  // most 8 sites per lane and the ring fits the LDS budget
  while (int64_t(p.T[1]) * p.T[2] * p.T[3] > kTiledPlaneSites || tiled_lds(p, elem) > kTiledLdsBudget) {
    int a = 1;
    if (p.T[2] > p.T[a]) a = 2;
    if (p.T[3] > 4 * p.T[a]) a = 3;
    p.T[a] = p.T[a] / 2 + (p.T[a] & 1);
    if (a == 3) p.T[3] = (p.T[3] + p.vec - 1) / p.vec * p.vec;
  }
  p.tiles = 1;
  for (int a = 0; a < 4; ++a) {
    p.n[a] = (p.L[a] - 1) / p.T[a] + 1;
    p.tiles *= p.n[a];
  }
  p.lds = tiled_lds(p, elem);
  return NF_OK;
}

static size_t round256(size_t n) { return (n + 255) & ~size_t(255); }

struct TiledArgs {
  const void *phi_src, *pi_src;     // read (begin: the chains and pi_in, which may be NULL = draw)
  void *phi_dst, *pi_dst;           // written (begin: pi only)
  double *part;                     // (C, tiles, 4): sum pi^2 / 2 and S at the start, then at the end
  int64_t V;
  int L[4], T[4], n[4];
  int ring, tiles;
  double w0, w2, w4, dt, eps;
  PhiloxPos pos;                    // begin: the position of the momentum draw
};

// What LADDER adds to the step kernels and to commit: the rungs' coefficient table and the rung every chain holds
// (nf_phi4_hmc_tiled_ladder; the layout is nf_phi4_hmc_ladder's).
struct TiledLadderArgs : TiledArgs {
  const double *coef;   // (K, 3)
  const int32_t *rung;  // (C), clamped into 0 .. K - 1 by the kernels
  int K;
};

__device__ __forceinline__ int ladder_rung(const int32_t *rung, int64_t c, int K) { return min(max(int(rung[c]), 0), K - 1); }

// A value every lane of the workgroup holds, moved into scalar registers
__device__ __forceinline__ double tiled_uniform(double v) {
  const uint64_t b = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = __builtin_amdgcn_readfirstlane(uint32_t(b)), hi = __builtin_amdgcn_readfirstlane(uint32_t(b >> 32));
  return __builtin_bit_cast(double, uint64_t(hi) << 32 | lo);
}

template <typename T, int W>
__device__ __forceinline__ void load_w(const T *p, T (&v)[W]) {
  if constexpr (W == 1) {
    v[0] = *p;
  } else if constexpr (sizeof(T) == 4) {
    const float4 q = *reinterpret_cast<const float4 *>(p);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
    const double2 q = *reinterpret_cast<const double2 *>(p);
    v[0] = q.x; v[1] = q.y;
  }
}

template <typename T, int W>
__device__ __forceinline__ void store_w(T *p, const T (&v)[W]) {
  if constexpr (W == 1) *p = v[0];
  else if constexpr (sizeof(T) == 4) *reinterpret_cast<float4 *>(p) = float4{v[0], v[1], v[2], v[3]};
  else *reinterpret_cast<double2 *>(p) = double2{v[0], v[1]};
}

// The momenta of the W sites from flat site i of chain c, as nf_normal_sample lays them out: Philox group i / PER of the
// chain, element i % PER.  W == PER: i is a multiple of PER and the unit is one group.  W == 1: the group is drawn for its
// one site (PER times the arithmetic, in the one begin pass of a trajectory, on lattices whose rows are no multiple of PER).
template <typename T, int W>
__device__ __forceinline__ void draw_w(const TiledArgs &A, int64_t c, int64_t i, T (&v)[W]) {
  constexpr int PER = sizeof(T) == 4 ? 4 : 2;
  const int64_t ngroups = (A.V + PER - 1) / PER;
  T z[PER];
  philox_normal_group<T>(A.pos, uint64_t(c) * uint64_t(ngroups) + uint64_t(i / PER), z);
  if constexpr (W == PER) {
#pragma unroll
    for (int j = 0; j < PER; ++j) v[j] = z[j];
  } else {
    const int j = int(i % PER);
    T pick = z[0];
#pragma unroll
    for (int e = 1; e < PER; ++e) pick = j == e ? z[e] : pick;
    v[0] = pick;
  }
}

// MODE 0: begin (phi' = phi, the momenta drawn or handed in, energies of the start, phi not written);
// MODE 1: a step;  MODE 2: the last step (energies of the end).
// LADDER: the coefficients are the row rung[c] of the table, read once by the workgroup; everything else is the same code.
template <typename T, int VEC, int MODE, bool LADDER>
__global__ __launch_bounds__(kTiledLanes) void hmc_tiled_step(std::conditional_t<LADDER, TiledLadderArgs, TiledArgs> A) {
  extern __shared__ __align__(16) unsigned char tiled_lds_raw[];
  double *red = reinterpret_cast<double *>(tiled_lds_raw);
  T *ring = reinterpret_cast<T *>(tiled_lds_raw + kTiledScratch);
  const int tid = threadIdx.x;
  const int64_t c = blockIdx.y;
  const T *__restrict__ gphi = static_cast<const T *>(A.phi_src) + c * A.V;
  const T *__restrict__ gpi = A.pi_src ? static_cast<const T *>(A.pi_src) + c * A.V : nullptr;
  T *__restrict__ ophi = MODE == 0 ? nullptr : static_cast<T *>(A.phi_dst) + c * A.V;
  T *__restrict__ opi = static_cast<T *>(A.pi_dst) + c * A.V;
  double lw0 = 0.0, lw2 = 0.0, lw4 = 0.0;
  if constexpr (LADDER) {
    const double *row = A.coef + 3 * int64_t(ladder_rung(A.rung, c, A.K));
    lw0 = tiled_uniform(row[0]);
    lw2 = tiled_uniform(row[1]);
    lw4 = tiled_uniform(row[2]);
  }
  // without LADDER the three are read from the arguments where they are used, as they always were
  auto cw0 = [&]() { if constexpr (LADDER) return lw0; else return A.w0; };
  auto cw2 = [&]() { if constexpr (LADDER) return lw2; else return A.w2; };
  auto cw4 = [&]() { if constexpr (LADDER) return lw4; else return A.w4; };
  const T w0 = T(cw0()), w2x2 = T(2) * T(cw2()), w4x4 = T(4) * T(cw4()), dt = T(A.dt), eps = T(A.eps);

  // ---- the tile: origin o, extents t (the last tile of an axis may be narrower), halo h on the tiled axes of the plane
  int tl = blockIdx.x;
  const int b3 = tl % A.n[3]; tl /= A.n[3];
  const int b2 = tl % A.n[2]; tl /= A.n[2];
  const int b1 = tl % A.n[1];
  const int b0 = tl / A.n[1];
  const int L0 = A.L[0], L1 = A.L[1], L2 = A.L[2], L3 = A.L[3];
  const int T1 = A.T[1], T2 = A.T[2], T3 = A.T[3];
  const int o0 = b0 * A.T[0], o1 = b1 * T1, o2 = b2 * T2, o3 = b3 * T3;
  const int t0 = min(A.T[0], L0 - o0), t1 = min(T1, L1 - o1), t2 = min(T2, L2 - o2), t3 = min(T3, L3 - o3);
  const int h1 = A.n[1] > 1, h2 = A.n[2] > 1, h3 = A.n[3] > 1;
  const int E2 = T2 + 2 * h2, E3 = T3 + 2 * h3;
  const int st1 = E2 * E3, st2 = E3;                        // LDS strides of the plane's axes (the fastest: 1)
  const int PS = (T1 + 2 * h1) * st1;                       // sites of a plane in the ring
  const int own_sites = T1 * T2 * T3;
  T *pibuf = ring + A.ring * PS;                            // lane-private: entry (k 256 + tid) VEC + v of plane p & 1
  const int s2 = L3, s1 = L3 * L2, s0 = L3 * L2 * L1;       // global strides
  const bool march = L0 > 1;
  const int rmask = A.ring - 1;

  // ---- the lane's units of a plane: the same in every plane, so the coordinates are worked out once.
  // u_l: LDS index in a plane, u_g: global offset in a plane, u_f: bit 0 valid, bits 1 .. 4 the wraps of the untiled axes
  // (y1 == 0, y1 == t1 - 1, y2 == 0, y2 == t2 - 1), bits 8 ..: y3 of the unit's first site
  const int U3 = T3 / VEC, NU = T1 * T2 * U3;
  int u_l[kTiledUnits], u_g[kTiledUnits];
  uint32_t u_f[kTiledUnits];
#pragma unroll
  for (int k = 0; k < kTiledUnits; ++k) {
    const int j = tid + k * kTiledLanes;
    const int jj = j < NU ? j : 0;
    int y3 = (jj % U3) * VEC;
    const int r = jj / U3;
    int y2 = r % T2, y1 = r / T2;
    const bool valid = j < NU && y1 < t1 && y2 < t2 && y3 < t3;
    if (!valid) y1 = y2 = y3 = 0;
    u_l[k] = (y1 + h1) * st1 + (y2 + h2) * st2 + y3 + h3;
    u_g[k] = (o1 + y1) * s1 + (o2 + y2) * s2 + o3 + y3;
    u_f[k] = uint32_t(valid) | uint32_t(y1 == 0) << 1 | uint32_t(y1 == t1 - 1) << 2 | uint32_t(y2 == 0) << 3 |
             uint32_t(y2 == t2 - 1) << 4 | uint32_t(y3) << 8;
  }

  // ---- the halo of a plane: the two faces of every tiled axis, units along the fastest axis (faces of axes 1 and 2) or
  // single sites (faces of axis 3)
  const int u3 = t3 / VEC;
  const int f1 = h1 ? t2 * u3 : 0, f2 = h2 ? t1 * u3 : 0, f3 = h3 ? t1 * t2 : 0;
  const int NH = 2 * (f1 + f2 + f3);

  auto load_plane = [&](int p, bool own) {
    int x0 = o0 + p;
    x0 += x0 < 0 ? L0 : 0;
    x0 -= x0 >= L0 ? L0 : 0;
    T *dst = ring + ((p + 1) & rmask) * PS;
    const int g0 = x0 * s0;
#pragma unroll
    for (int k = 0; k < kTiledUnits; ++k) {
      if (k * kTiledLanes < NU && (u_f[k] & 1u)) {
        const int g = g0 + u_g[k];
        T f[VEC], q[VEC];
        load_w<T, VEC>(gphi + g, f);
        if constexpr (MODE == 0) {
          if (own) {
            if (gpi) load_w<T, VEC>(gpi + g, q);
            else draw_w<T, VEC>(A, c, g, q);
          }
        } else {
          load_w<T, VEC>(gpi + g, q);
#pragma unroll
          for (int v = 0; v < VEC; ++v) f[v] += dt * q[v];
        }
        T *pb = pibuf + (p & 1) * own_sites + (k * kTiledLanes + tid) * VEC;
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          dst[u_l[k] + v] = f[v];
          if (own) pb[v] = q[v];
        }
      }
    }
    if (!own) return;                                      // the planes before and behind the segment: no halo needed
    for (int j = tid; j < NH; j += kTiledLanes) {
      int y1, y2, y3, jj = j;
      bool wide = true;
      if (jj < 2 * f1) {
        const int side = jj >= f1;
        jj -= side * f1;
        y1 = side ? t1 : -1; y2 = jj / u3; y3 = (jj % u3) * VEC;
      } else if ((jj -= 2 * f1) < 2 * f2) {
        const int side = jj >= f2;
        jj -= side * f2;
        y2 = side ? t2 : -1; y1 = jj / u3; y3 = (jj % u3) * VEC;
      } else {
        jj -= 2 * f2;
        const int side = jj >= f3;
        jj -= side * f3;
        y3 = side ? t3 : -1; y1 = jj / t2; y2 = jj % t2;
        wide = false;
      }
      int x1 = o1 + y1, x2 = o2 + y2, x3 = o3 + y3;
      x1 += x1 < 0 ? L1 : 0; x1 -= x1 >= L1 ? L1 : 0;
      x2 += x2 < 0 ? L2 : 0; x2 -= x2 >= L2 ? L2 : 0;
      x3 += x3 < 0 ? L3 : 0; x3 -= x3 >= L3 ? L3 : 0;
      const int g = g0 + x1 * s1 + x2 * s2 + x3;
      T *d = dst + (y1 + h1) * st1 + (y2 + h2) * st2 + y3 + h3;
      if (VEC > 1 && wide) {
        T f[VEC], q[VEC];
        load_w<T, VEC>(gphi + g, f);
        if constexpr (MODE != 0) {
          load_w<T, VEC>(gpi + g, q);
#pragma unroll
          for (int v = 0; v < VEC; ++v) f[v] += dt * q[v];
        }
#pragma unroll
        for (int v = 0; v < VEC; ++v) d[v] = f[v];
      } else {
        T f = gphi[g];
        if constexpr (MODE != 0) f += dt * gpi[g];
        d[0] = f;
      }
    }
  };

  double kin = 0.0, pot = 0.0;
  auto update_plane = [&](int q) {
    const T *cur = ring + ((q + 1) & rmask) * PS;
    const T *below = ring + (q & rmask) * PS, *above = ring + ((q + 2) & rmask) * PS;
    const int g0 = (o0 + q) * s0;
#pragma unroll
    for (int k = 0; k < kTiledUnits; ++k) {
      if (k * kTiledLanes < NU && (u_f[k] & 1u)) {
        const uint32_t fl = u_f[k];
        const int i0 = u_l[k], y30 = int(fl >> 8);
        // the neighbours on the plane's slow axes: through the halo where the axis is tiled, else wrapped inside the tile
        const int b1i = (!h1 && (fl & 2u)) ? (t1 - 1) * st1 : -st1, f1i = (!h1 && (fl & 4u)) ? -(t1 - 1) * st1 : st1;
        const int b2i = (!h2 && (fl & 8u)) ? (t2 - 1) * st2 : -st2, f2i = (!h2 && (fl & 16u)) ? -(t2 - 1) * st2 : st2;
        const T *pb = pibuf + (q & 1) * own_sites + (k * kTiledLanes + tid) * VEC;
        T fo[VEC], po[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          const int i = i0 + v, y3 = y30 + v;
          const T ph = cur[i];
          T nb = T(0);
          double nbk = 0.0;
          if (march) {
            const T b = below[i];
            nb += b + above[i];
            nbk += double(b);
          }
          if (L1 > 1) {
            const T b = cur[i + b1i];
            nb += b + cur[i + f1i];
            nbk += double(b);
          }
          if (L2 > 1) {
            const T b = cur[i + b2i];
            nb += b + cur[i + f2i];
            nbk += double(b);
          }
          if (L3 > 1) {
            const T b = cur[i + ((!h3 && y3 == 0) ? t3 - 1 : -1)];
            nb += b + cur[i + ((!h3 && y3 == t3 - 1) ? -(t3 - 1) : 1)];
            nbk += double(b);
          }
          const T pi0 = pb[v];
          const T pi1 = pi0 - eps * phi4_force(ph, nb, w2x2, w4x4, w0);
          fo[v] = ph;
          po[v] = pi1;
          if constexpr (MODE != 1) {
            const double qd = double(MODE == 0 ? pi0 : pi1);
            kin += 0.5 * qd * qd;
            pot += phi4_site_energy(double(ph), nbk, cw0(), cw2(), cw4());
          }
        }
        const int g = g0 + u_g[k];
        if constexpr (MODE != 0) store_w<T, VEC>(ophi + g, fo);
        store_w<T, VEC>(opi + g, po);
      }
    }
  };

  if (march) {
    for (int p = -1; p <= t0; ++p) {
      load_plane(p, p >= 0 && p < t0);
      __syncthreads();
      if (p >= 1) update_plane(p - 1);
    }
  } else {
    load_plane(0, true);
    __syncthreads();
    update_plane(0);
  }

  if constexpr (MODE != 1) {
    kin = wave_sum(kin);
    pot = wave_sum(pot);
    const int lane = tid & (kWave - 1), w = tid / kWave;
    if (lane == 0) {
      red[2 * w] = kin;
      red[2 * w + 1] = pot;
    }
    __syncthreads();
    if (tid == 0) {
      double a = 0.0, b = 0.0;
      for (int i = 0; i < kTiledLanes / kWave; ++i) {
        a += red[2 * i];
        b += red[2 * i + 1];
      }
      double *out = A.part + (c * A.tiles + blockIdx.x) * 4 + (MODE == 0 ? 0 : 2);
      out[0] = a;
      out[1] = b;
    }
  }
}

struct CommitArgs {
  void *phi;                 // the chains
  const void *prop, *pi_fin; // the proposal and its momenta
  void *record, *pi_out;     // this trajectory's record row and pi_out, or NULL
  const double *part;
  double *dh_out, *action_out;   // this trajectory's row of dh_out
  uint8_t *accept_out;
  int64_t V;
  int tiles, force;
  PhiloxPos pos;
};

struct CommitLadderArgs : CommitArgs {
  const int32_t *rung;
  int K;
};

// One chain per blockIdx.y, a slice of its sites per blockIdx.x.  Every workgroup of a chain adds the same partials in
// the same order and takes the same decision; the first one writes it out.
// LADDER: dh_out, accept_out and the record row go to the chain's rung-ordered column, (c / K) K + rung[c].
template <typename T, bool LADDER>
__global__ __launch_bounds__(kTiledLanes) void hmc_tiled_commit(std::conditional_t<LADDER, CommitLadderArgs, CommitArgs> A) {
  __shared__ double sums[4];
  const int tid = threadIdx.x;
  const int64_t c = blockIdx.y;
  int64_t oc = c;
  if constexpr (LADDER) oc = c / A.K * A.K + ladder_rung(A.rung, c, A.K);
  if (tid < 4) {
    const double *p = A.part + c * A.tiles * 4 + tid;
    double acc = 0.0;
    for (int i = 0; i < A.tiles; ++i) acc += p[4 * i];
    sums[tid] = acc;
  }
  __syncthreads();
  const double k0 = sums[0], e0 = sums[1], k1 = sums[2], e1 = sums[3];
  const double dh = (k1 + e1) - (k0 + e0);
  const bool ok = hmc_accepts(philox_log_uniform(A.pos, uint64_t(c)), dh, A.force);
  if (blockIdx.x == 0 && tid == 0) {
    A.dh_out[oc] = dh;
    A.accept_out[oc] = uint8_t(ok);
    A.action_out[c] = ok ? e1 : e0;
  }
  T *__restrict__ phi = static_cast<T *>(A.phi) + c * A.V;
  const T *__restrict__ prop = static_cast<const T *>(A.prop) + c * A.V;
  const T *__restrict__ pif = static_cast<const T *>(A.pi_fin) + c * A.V;
  T *rec = A.record ? static_cast<T *>(A.record) + oc * A.V : nullptr;
  T *pout = A.pi_out ? static_cast<T *>(A.pi_out) + c * A.V : nullptr;
  if (!ok && !rec && !pout) return;
  for (int64_t i = int64_t(blockIdx.x) * kTiledLanes + tid; i < A.V; i += int64_t(gridDim.x) * kTiledLanes) {
    if (ok) {
      const T v = prop[i];
      phi[i] = v;
      if (rec) rec[i] = v;
    } else if (rec) {
      rec[i] = phi[i];
    }
    if (pout) pout[i] = pif[i];
  }
}

template <typename Args> constexpr bool kTiledLadder = std::is_same_v<Args, TiledLadderArgs>;
template <typename Args> constexpr const char *kTiledName = kTiledLadder<Args> ? "nf_phi4_hmc_tiled_ladder" : "nf_phi4_hmc_tiled";

template <typename T, int VEC, typename Args>
static int launch_tiled_step(int mode, const Args &A, const TiledPlan &p, int64_t C, hipStream_t s) {
  const dim3 grid(unsigned(p.tiles), unsigned(C)), block(kTiledLanes);
  auto k0 = hmc_tiled_step<T, VEC, 0, kTiledLadder<Args>>;
  auto k1 = hmc_tiled_step<T, VEC, 1, kTiledLadder<Args>>;
  auto k2 = hmc_tiled_step<T, VEC, 2, kTiledLadder<Args>>;
  auto kern = mode == 0 ? k0 : mode == 1 ? k1 : k2;
  hipLaunchKernelGGL(kern, grid, block, p.lds, s, A);
  return check_launch(kTiledName<Args>);
}

template <typename T, int VEC, bool LADDER>
static int raise_lds(const TiledPlan &p) {
  if (p.lds <= 64 * 1024) return NF_OK;
  const void *kerns[3] = {reinterpret_cast<const void *>(hmc_tiled_step<T, VEC, 0, LADDER>),
                          reinterpret_cast<const void *>(hmc_tiled_step<T, VEC, 1, LADDER>),
                          reinterpret_cast<const void *>(hmc_tiled_step<T, VEC, 2, LADDER>)};
  for (const void *k : kerns)
    if (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, int(p.lds)) != hipSuccess) {
      (void)hipGetLastError();
      set_error("%s: cannot raise the dynamic LDS limit to %zu B", LADDER ? "nf_phi4_hmc_tiled_ladder" : "nf_phi4_hmc_tiled",
                p.lds);
      return NF_ELAUNCH;
    }
  return NF_OK;
}

template <typename T, int VEC, typename Args>
static int run_tiled(const HmcCall &K, const HmcSteps &st, unsigned char *ws, Args A, const TiledPlan &p, hipStream_t s) {
  constexpr bool LADDER = kTiledLadder<Args>;
  int rc = raise_lds<T, VEC, LADDER>(p);
  if (rc) return rc;
  const size_t field = round256(size_t(K.C) * size_t(p.V) * sizeof(T));
  double *part = reinterpret_cast<double *>(ws);
  unsigned char *base = ws + round256(size_t(K.C) * size_t(p.tiles) * 4 * sizeof(double));
  void *fphi[2] = {base, base + field}, *fpi[2] = {base + 2 * field, base + 3 * field};
  A.part = part;
  const int evals = K.n_md * st.stages;                // step launches of a trajectory: one per force evaluation
  const int64_t per_chain = (p.V + kTiledLanes * 8 - 1) / (kTiledLanes * 8);
  const unsigned cblocks = unsigned(per_chain < 1024 ? per_chain : 1024);
  for (int t = 0; t < K.n_traj; ++t) {
    A.pos = philox_pos(K.seed, NF_PHILOX_KEY_DOMAIN, K.offset + 2 * uint64_t(t));
    A.phi_src = K.phi; A.pi_src = K.pi_in; A.phi_dst = nullptr; A.pi_dst = fpi[0];
    A.dt = 0.0;                                        // begin moves no site
    A.eps = st.kick_half;
    if ((rc = launch_tiled_step<T, VEC>(0, A, p, K.C, s))) return rc;
    const void *src = K.phi;
    // launch k of the n_md s: stage (k - 1) % s of the scheme, the buffers alternating with k, the last launch with
    // the half kick and the energies of the end
    for (int k = 1, j = 0; k <= evals; ++k, j = j + 1 == st.stages ? 0 : j + 1) {
      A.phi_src = src; A.pi_src = fpi[(k - 1) & 1]; A.phi_dst = fphi[(k - 1) & 1]; A.pi_dst = fpi[k & 1];
      A.dt = st.drift[j];
      A.eps = k == evals ? st.kick_half : st.kick[j];
      if ((rc = launch_tiled_step<T, VEC>(k == evals ? 2 : 1, A, p, K.C, s))) return rc;
      src = A.phi_dst;
    }
    std::conditional_t<LADDER, CommitLadderArgs, CommitArgs> Q{};
    Q.phi = K.phi; Q.prop = src; Q.pi_fin = fpi[evals & 1];
    const bool due = K.record && (t + 1) % K.record_every == 0;
    Q.record = due ? static_cast<T *>(K.record) + int64_t((t + 1) / K.record_every - 1) * K.C * p.V : nullptr;
    Q.pi_out = t + 1 == K.n_traj ? K.pi_out : nullptr;
    Q.part = part;
    Q.dh_out = K.dh_out + int64_t(t) * K.C;
    Q.accept_out = K.accept_out + int64_t(t) * K.C;
    Q.action_out = K.action_out;
    Q.V = p.V; Q.tiles = p.tiles; Q.force = K.force;
    Q.pos = philox_pos(K.seed, NF_PHILOX_ACCEPT_DOMAIN, K.offset + 2 * uint64_t(t) + 1);
    if constexpr (LADDER) {
      Q.rung = A.rung;
      Q.K = A.K;
    }
    hipLaunchKernelGGL((hmc_tiled_commit<T, LADDER>), dim3(cblocks, unsigned(K.C)), dim3(kTiledLanes), 0, s, Q);
    if ((rc = check_launch(LADDER ? "nf_phi4_hmc_tiled_ladder (commit)" : "nf_phi4_hmc_tiled (commit)"))) return rc;
  }
  return NF_OK;
}

static size_t tiled_workspace(int64_t C, const TiledPlan &p, size_t elem) {
  return round256(size_t(C) * size_t(p.tiles) * 4 * sizeof(double)) + 4 * round256(size_t(C) * size_t(p.V) * elem);
}

}  // namespace nf

using namespace nf;

extern "C" int nf_phi4_hmc_tiled_supported(const int32_t *lattice, int dtype) {
  TiledPlan p;
  return tiled_plan("nf_phi4_hmc_tiled_supported", lattice, dtype, p) == NF_OK ? 1 : 0;
}

extern "C" int nf_phi4_hmc_tiled_plan(const int32_t *lattice, int dtype, nf_hmc_tiled_plan *out) {
  NF_REQUIRE(out != nullptr, "nf_phi4_hmc_tiled_plan: out is NULL");
  TiledPlan p;
  const int rc = tiled_plan("nf_phi4_hmc_tiled_plan", lattice, dtype, p);
  if (rc) return rc;
  for (int mu = 0; mu < 4; ++mu) {
    out->tile[mu] = 1;
    out->ntiles[mu] = 1;
  }
  for (int s = 0; s < 4; ++s)
    if (p.ax[s] >= 0) {
      out->tile[p.ax[s]] = p.T[s];
      out->ntiles[p.ax[s]] = p.n[s];
    }
  out->tiles = p.tiles;
  out->march_axis = p.L[0] > 1 ? p.ax[0] : -1;
  out->ring_depth = p.L[0] > 1 ? p.ring : 0;
  out->lanes = kTiledLanes;
  out->vec = p.vec;
  out->lds_bytes = int64_t(p.lds);
  out->lds_budget = int64_t(kTiledLdsBudget);
  return NF_OK;
}

extern "C" size_t nf_phi4_hmc_tiled_workspace(int64_t C, const int32_t *lattice, int dtype) {
  TiledPlan p;
  if (C < 1 || tiled_plan("nf_phi4_hmc_tiled_workspace", lattice, dtype, p) != NF_OK) return 0;
  return tiled_workspace(C, p, dtype == NF_F32 ? 4 : 8);
}

// The body of nf_phi4_hmc_tiled (coef NULL: the three scalars) and of nf_phi4_hmc_tiled_ladder.
static int tiled_entry(const char *what, bool ladder, void *phi, double *action_out, const void *pi_in, void *pi_out,
                       double *dh_out, uint8_t *accept_out, void *record, int record_every, int64_t C, const int32_t *lattice,
                       double w0, double w2, double w4, const double *coef, int Kr, const int32_t *rung, int n_md, double dt,
                       int n_traj, int force_accept, uint64_t seed, uint64_t offset, void *workspace, size_t workspace_bytes,
                       int dtype, void *stream, const nf_hmc_scheme *scheme) {
  HmcSteps st;
  int rc = hmc_steps(what, scheme, dt, st);              // the scheme first: a bad one is refused before anything else
  if (rc) return rc;
  const HmcCall K{phi, action_out, pi_in, pi_out, dh_out, accept_out, record, record_every, C, n_md, n_traj,
                  force_accept != 0, seed, offset};
  TiledPlan p;
  rc = hmc_call_checks(what, K);
  if (!rc && ladder) rc = hmc_ladder_checks(what, coef, Kr, rung, C);
  if (!rc) rc = tiled_plan(what, lattice, dtype, p);
  if (rc) return rc;
  NF_REQUIRE(int64_t(p.tiles) * C <= kTiledMaxGroups,
             "%s: %d tiles x %lld chains exceed the %lld workgroups of one launch: run the chains in several "
             "calls", what, p.tiles, (long long)C, (long long)kTiledMaxGroups);
  const int64_t launches = (int64_t(n_md) * st.stages + 2) * int64_t(n_traj);
  NF_REQUIRE(launches <= NF_HMC_TILED_MAX_LAUNCHES,
             "%s: (n_md s + 2) n_traj = %lld launches (s = %d stages) exceed NF_HMC_TILED_MAX_LAUNCHES (%d): split the run "
             "into several calls", what, (long long)launches, st.stages, NF_HMC_TILED_MAX_LAUNCHES);
  const size_t elem = dtype == NF_F32 ? 4 : 8;
  const size_t need = tiled_workspace(C, p, elem);
  NF_REQUIRE(workspace != nullptr && workspace_bytes >= need, "%s: workspace %zu B < %zu B needed", what,
             workspace ? workspace_bytes : size_t(0), need);
  TiledLadderArgs A{};
  A.V = p.V;
  for (int a = 0; a < 4; ++a) {
    A.L[a] = p.L[a];
    A.T[a] = p.T[a];
    A.n[a] = p.n[a];
  }
  A.ring = p.ring; A.tiles = p.tiles;
  A.w0 = w0; A.w2 = w2; A.w4 = w4;
  A.coef = coef; A.rung = rung; A.K = Kr;
  // 16-byte accesses need every row to start on 16 bytes: the lattice's fastest extent a multiple of 16 / sizeof (the
  // plan's vec) and the caller's fields aligned; the workspace's fields are, when the workspace is
  const uintptr_t bits = reinterpret_cast<uintptr_t>(phi) | reinterpret_cast<uintptr_t>(pi_in) |
                         reinterpret_cast<uintptr_t>(workspace);
  const bool wide = p.vec > 1 && (bits & 15) == 0;
  NF_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "%s: the workspace must be 8-byte aligned", what);
  hipStream_t s = static_cast<hipStream_t>(stream);
  unsigned char *ws = static_cast<unsigned char *>(workspace);
  if (ladder) {
    if (dtype == NF_F32) return wide ? run_tiled<float, 4>(K, st, ws, A, p, s) : run_tiled<float, 1>(K, st, ws, A, p, s);
    return wide ? run_tiled<double, 2>(K, st, ws, A, p, s) : run_tiled<double, 1>(K, st, ws, A, p, s);
  }
  const TiledArgs &B = A;
  if (dtype == NF_F32) return wide ? run_tiled<float, 4>(K, st, ws, B, p, s) : run_tiled<float, 1>(K, st, ws, B, p, s);
  return wide ? run_tiled<double, 2>(K, st, ws, B, p, s) : run_tiled<double, 1>(K, st, ws, B, p, s);
}

extern "C" int nf_phi4_hmc_tiled(void *phi, double *action_out, const void *pi_in, void *pi_out, double *dh_out,
                                 uint8_t *accept_out, void *record, int record_every, int64_t C, const int32_t *lattice,
                                 double w0, double w2, double w4, int n_md, double dt, int n_traj, int force_accept,
                                 uint64_t seed, uint64_t offset, void *workspace, size_t workspace_bytes, int dtype,
                                 void *stream) {
  return tiled_entry("nf_phi4_hmc_tiled", false, phi, action_out, pi_in, pi_out, dh_out, accept_out, record, record_every, C,
                     lattice, w0, w2, w4, nullptr, 0, nullptr, n_md, dt, n_traj, force_accept, seed, offset, workspace,
                     workspace_bytes, dtype, stream, nullptr);
}

extern "C" int nf_phi4_hmc_tiled_ladder(void *phi, double *action_out, const void *pi_in, void *pi_out, double *dh_out,
                                        uint8_t *accept_out, void *record, int record_every, int64_t C,
                                        const int32_t *lattice, const double *coef, int K, const int32_t *rung, int n_md,
                                        double dt, int n_traj, int force_accept, uint64_t seed, uint64_t offset,
                                        void *workspace, size_t workspace_bytes, int dtype, void *stream) {
  return tiled_entry("nf_phi4_hmc_tiled_ladder", true, phi, action_out, pi_in, pi_out, dh_out, accept_out, record,
                     record_every, C, lattice, 0.0, 0.0, 0.0, coef, K, rung, n_md, dt, n_traj, force_accept, seed, offset,
                     workspace, workspace_bytes, dtype, stream, nullptr);
}

// The same launchers with an integration scheme (NULL: leapfrog, the launchers above).
extern "C" int nf_phi4_hmc_tiled_scheme(void *phi, double *action_out, const void *pi_in, void *pi_out, double *dh_out,
                                 uint8_t *accept_out, void *record, int record_every, int64_t C, const int32_t *lattice,
                                 double w0, double w2, double w4, int n_md, double dt, int n_traj, int force_accept,
                                 uint64_t seed, uint64_t offset, void *workspace, size_t workspace_bytes, int dtype,
                                 void *stream, const nf_hmc_scheme *scheme) {
  return tiled_entry("nf_phi4_hmc_tiled_scheme", false, phi, action_out, pi_in, pi_out, dh_out, accept_out, record, record_every, C,
                     lattice, w0, w2, w4, nullptr, 0, nullptr, n_md, dt, n_traj, force_accept, seed, offset, workspace,
                     workspace_bytes, dtype, stream, scheme);
}

extern "C" int nf_phi4_hmc_tiled_ladder_scheme(void *phi, double *action_out, const void *pi_in, void *pi_out, double *dh_out,
                                        uint8_t *accept_out, void *record, int record_every, int64_t C,
                                        const int32_t *lattice, const double *coef, int K, const int32_t *rung, int n_md,
                                        double dt, int n_traj, int force_accept, uint64_t seed, uint64_t offset,
                                        void *workspace, size_t workspace_bytes, int dtype, void *stream, const nf_hmc_scheme *scheme) {
  return tiled_entry("nf_phi4_hmc_tiled_ladder_scheme", true, phi, action_out, pi_in, pi_out, dh_out, accept_out, record,
                     record_every, C, lattice, 0.0, 0.0, 0.0, coef, K, rung, n_md, dt, n_traj, force_accept, seed, offset,
                     workspace, workspace_bytes, dtype, stream, scheme);
}

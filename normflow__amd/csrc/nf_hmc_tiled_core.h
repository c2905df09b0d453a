// nf_hmc_tiled_core.h -- the planner and the kernels of the tiled phi^4 HMC, what nf_hmc_tiled.hip (nf_phi4_hmc_tiled and its
// ladder and scheme forms) and nf_hmc_fa_tiled.hip (the Fourier-accelerated nf_phi4_hmc_fa_tiled) share, stated ONCE: the
// tile plan, the marched drift-and-kick step with its ring of four planes, halo rule and wide accesses, and commit.  The
// layout of a trajectory and of the tiles is described at the head of nf_hmc_tiled.hip.
// VEL (the accelerated trajectory, include/normflow_hip.h "Fourier-accelerated hybrid Monte Carlo"): the step takes the
// velocity v = A pi as a separate operand, phi' = phi + dt v and pi' = pi - eps F(phi'), and its energy forms take the
// kinetic term from pi and v, sum pi v / 2; without VEL every instantiation is the code it always was.
#pragma once
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

// nf_hmc_tiled_plan from the planner's answer, per axis of the caller's lattice
static void tiled_plan_out(const TiledPlan &p, nf_hmc_tiled_plan *out) {
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
  out->reserved = 0;
  out->lds_bytes = int64_t(p.lds);
  out->lds_budget = int64_t(kTiledLdsBudget);
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

// What VEL adds: the velocity A pi of the chains, (C, V) like the other fields.
struct TiledVelArgs : TiledArgs {
  const void *vel_src;
};

template <bool LADDER, bool VEL>
using TiledStepArgs = std::conditional_t<LADDER, TiledLadderArgs, std::conditional_t<VEL, TiledVelArgs, TiledArgs>>;

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
// MODE 1: a step;  MODE 2: the last step (energies of the end);
// MODE 3 (VEL only): the energies of the end alone -- phi' = phi, nothing but the partials is written.
// LADDER: the coefficients are the row rung[c] of the table, read once by the workgroup; everything else is the same code.
// VEL: the drift reads the velocity from its own buffer (the momenta are always handed in: the draw and its refresh are
// launches of their own), and the kinetic partial of MODE 0 / 3 is sum pi v / 2, added where the plane is loaded.
template <typename T, int VEC, int MODE, bool LADDER, bool VEL = false>
__global__ __launch_bounds__(kTiledLanes) void hmc_tiled_step(TiledStepArgs<LADDER, VEL> A) {
  static_assert(!(LADDER && VEL), "there is no accelerated ladder");
  static_assert(VEL ? MODE != 2 : MODE != 3, "MODE 2 is the plain kernels', MODE 3 the accelerated one's");
  constexpr bool STILL = MODE == 0 || MODE == 3;              // phi' = phi
  extern __shared__ __align__(16) unsigned char tiled_lds_raw[];
  double *red = reinterpret_cast<double *>(tiled_lds_raw);
  T *ring = reinterpret_cast<T *>(tiled_lds_raw + kTiledScratch);
  const int tid = threadIdx.x;
  const int64_t c = blockIdx.y;
  const T *__restrict__ gphi = static_cast<const T *>(A.phi_src) + c * A.V;
  const T *__restrict__ gpi = A.pi_src ? static_cast<const T *>(A.pi_src) + c * A.V : nullptr;
  const T *__restrict__ gvel = nullptr;
  if constexpr (VEL) gvel = static_cast<const T *>(A.vel_src) + c * A.V;
  T *__restrict__ ophi = STILL ? nullptr : static_cast<T *>(A.phi_dst) + c * A.V;
  T *__restrict__ opi = MODE == 3 ? nullptr : static_cast<T *>(A.pi_dst) + c * A.V;
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

  double kin = 0.0, pot = 0.0;
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
        if constexpr (VEL) {
          // the velocity moves phi (every plane loaded); the momenta wait for the force (the tile's own planes)
          if constexpr (STILL) {
            if (own) {
              T vq[VEC];
              load_w<T, VEC>(gpi + g, q);
              load_w<T, VEC>(gvel + g, vq);
#pragma unroll
              for (int v = 0; v < VEC; ++v) kin += 0.5 * double(q[v]) * double(vq[v]);
            }
          } else {
            T vq[VEC];
            load_w<T, VEC>(gvel + g, vq);
#pragma unroll
            for (int v = 0; v < VEC; ++v) f[v] += dt * vq[v];
            if (own) load_w<T, VEC>(gpi + g, q);
          }
        } else if constexpr (MODE == 0) {
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
    const T *__restrict__ gmove = VEL ? gvel : gpi;        // what the drift adds
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
        if constexpr (!STILL) {
          load_w<T, VEC>(gmove + g, q);
#pragma unroll
          for (int v = 0; v < VEC; ++v) f[v] += dt * q[v];
        }
#pragma unroll
        for (int v = 0; v < VEC; ++v) d[v] = f[v];
      } else {
        T f = gphi[g];
        if constexpr (!STILL) f += dt * gmove[g];
        d[0] = f;
      }
    }
  };

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
          if constexpr (MODE != 3) {
            const T pi0 = pb[v];
            const T pi1 = pi0 - eps * phi4_force(ph, nb, w2x2, w4x4, w0);
            fo[v] = ph;
            po[v] = pi1;
            if constexpr (MODE != 1 && !VEL) {
              const double qd = double(MODE == 0 ? pi0 : pi1);
              kin += 0.5 * qd * qd;
            }
          }
          if constexpr (MODE != 1) pot += phi4_site_energy(double(ph), nbk, cw0(), cw2(), cw4());
        }
        const int g = g0 + u_g[k];
        if constexpr (!STILL) store_w<T, VEC>(ophi + g, fo);
        if constexpr (MODE != 3) store_w<T, VEC>(opi + g, po);
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

// The workgroups of a commit launch per chain
static unsigned tiled_commit_blocks(int64_t V) {
  const int64_t per_chain = (V + kTiledLanes * 8 - 1) / (kTiledLanes * 8);
  return unsigned(per_chain < 1024 ? per_chain : 1024);
}

}  // namespace nf

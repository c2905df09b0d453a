// nf_hmc.hip -- hybrid Monte Carlo for the lattice phi^4 action with the chain resident in a CU (MI355X-side extension, no
// counterpart in the reference; the action is src/action/scalar_action.py:24-46).  For C independent chains:
//   F(phi)(x) = 2 w2 phi(x) + 4 w4 phi(x)^3 - w0 sum_mu [phi(x + mu) + phi(x - mu)]                     (periodic)
//   pi ~ N(0, 1)^V;  H0 = sum pi^2 / 2 + S(phi);  leapfrog of n_md steps of length dt (half kicks at both ends);
//   H1 likewise;  accept iff log u < -(H1 - H0).
// One workgroup per chain runs ALL n_traj trajectories of its chain in one launch.  Lane `tid` of the NT lanes owns the
// sites tid + k NT (k < NS) and keeps their phi and pi in registers; one image of phi lives in LDS for the neighbour reads
// (lanes of a wave read consecutive addresses along every axis: no bank conflicts away from the wrap).  An MD step is
// "phi += dt pi | barrier | image <- phi | barrier | pi -= dt F(image)": two barriers.  The chain's phi in HBM is written
// only when a trajectory is accepted and read back when one is rejected, so a rejected chain keeps its bits.
// The energies are summed in double whatever the field dtype, in a fixed order (lane partial over k, wave shuffle tree,
// waves in order): no atomics, the same inputs give the same bits, and a launch of n_traj trajectories equals n_traj
// launches of one.  Random numbers: the streams of nf_normal_sample (momenta) and nf_block_accept (uniform), see the header;
// the two draws, the accept rule and the site terms of F and S are nf_sampler_core.h's, shared with nf_hmc_tiled.hip.
// nf_phi4_hmc_measure is the same kernel compiled with MEASURE: after the decision of every record_every-th trajectory the
// image is refilled with the chain's state and measure_image (nf_measure_core.h) takes nf_lattice_measure's row from it,
// by that kernel's team for the lattice on the first lanes of the workgroup, so the row has nf_lattice_measure's bits.
// nf_phi4_hmc_ladder is the same kernel compiled with LADDER (with or without MEASURE): the workgroup of chain c takes its
// three coefficients from row rung[c] of a table instead of from the arguments, once, into scalar registers, and writes
// its time series (dH, accept flag, record row, measure row) at the rung-ordered column (c / K) K + rung[c]; its state, its
// momenta and its Philox draws stay at c.  From there on it is the code above: a chain on rung k has nf_phi4_hmc's bits
// at rung k's coefficients.  The exchange sweep that permutes `rung` between launches is nf_ladder.hip.
// Integration schemes (the _scheme entry points; include/normflow_hip.h): the MD loop runs n_md s stages "phi += a_j dt pi
// | barrier | image <- phi | barrier | pi -= b_j dt F(image)" with the lengths a_j dt, b_j dt and (b_s / 2) dt formed on the
// host (HmcSteps, nf_sampler_core.h) and carried in the by-value arguments; leapfrog is s = 1 through the same loop, and
// its lengths dt and dt / 2 are the bits they always were.
#include <type_traits>

#include "nf_measure_core.h"
#include "nf_sampler_core.h"

namespace nf {

constexpr int kHmcMaxLanes = 1024;
constexpr size_t kHmcFieldBytes = 64 * 1024;       // the LDS image of one chain: V sizeof(T) <= 64 KiB
constexpr size_t kHmcScratchBytes = 1024;          // reduction slots and the broadcast of the decision, in front of the image
// MEASURE: measure_image's slots between the two -- 8 doubles per wave of the WORKGROUP (a wave outside the team writes its
// empty sums to its own slot, so the slots are sized for the 16 waves of kHmcMaxLanes, not for the team's) and one stripe
// partial per lane of the widest team
constexpr size_t kHmcMsRed = kHmcMaxLanes / kWave * 8;
constexpr size_t kHmcMsScratchBytes = (kHmcMsRed + kMsMaxLanes) * sizeof(double);
constexpr int kHmcIdleLane = 1 << 30;              // the team lane of a wave outside the team: beyond every loop bound of measure_image

struct HmcPlan {
  int64_t V;
  int L[4];      // the extents above 1, in order, behind leading 1s: dropping an axis of extent 1 moves no site
  int nd;        // how many there are (1 .. 4; a lattice of one site counts as one axis of extent 1)
  int ns;        // sites per lane (1, 2, 4, 8, 16): the smallest power of two with ceil(V / ns) <= 1024
  int nt;        // lanes per chain: ceil(V / ns) rounded up to whole waves
  size_t lds;    // dynamic LDS of the launch (MEASURE: + kHmcMsScratchBytes)
};

// The one planner: nf_phi4_hmc_supported answers from it and nf_phi4_hmc launches by it.
static int hmc_plan(const char *what, const int32_t *lattice, int dtype, HmcPlan &p) {
  NF_REQUIRE(lattice != nullptr, "%s: lattice is NULL", what);
  NF_REQUIRE(dtype == NF_F32 || dtype == NF_F64, "%s: unsupported dtype %d", what, dtype);
  const size_t elem = dtype == NF_F32 ? 4 : 8;
  p.V = 1;
  p.nd = 0;
  for (int mu = 0; mu < 4; ++mu) p.L[mu] = 1;
  for (int mu = 0; mu < 4; ++mu) {
    NF_REQUIRE(lattice[mu] >= 1, "%s: lattice extents must be >= 1", what);
    if (lattice[mu] > 1) {
      for (int nu = 0; nu < 3; ++nu) p.L[nu] = p.L[nu + 1];
      p.L[3] = lattice[mu];
      ++p.nd;
    }
    p.V *= lattice[mu];
    NF_REQUIRE(size_t(p.V) * elem <= kHmcFieldBytes,
               "%s: a chain of the lattice (%d, %d, %d, %d) does not fit the %zu KiB LDS image of the fused kernel", what,
               lattice[0], lattice[1], lattice[2], lattice[3], kHmcFieldBytes / 1024);
  }
  if (p.nd == 0) p.nd = 1;
  p.ns = 1;
  while ((p.V + p.ns - 1) / p.ns > kHmcMaxLanes) p.ns *= 2;
  const int lanes = int((p.V + p.ns - 1) / p.ns);
  p.nt = (lanes + kWave - 1) / kWave * kWave;
  p.lds = kHmcScratchBytes + ((size_t(p.V) * elem + 15) & ~size_t(15));
  return NF_OK;
}

struct HmcArgs {
  void *phi;
  double *action_out;
  const void *pi_in;
  void *pi_out;
  double *dh_out;
  uint8_t *accept_out;
  void *record;
  int64_t C, V;
  int L[4];
  double w0, w2, w4;
  int n_md, n_traj, record_every, force;
  uint32_t k0n, k1n, k0a, k1a;   // keys of the normal and of the accept stream
  uint64_t offset;
  HmcSteps steps;                // the scheme's update lengths (nf_sampler_core.h): uniform, read by scalar loads
};

// What MEASURE adds to the kernel's arguments; the kernels without it take HmcArgs as before.
struct HmcMeasureArgs : HmcArgs {
  double *measure;      // (n_traj / record_every, C, n_out)
  int Lm[4], moff[4];   // the caller's four extents (NOT HmcPlan's compressed ones) and the slice sums' offsets in a row
  int n_out, team;      // nf_lattice_measure_plan's n_out and lanes for the lattice
};

// What LADDER adds: the table of the K rungs' coefficients and the rung every chain holds.  A ladder launch without
// measure_out leaves the fields of HmcMeasureArgs unset; the kernel compiled without MEASURE does not read them.
struct HmcLadderArgs : HmcMeasureArgs {
  const double *coef;   // (K, 3): w0, w2, w4 of rung k, a user axis of extent 1 folded into w2
  const int32_t *rung;  // (C): the rung of chain c, clamped into 0 .. K - 1 by the kernel
  int K;
};

template <bool MEASURE, bool LADDER>
using HmcKernelArgs = std::conditional_t<LADDER, HmcLadderArgs, std::conditional_t<MEASURE, HmcMeasureArgs, HmcArgs>>;

// Sum of (a, b) over the workgroup, valid in every lane and the same bits in every lane: lane partials -> shuffle tree ->
// one slot per wave -> the waves added in order.  `slot` alternates between calls, so a slot is overwritten only after a
// barrier that follows its last read.
__device__ __forceinline__ void hmc_sum2(double &a, double &b, double *red, int &slot) {
  a = wave_sum(a);
  b = wave_sum(b);
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave, nw = blockDim.x / kWave;
  double *r = red + slot * (2 * kHmcMaxLanes / kWave);
  if (lane == 0) {
    r[2 * w] = a;
    r[2 * w + 1] = b;
  }
  __syncthreads();
  a = 0.0;
  b = 0.0;
  for (int i = 0; i < nw; ++i) {
    a += r[2 * i];
    b += r[2 * i + 1];
  }
  slot ^= 1;
}

// measure_image out of line, for the instantiations that keep 32 bytes or more of phi per lane (float x 8 and x 16, double x 4
// and x 8): inlined there it costs the MD loop scratch reloads; called, its registers are the callee's.  The LDS
// is named here, not handed in, so that the reads stay LDS reads: every dynamic extern array starts at the same base.
template <typename T>
__device__ __noinline__ void hmc_measure_image(int e0, int e1, int e2, int e3, int o0, int o1, int o2, int o3, int tl, int nt,
                                               double *dst, bool live) {
  extern __shared__ __align__(16) unsigned char hmc_lds_m[];
  double *mred = reinterpret_cast<double *>(hmc_lds_m + kHmcScratchBytes), *msp = mred + kHmcMsRed;
  const T *img = reinterpret_cast<const T *>(hmc_lds_m + kHmcScratchBytes + kHmcMsScratchBytes);
  const int E[4] = {e0, e1, e2, e3}, off[4] = {o0, o1, o2, o3};
  measure_image<T, false>(img, nullptr, nullptr, E, E, off, 0, -1, tl, nt, 0, 0, mred, msp, dst, live);
}

// The waves per SIMD that the light instantiations are compiled for -- float with one or two sites per lane and no
// measure code (7 and 6), and the 256-lane double kernel with the measure and the ladder code (4): what they had before
// the MD loop took its lengths from memory.  Left alone the register allocator spends a dozen registers more on them (on
// the unrolled reads of the wave sums, not on the loop), and a CU holds fewer chains of up to 2048 sites.  1: no request.
template <typename T, int NS, int LANES, bool MEASURE, bool LADDER>
constexpr int kHmcMinWaves = sizeof(T) == 4 ? (MEASURE || NS > 2 ? 1 : NS == 1 ? 7 : 6)
                                            : (LANES == 256 && MEASURE && LADDER ? 4 : 1);

template <typename T, int NS, int D, int LANES, bool MEASURE, bool LADDER>
__global__ __launch_bounds__(LANES, (kHmcMinWaves<T, NS, LANES, MEASURE, LADDER>))
void phi4_hmc_kernel(HmcKernelArgs<MEASURE, LADDER> A) {
  extern __shared__ __align__(16) unsigned char hmc_lds[];
  double *red = reinterpret_cast<double *>(hmc_lds);                       // 2 slots x 16 waves x 2 doubles = 512 B
  int *s_ok = reinterpret_cast<int *>(hmc_lds + 512);
  T *img = reinterpret_cast<T *>(hmc_lds + kHmcScratchBytes + (MEASURE ? kHmcMsScratchBytes : 0));
  constexpr int PER = sizeof(T) == 4 ? 4 : 2;
  const int tid = threadIdx.x, NT = blockDim.x;
  const int V = int(A.V);
  const int64_t c = blockIdx.x;
  T *__restrict__ gphi = static_cast<T *>(A.phi) + c * A.V;
  // The chain's coefficients and its column `oc` in the time series (dh_out, accept_out, record, measure).  LADDER: the
  // row rung[c] of the table, read once, and the column of that rung in the chain's replica set; the chain's own state
  // (phi, pi_in, pi_out, action_out) and its Philox draws stay at c.
  // Without LADDER the three are read from the arguments where they are used, as they always were.
  double lw0 = 0.0, lw2 = 0.0, lw4 = 0.0;
  int64_t oc = c;
  if constexpr (LADDER) {
    const int r = min(max(int(A.rung[c]), 0), A.K - 1);
    const double *row = A.coef + 3 * int64_t(r);
    lw0 = V > 1 ? uniform_scalar(row[0]) : 0.0;             // a lattice of one site: the site is read as its own neighbour
    lw2 = uniform_scalar(row[1]);
    lw4 = uniform_scalar(row[2]);
    oc = c / A.K * A.K + r;
  }
  const T w0 = T(LADDER ? lw0 : A.w0), w2x2 = T(2) * T(LADDER ? lw2 : A.w2), w4x4 = T(4) * T(LADDER ? lw4 : A.w4);
  const int s3 = 1, s2 = A.L[3], s1 = A.L[3] * A.L[2], s0 = A.L[3] * A.L[2] * A.L[1];
  const int st[4] = {s0, s1, s2, s3};
  // A.L holds the D axes of extent > 1 (HmcPlan): axes 4 - D .. 3 have neighbours, the others are not looked at

  // Slot k of a lane is site tid + k NT.  A slot past the last site shadows site V - 1: it reads what that site reads and
  // computes what it computes, so the loops below have no divergent branch; only the stores and the energy sums ask
  // whether the slot owns its site.  Per slot one byte of wrap flags (bit 2 mu: x_mu == 0, bit 2 mu + 1: x_mu == L_mu - 1),
  // four slots per register.  The neighbour indices are three instructions each from a flag bit; left alone the compiler
  // hoists all 8 NS of them (and the global addresses of the passes at a trajectory's end) out of the loops and spills,
  // so every pass starts from `fresh()`: an empty asm that "writes" the lane index and the flag words keeps the index
  // arithmetic inside the loop.  What the compiler reports with that (1024-lane bound = 128 registers; -Rpass-analysis=
  // kernel-resource-usage): no scratch for float with 1 .. 8 sites per lane and double with 1 .. 4; float x 16 (24^3, 128^2)
  // 116 B per lane and double x 8 (8192 sites) 200 B per lane, spent in this prologue (the coordinate divisions) and in the
  // momentum draw of a trajectory (the double sincos); the MD loop of float x 16 has no scratch access, that of double x 8
  // one reload per step.  With MEASURE the numbers are DESIGN.md's (section 4.9): more registers around the measurement,
  // none of its scratch traffic in the MD loop; without it the instantiations report what they did before there was one.
  uint32_t flg[(NS + 3) / 4] = {};
  T phi[NS], pi[NS];
  auto site = [&](int tv, int k) { const int i = tv + k * NT; return i < V ? i : V - 1; };
  auto owns = [&](int tv, int k) { return tv + k * NT < V; };
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    const int i = site(tid, k);
    int r = i;
    const int x3 = r % A.L[3]; r /= A.L[3];
    const int x2 = r % A.L[2]; r /= A.L[2];
    const int x1 = r % A.L[1];
    const int x0 = r / A.L[1];
    const uint32_t f = uint32_t(x0 == 0) | uint32_t(x0 == A.L[0] - 1) << 1 | uint32_t(x1 == 0) << 2 |
                       uint32_t(x1 == A.L[1] - 1) << 3 | uint32_t(x2 == 0) << 4 | uint32_t(x2 == A.L[2] - 1) << 5 |
                       uint32_t(x3 == 0) << 6 | uint32_t(x3 == A.L[3] - 1) << 7;
    flg[k >> 2] |= f << (8 * (k & 3));
    phi[k] = gphi[i];
    pi[k] = T(0);
    __builtin_amdgcn_sched_barrier(0);                   // one slot's divisions at a time
  }
  auto fresh = [&]() {
#pragma unroll
    for (int w = 0; w < (NS + 3) / 4; ++w) asm volatile("" : "+v"(flg[w]));
    int tv = tid;
    asm volatile("" : "+v"(tv));
    return tv;
  };
  auto back = [&](int i, uint32_t f, int mu) { return i + ((f >> (2 * mu)) & 1u ? st[mu] * (A.L[mu] - 1) : -st[mu]); };
  auto fwd = [&](int i, uint32_t f, int mu) { return i + ((f >> (2 * mu + 1)) & 1u ? -st[mu] * (A.L[mu] - 1) : st[mu]); };

  // The scheme's lengths where the stage is a loop variable: read from the kernel's argument segment itself, in the
  // constant address space, so that a uniform index makes scalar loads.  (Indexing the by-value copy `A` with a variable
  // would make the compiler keep both arrays in vector registers.)  The kernel has one argument, at offset 0, and
  // HmcArgs is the first base of every argument struct.
  using KernArgByte = const __attribute__((address_space(4))) unsigned char;
  using KernArgDouble = const __attribute__((address_space(4))) double;
  KernArgDouble *lens = reinterpret_cast<KernArgDouble *>((KernArgByte *)__builtin_amdgcn_kernarg_segment_ptr() +
                                                         offsetof(HmcArgs, steps) + offsetof(HmcSteps, drift));
  static_assert(offsetof(HmcSteps, kick) == offsetof(HmcSteps, drift) + NF_HMC_MAX_STAGES * sizeof(double),
                "kick follows drift");
  // An update length of the scheme, cast to the field type: uniform, and kept in scalar registers
  auto length = [&](double v) {
    if constexpr (sizeof(T) == 4)
      return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(uint32_t, float(v))));
    else
      return v;
  };
  // pi -= step * F(phi), the neighbours from the image (which holds phi)
  auto kick = [&](T step) {
    const int tv = fresh();
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      const int i = site(tv, k);
      const uint32_t f = (flg[k >> 2] >> (8 * (k & 3))) & 255u;
      T nb = T(0);
#pragma unroll
      for (int mu = 4 - D; mu < 4; ++mu) nb += img[back(i, f, mu)] + img[fwd(i, f, mu)];
      const T p = phi[k];
      pi[k] -= step * phi4_force(p, nb, w2x2, w4x4, w0);
      __builtin_amdgcn_sched_barrier(0);               // one slot's 8 reads in flight at a time: the registers go to phi and pi
    }
  };
  // lane partials of sum pi^2 / 2 and of S(phi) (phi4_site_energy), in double on the values cast to double
  auto energy = [&](double &kin, double &pot) {
    kin = 0.0;
    pot = 0.0;
    const int tv = fresh();
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      const int i = site(tv, k);
      const uint32_t f = (flg[k >> 2] >> (8 * (k & 3))) & 255u;
      double nb = 0.0;
#pragma unroll
      for (int mu = 4 - D; mu < 4; ++mu) nb += double(img[back(i, f, mu)]);
      const double p = double(phi[k]), q = double(pi[k]);
      const bool mine = owns(tv, k);
      kin += mine ? 0.5 * q * q : 0.0;
      pot += mine ? phi4_site_energy(p, nb, LADDER ? lw0 : A.w0, LADDER ? lw2 : A.w2, LADDER ? lw4 : A.w4) : 0.0;
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  auto put_image = [&]() {
    const int tv = fresh();
#pragma unroll
    for (int k = 0; k < NS; ++k)
      if (owns(tv, k)) img[tv + k * NT] = phi[k];
  };

  double s_cur = 0.0;
  int slot = 0;
  const int64_t ngroups = (A.V + PER - 1) / PER;
  for (int t = 0; t < A.n_traj; ++t) {
    // ---- momenta: the image is the transit buffer from the Philox groups (PER consecutive sites) to the lanes' sites
    if (A.pi_in) {
      const T *__restrict__ gpi = static_cast<const T *>(A.pi_in) + c * A.V;
#pragma unroll
      for (int k = 0; k < NS; ++k) pi[k] = gpi[site(tid, k)];
    } else {
      __syncthreads();                                   // the previous trajectory's reads of the image are done
      const uint64_t off = A.offset + 2 * uint64_t(t);
      const PhiloxPos at{A.k0n, A.k1n, uint32_t(off), uint32_t(off >> 32)};
      for (int64_t q = tid; q < ngroups; q += NT) {
        T z[PER];
        philox_normal_group<T>(at, uint64_t(c) * uint64_t(ngroups) + uint64_t(q), z);
#pragma unroll
        for (int j = 0; j < PER; ++j)
          if (q * PER + j < A.V) img[q * PER + j] = z[j];
      }
      __syncthreads();
      const int tv = fresh();
#pragma unroll
      for (int k = 0; k < NS; ++k) pi[k] = img[site(tv, k)];
    }
    __syncthreads();                                     // the momenta are read (with pi_in: nothing reads the image yet)
    put_image();
    __syncthreads();
    double k0, e0;
    energy(k0, e0);
    hmc_sum2(k0, e0, red, slot);
    // ---- the molecular dynamics: n_md steps of the scheme's stages, one force evaluation (two barriers) per stage; the
    // loop's bounds and lengths are uniform, so every barrier below is met by the whole workgroup
    const T hdt = length(A.steps.kick_half);
    kick(hdt);
    {
      // one flat loop over the n_md s force evaluations, its body straight-line code; the two lengths of a stage are
      // two scalar loads at a uniform index (leapfrog: always the same two), asked for one stage ahead so that they
      // arrive behind the barriers of the stage before
      const int evals = A.n_md * A.steps.stages;
      double da = lens[0], db = lens[NF_HMC_MAX_STAGES];
      for (int n = 1, j = 0; n <= evals; ++n) {
        j = j + 1 == A.steps.stages ? 0 : j + 1;
        const double na = lens[j], nb = lens[NF_HMC_MAX_STAGES + j];
        const T ta = length(da);
#pragma unroll
        for (int q = 0; q < NS; ++q) phi[q] += ta * pi[q];
        __syncthreads();                                 // every lane has read the old image
        put_image();
        __syncthreads();
        kick(n == evals ? hdt : length(db));
        da = na;
        db = nb;
      }
    }
    double k1, e1;
    energy(k1, e1);
    hmc_sum2(k1, e1, red, slot);
    // ---- the decision: one lane decides, the workgroup reads it from LDS
    if (tid == 0) {
      const double dh = (k1 + e1) - (k0 + e0);
      const uint64_t offa = A.offset + 2 * uint64_t(t) + 1;
      const PhiloxPos at{A.k0a, A.k1a, uint32_t(offa), uint32_t(offa >> 32)};
      const bool ok = hmc_accepts(philox_log_uniform(at, uint64_t(c)), dh, A.force);
      A.dh_out[int64_t(t) * A.C + oc] = dh;
      A.accept_out[int64_t(t) * A.C + oc] = uint8_t(ok);
      *s_ok = int(ok);
    }
    __syncthreads();
    const bool ok = *s_ok != 0;
    s_cur = ok ? e1 : e0;
    const int tg = fresh();                              // the global addresses of the passes below are not kept either
    if (t + 1 == A.n_traj && A.pi_out) {
      T *__restrict__ gpo = static_cast<T *>(A.pi_out) + c * A.V;
#pragma unroll
      for (int k = 0; k < NS; ++k)
        if (owns(tg, k)) gpo[tg + k * NT] = pi[k];
    }
    if (ok) {
#pragma unroll
      for (int k = 0; k < NS; ++k)
        if (owns(tg, k)) gphi[tg + k * NT] = phi[k];
    } else {
      // a lane reads back what it stored itself, or what nobody has written in this launch; a shadow slot reads site
      // V - 1, which its owner may be storing in this very pass -- on accept only, and then no slot reads
#pragma unroll
      for (int k = 0; k < NS; ++k) phi[k] = gphi[site(tg, k)];
    }
    if (A.record && (t + 1) % A.record_every == 0) {
      T *__restrict__ rec = static_cast<T *>(A.record) + (int64_t((t + 1) / A.record_every - 1) * A.C + oc) * A.V;
#pragma unroll
      for (int k = 0; k < NS; ++k)
        if (owns(tg, k)) rec[tg + k * NT] = phi[k];
    }
    if constexpr (MEASURE) {
      if ((t + 1) % A.record_every == 0) {
        // the image holds the proposal; the registers hold the chain's state (restored above on a reject)
        __syncthreads();
        put_image();
        __syncthreads();
        double *mred = reinterpret_cast<double *>(hmc_lds + kHmcScratchBytes), *msp = mred + kHmcMsRed;
        int E[4], off[4];
#pragma unroll
        for (int mu = 0; mu < 4; ++mu) {
          E[mu] = A.Lm[mu];
          off[mu] = A.moff[mu];
        }
        // lanes 0 .. team - 1 are nf_lattice_measure's team for the lattice (its first wave 0, its first lane 0); the
        // other waves run empty loops and meet the barriers
        const bool team = tid < A.team;
        double *dst = A.measure + (int64_t((t + 1) / A.record_every - 1) * A.C + oc) * A.n_out;
        if constexpr (NS * sizeof(T) >= 32)
          hmc_measure_image<T>(E[0], E[1], E[2], E[3], off[0], off[1], off[2], off[3], team ? tid : kHmcIdleLane, A.team, dst,
                               team);
        else
          measure_image<T, false>(img, nullptr, nullptr, E, E, off, 0, -1, team ? tid : kHmcIdleLane, A.team, 0, 0, mred, msp,
                                  dst, team);
        __syncthreads();                                 // before the next trajectory's momenta pass through the image
      }
    }
  }
  if (tid == 0) A.action_out[c] = s_cur;
}

// Args: HmcArgs launches the kernel as it always was, HmcMeasureArgs the one compiled with MEASURE, HmcLadderArgs the
// ones compiled with LADDER (with and without MEASURE: a ladder launch may leave measure_out NULL)
template <typename Args> constexpr bool kHmcLadder = std::is_same_v<Args, HmcLadderArgs>;
template <typename Args, bool MEASURE>
constexpr const char *kHmcName = kHmcLadder<Args> ? "nf_phi4_hmc_ladder" : MEASURE ? "nf_phi4_hmc_measure" : "nf_phi4_hmc";

template <typename T, int NS, int D, int LANES, bool MEASURE, typename Args>
static int launch_hmc(const Args &A, const HmcPlan &p, hipStream_t s) {
  static_assert(std::is_same_v<Args, HmcKernelArgs<MEASURE, kHmcLadder<Args>>>, "the arguments of another instantiation");
  auto kern = phi4_hmc_kernel<T, NS, D, LANES, MEASURE, kHmcLadder<Args>>;
  const size_t lds = p.lds + (MEASURE ? kHmcMsScratchBytes : 0);
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                          int(lds)) != hipSuccess) {
    (void)hipGetLastError();
    set_error("%s: cannot raise the dynamic LDS limit to %zu B", kHmcName<Args, MEASURE>, lds);
    return NF_ELAUNCH;
  }
  hipLaunchKernelGGL(kern, dim3(unsigned(A.C)), dim3(unsigned(p.nt)), lds, s, A);
  return check_launch(kHmcName<Args, MEASURE>);
}

template <typename T, int D, bool MEASURE, typename Args>
static int dispatch_ns(const Args &A, const HmcPlan &p, hipStream_t s) {
  switch (p.ns) {
    // one site per lane on up to 256 lanes (V <= 256) is compiled for 256 lanes: twice the registers of the 1024-lane bound
    case 1:
      return p.nt <= 256 ? launch_hmc<T, 1, D, 256, MEASURE>(A, p, s) : launch_hmc<T, 1, D, kHmcMaxLanes, MEASURE>(A, p, s);
    case 2: return launch_hmc<T, 2, D, kHmcMaxLanes, MEASURE>(A, p, s);     // more than one site per lane: always above 512 lanes
    case 4: return launch_hmc<T, 4, D, kHmcMaxLanes, MEASURE>(A, p, s);
    case 8: return launch_hmc<T, 8, D, kHmcMaxLanes, MEASURE>(A, p, s);
    case 16:
      if constexpr (sizeof(T) == 4) return launch_hmc<T, 16, D, kHmcMaxLanes, MEASURE>(A, p, s);   // 8-byte fields end at 8 sites per lane
  }
  set_error("%s: no kernel for %d sites per lane", kHmcName<Args, MEASURE>, p.ns);
  return NF_EINVAL;
}

template <typename T, bool MEASURE, typename Args>
static int dispatch_hmc(const Args &A, const HmcPlan &p, hipStream_t s) {
  switch (p.nd) {
    case 1: return dispatch_ns<T, 1, MEASURE>(A, p, s);
    case 2: return dispatch_ns<T, 2, MEASURE>(A, p, s);
    case 3: return dispatch_ns<T, 3, MEASURE>(A, p, s);
    default: return dispatch_ns<T, 4, MEASURE>(A, p, s);
  }
}

}  // namespace nf

using namespace nf;

extern "C" int nf_phi4_hmc_supported(const int32_t *lattice, int dtype) {
  HmcPlan p;
  return hmc_plan("nf_phi4_hmc_supported", lattice, dtype, p) == NF_OK ? 1 : 0;
}

// The body of nf_phi4_hmc (measure_out unused, measures = false), of nf_phi4_hmc_measure and of nf_phi4_hmc_ladder
// (coef != NULL or ladder: the three scalars unused, measures = measure_out given).
static int hmc_entry(const char *what, bool ladder, bool measures, double *measure_out, void *phi, double *action_out,
                     const void *pi_in, void *pi_out, double *dh_out, uint8_t *accept_out, void *record, int record_every,
                     int64_t C, const int32_t *lattice, double w0, double w2, double w4, const double *coef, int K,
                     const int32_t *rung, int n_md, double dt, int n_traj, int force_accept, uint64_t seed, uint64_t offset,
                     int dtype, void *stream, const nf_hmc_scheme *scheme) {
  HmcSteps steps;
  int rc = hmc_steps(what, scheme, dt, steps);           // the scheme first: a bad one is refused before anything else
  if (rc) return rc;
  const HmcCall Kc{phi, action_out, pi_in, pi_out, dh_out, accept_out, record, record_every, C, n_md, n_traj,
                   force_accept != 0, seed, offset};     // for the shared checks only: HmcArgs below keeps its kernel layout
  HmcPlan p;
  rc = hmc_call_checks(what, Kc);
  if (!rc && ladder) rc = hmc_ladder_checks(what, coef, K, rung, C);
  if (!rc) rc = hmc_plan(what, lattice, dtype, p);
  if (rc) return rc;
  NF_REQUIRE(ladder || !measures || measure_out != nullptr, "%s: measure_out is NULL", what);
  // an MD step costs two barriers however few the sites: below 256 sites the steps, not the sites, set the time; and the
  // chains beyond the resident ones wait for a free CU: the time grows with every further 1024 chains
  // the caps count force evaluations: n_md s of them per trajectory, s the stages of the scheme (1: leapfrog)
  const int64_t per_step = (p.V > 256 ? p.V : 256) * ((C + 1023) / 1024);
  const int64_t evals = int64_t(n_md) * steps.stages;
  if (!measures) {
    const int64_t work = evals * int64_t(n_traj) * per_step;
    NF_REQUIRE(work <= NF_HMC_MAX_WORK,
               "%s: n_md s n_traj max(V, 256) ceil(C / 1024) = %lld (s = %d stages) exceeds NF_HMC_MAX_WORK (%lld): split "
               "the run into several launches", what, (long long)work, steps.stages, (long long)NF_HMC_MAX_WORK);
  } else {
    const int64_t work = (evals * int64_t(n_traj) + int64_t(NF_HMC_MEASURE_MD_STEPS) * (n_traj / record_every)) * per_step;
    NF_REQUIRE(work <= NF_HMC_MAX_WORK,
               "%s: (n_md s n_traj + NF_HMC_MEASURE_MD_STEPS (n_traj / record_every)) max(V, 256) "
               "ceil(C / 1024) = %lld (s = %d stages) exceeds NF_HMC_MAX_WORK (%lld): split the run into several launches",
               what, (long long)work, steps.stages, (long long)NF_HMC_MAX_WORK);
  }
  HmcLadderArgs A{};
  A.phi = phi; A.action_out = action_out; A.pi_in = pi_in; A.pi_out = pi_out; A.dh_out = dh_out; A.accept_out = accept_out;
  A.record = record; A.C = C; A.V = p.V;
  for (int mu = 0; mu < 4; ++mu) A.L[mu] = p.L[mu];
  A.w0 = p.V > 1 ? w0 : 0.0;     // the one site of a lattice of one site is read as its own neighbour: weight 0
  A.w2 = w2; A.w4 = w4; A.steps = steps;
  A.n_md = n_md; A.n_traj = n_traj; A.record_every = record_every; A.force = force_accept != 0;
  // the keys of the two streams; the kernel adds 2 t (+ 1) to the offset itself
  const PhiloxPos kn = philox_pos(seed, NF_PHILOX_KEY_DOMAIN, offset), ka = philox_pos(seed, NF_PHILOX_ACCEPT_DOMAIN, offset);
  A.k0n = kn.k0; A.k1n = kn.k1; A.k0a = ka.k0; A.k1a = ka.k1;
  A.offset = offset;
  A.coef = coef; A.rung = rung; A.K = K;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (!measures) {
    if (ladder) return dtype == NF_F32 ? dispatch_hmc<float, false>(A, p, s) : dispatch_hmc<double, false>(A, p, s);
    const HmcArgs &B = A;
    return dtype == NF_F32 ? dispatch_hmc<float, false>(B, p, s) : dispatch_hmc<double, false>(B, p, s);
  }
  // the team and the row layout are nf_lattice_measure's own plan for the lattice: a chain that fits the image is one of
  // its packed or resident rows
  nf_measure_plan mp;
  rc = nf_lattice_measure_plan(lattice, dtype, &mp);
  if (rc) return rc;
  NF_REQUIRE(mp.segments == 1 && mp.lanes <= p.nt && mp.lanes <= kMsMaxLanes,
             "%s: the measure team of %d lanes (%d segments) does not fit the %d lanes of a chain", what, mp.lanes,
             mp.segments, p.nt);
  A.measure = measure_out;
  A.n_out = mp.n_out;
  A.team = mp.lanes;
  int at = 0;
  for (int mu = 0; mu < 4; ++mu) {
    A.Lm[mu] = lattice[mu];
    A.moff[mu] = at;
    at += lattice[mu];
  }
  if (ladder) return dtype == NF_F32 ? dispatch_hmc<float, true>(A, p, s) : dispatch_hmc<double, true>(A, p, s);
  const HmcMeasureArgs &M = A;
  return dtype == NF_F32 ? dispatch_hmc<float, true>(M, p, s) : dispatch_hmc<double, true>(M, p, s);
}

extern "C" int nf_phi4_hmc_plan(const int32_t *lattice, int dtype, nf_hmc_plan *out) {
  NF_REQUIRE(out != nullptr, "nf_phi4_hmc_plan: out is NULL");
  HmcPlan p;
  const int rc = hmc_plan("nf_phi4_hmc_plan", lattice, dtype, p);
  if (rc) return rc;
  out->sites_per_lane = p.ns;
  out->lanes = p.nt;
  out->lds_bytes = int64_t(p.lds);
  out->lds_bytes_measure = int64_t(p.lds + kHmcMsScratchBytes);
  return NF_OK;
}

extern "C" int nf_phi4_hmc(void *phi, double *action_out, const void *pi_in, void *pi_out, double *dh_out,
                           uint8_t *accept_out, void *record, int record_every, int64_t C, const int32_t *lattice,
                           double w0, double w2, double w4, int n_md, double dt, int n_traj, int force_accept,
                           uint64_t seed, uint64_t offset, int dtype, void *stream) {
  return hmc_entry("nf_phi4_hmc", false, false, nullptr, phi, action_out, pi_in, pi_out, dh_out, accept_out, record,
                   record_every, C, lattice, w0, w2, w4, nullptr, 0, nullptr, n_md, dt, n_traj, force_accept, seed, offset,
                   dtype, stream, nullptr);
}

extern "C" int nf_phi4_hmc_measure(void *phi, double *action_out, const void *pi_in, void *pi_out, double *dh_out,
                                   uint8_t *accept_out, void *record, double *measure_out, int record_every, int64_t C,
                                   const int32_t *lattice, double w0, double w2, double w4, int n_md, double dt, int n_traj,
                                   int force_accept, uint64_t seed, uint64_t offset, int dtype, void *stream) {
  return hmc_entry("nf_phi4_hmc_measure", false, true, measure_out, phi, action_out, pi_in, pi_out, dh_out, accept_out,
                   record, record_every, C, lattice, w0, w2, w4, nullptr, 0, nullptr, n_md, dt, n_traj, force_accept, seed,
                   offset, dtype, stream, nullptr);
}

extern "C" int nf_phi4_hmc_ladder(void *phi, double *action_out, const void *pi_in, void *pi_out, double *dh_out,
                                  uint8_t *accept_out, void *record, double *measure_out, int record_every, int64_t C,
                                  const int32_t *lattice, const double *coef, int K, const int32_t *rung, int n_md, double dt,
                                  int n_traj, int force_accept, uint64_t seed, uint64_t offset, int dtype, void *stream) {
  return hmc_entry("nf_phi4_hmc_ladder", true, measure_out != nullptr, measure_out, phi, action_out, pi_in, pi_out, dh_out,
                   accept_out, record, record_every, C, lattice, 0.0, 0.0, 0.0, coef, K, rung, n_md, dt, n_traj,
                   force_accept, seed, offset, dtype, stream, nullptr);
}

// The same launchers with an integration scheme (NULL: leapfrog, the launchers above).
extern "C" int nf_phi4_hmc_scheme(void *phi, double *action_out, const void *pi_in, void *pi_out, double *dh_out,
                           uint8_t *accept_out, void *record, int record_every, int64_t C, const int32_t *lattice,
                           double w0, double w2, double w4, int n_md, double dt, int n_traj, int force_accept,
                           uint64_t seed, uint64_t offset, int dtype, void *stream, const nf_hmc_scheme *scheme) {
  return hmc_entry("nf_phi4_hmc_scheme", false, false, nullptr, phi, action_out, pi_in, pi_out, dh_out, accept_out, record,
                   record_every, C, lattice, w0, w2, w4, nullptr, 0, nullptr, n_md, dt, n_traj, force_accept, seed, offset,
                   dtype, stream, scheme);
}

extern "C" int nf_phi4_hmc_measure_scheme(void *phi, double *action_out, const void *pi_in, void *pi_out, double *dh_out,
                                   uint8_t *accept_out, void *record, double *measure_out, int record_every, int64_t C,
                                   const int32_t *lattice, double w0, double w2, double w4, int n_md, double dt, int n_traj,
                                   int force_accept, uint64_t seed, uint64_t offset, int dtype, void *stream, const nf_hmc_scheme *scheme) {
  return hmc_entry("nf_phi4_hmc_measure_scheme", false, true, measure_out, phi, action_out, pi_in, pi_out, dh_out, accept_out,
                   record, record_every, C, lattice, w0, w2, w4, nullptr, 0, nullptr, n_md, dt, n_traj, force_accept, seed,
                   offset, dtype, stream, scheme);
}

extern "C" int nf_phi4_hmc_ladder_scheme(void *phi, double *action_out, const void *pi_in, void *pi_out, double *dh_out,
                                  uint8_t *accept_out, void *record, double *measure_out, int record_every, int64_t C,
                                  const int32_t *lattice, const double *coef, int K, const int32_t *rung, int n_md, double dt,
                                  int n_traj, int force_accept, uint64_t seed, uint64_t offset, int dtype, void *stream, const nf_hmc_scheme *scheme) {
  return hmc_entry("nf_phi4_hmc_ladder_scheme", true, measure_out != nullptr, measure_out, phi, action_out, pi_in, pi_out, dh_out,
                   accept_out, record, record_every, C, lattice, 0.0, 0.0, 0.0, coef, K, rung, n_md, dt, n_traj,
                   force_accept, seed, offset, dtype, stream, scheme);
}

extern "C" int nf_hmc_scheme_check(const nf_hmc_scheme *scheme) { return hmc_scheme_checks("nf_hmc_scheme_check", scheme); }

extern "C" int nf_hmc_scheme_named(int which, nf_hmc_scheme *out) {
  NF_REQUIRE(out != nullptr, "nf_hmc_scheme_named: out is NULL");
  nf_hmc_scheme sc{};
  switch (which) {
    case NF_HMC_LEAPFROG:
      sc.stages = 1;
      sc.a[0] = sc.b[0] = 1.0;
      break;
    case NF_HMC_OMELYAN2: {
      const double lambda = 0.1931833275037836;
      sc.stages = 2;
      sc.a[0] = sc.a[1] = 0.5;
      sc.b[0] = 1.0 - 2.0 * lambda;
      sc.b[1] = 2.0 * lambda;
      break;
    }
    case NF_HMC_OMF4: {
      const double r1 = 0.08398315262876693, r2 = 0.2539785108410595, r3 = 0.6822365335719091, r4 = -0.03230286765269967;
      sc.stages = 5;
      sc.a[0] = sc.a[4] = r2;
      sc.a[1] = sc.a[3] = r4;
      sc.a[2] = 1.0 - 2.0 * (r2 + r4);
      sc.b[0] = sc.b[3] = r3;
      sc.b[1] = sc.b[2] = 0.5 - r1 - r3;
      sc.b[4] = 2.0 * r1;
      break;
    }
    default:
      set_error("nf_hmc_scheme_named: no scheme %d (NF_HMC_LEAPFROG, NF_HMC_OMELYAN2, NF_HMC_OMF4)", which);
      return NF_EINVAL;
  }
  *out = sc;
  return NF_OK;
}

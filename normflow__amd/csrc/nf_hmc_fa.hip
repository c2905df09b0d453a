// nf_hmc_fa.hip -- Fourier-accelerated hybrid Monte Carlo for the lattice phi^4 action, the chain resident in a CU
// (MI355X-side extension; the rule is include/normflow_hip.h, "Fourier-accelerated hybrid Monte Carlo").  nf_phi4_hmc's
// trajectory with the kinetic term pi^T A pi / 2, A = T diag(a) T, T the orthonormal separable Hartley transform of
// nf_spectral_core.h and a(k) = 1 / (w0 sum_mu shat_mu(k_mu) + M^2):
//   pi = A^(-1/2) eta;  H0 = sum pi (A pi) / 2 + S(phi);  pi -= (b_s / 2) dt F(phi);
//   stages: phi += a_j dt (A pi), pi -= b_j dt F(phi) (the last kick halved);  H1 likewise;  accept as nf_phi4_hmc does.
// One workgroup per chain runs ALL n_traj trajectories of its chain in one launch, with nf_phi4_hmc's lane map: lane `tid`
// of the NT lanes owns the sites tid + k NT (k < NS).  Storage: pi in registers; phi IN LDS (the image that the force's
// neighbour reads need is the chain's state itself: a drift adds to the lane's own sites of it); one transform buffer of V
// elements; the Hartley matrices, built once per launch.  Dynamic LDS = 2 V sizeof(T) + the matrices, nothing else: the
// reduction slots and the broadcast of the decision lie in the first bytes of the transform buffer, which is dead
// whenever an energy is summed (written as 32-bit words: the buffer of an odd fp32 lattice is 4-byte aligned).
// A filter "buf <- T diag(d) T buf" is: lanes write their own sites of buf | barrier | d passes | multiply own sites |
// barrier | d passes (a pass ends with its barrier).  The site index of buf after the first transform is the momentum
// index (k_0, .., k_3) row-major, so a lane multiplies by the a(k) of its OWN site indices: NS values of dtype, formed
// once per launch in double from the shat table and kept in registers (up to 8 sites per lane; beyond, the registers go to
// pi and a(k) is formed again in every filter).  The workgroup has at most 512 lanes, not nf_phi4_hmc's 1024: the tiles
// of the transform take about 100 (float) to 120 (double) registers, and 2 waves per SIMD leave 256.  The table (sum L_mu doubles, made by the host
// through sinpi) travels in the kernel's argument segment and is read from there: once per launch for a(k), once per
// trajectory for a^(-1/2) (the momentum refresh).  n_md s + 3 filters per trajectory: refresh, H0, one per drift, H1.
// Every barrier is in uniform control flow: the loops that hold them run over the kernel's arguments only.
// The energies are summed in double in a fixed order (lane partial over k, wave shuffle tree, waves in order): no atomics,
// the same inputs give the same bits, and a launch of n_traj trajectories equals n_traj launches of one.
#include <type_traits>

#include "nf_sampler_core.h"
#include "nf_spectral_core.h"

namespace nf {

constexpr int kFaMaxLanes = 512;                   // 2 waves per SIMD: 256 registers for pi, a(k) and the transform's tiles
constexpr size_t kFaFieldBytes = 64 * 1024;        // V sizeof(T) <= 64 KiB, as for nf_phi4_hmc
constexpr size_t kFaLdsBytes = 160 * 1024;         // LDS of a CU
constexpr int kFaMinSites = 8;                     // the slots of one wave (20 B) fit the buffer of 8 sites of either dtype
constexpr int kFaMaxTable = 4 * kSpecMaxAxis;      // entries of the shat table

struct FaPlan {
  int64_t V;
  int L[4];      // the extents above 1, in order, behind leading 1s (nf_phi4_hmc's HmcPlan)
  int ns, nt;    // sites per lane, lanes per chain (whole waves)
  HartleyAxes ax;
  size_t lds, hbytes;
};

// shat_mu(k) = 4 sin^2(pi k / L_mu), k = 0 .. L_mu - 1, for the four extents one behind the other (an axis of extent 1
// contributes its one entry 0): the one table every path shares.
// sinpi: the argument is folded exactly onto k' = min(k, L - k) <= L / 2 (so shat(k) = shat(L - k) bit for bit) and the sine
// taken in long double before the one rounding to double.
static void fa_table(const int L[4], double *out) {
  const long double pi = 3.14159265358979323846264338327950288L;
  for (int mu = 0, at = 0; mu < 4; ++mu)
    for (int k = 0; k < L[mu]; ++k) {
      const int kf = k < L[mu] - k ? k : L[mu] - k;
      const long double s = 2 * kf == L[mu] ? 1.0L : sinl(pi * (long double)kf / (long double)L[mu]);
      out[at++] = double(4.0L * s * s);
    }
}

static int fa_plan(const char *what, const int32_t *lattice, int dtype, FaPlan &p) {
  NF_REQUIRE(lattice != nullptr, "%s: lattice is NULL", what);
  NF_REQUIRE(dtype == NF_F32 || dtype == NF_F64, "%s: unsupported dtype %d (float32 and float64 fields)", what, dtype);
  const size_t elem = dtype == NF_F32 ? 4 : 8;
  p = FaPlan{};
  p.V = 1;
  for (int mu = 0; mu < 4; ++mu) p.L[mu] = 1;
  for (int mu = 0; mu < 4; ++mu) {
    NF_REQUIRE(lattice[mu] >= 1, "%s: lattice extents must be >= 1", what);
    NF_REQUIRE(lattice[mu] <= kSpecMaxAxis, "%s: axis of %d sites (1 to %d fit the LDS-resident transform)", what,
               lattice[mu], kSpecMaxAxis);
    if (lattice[mu] > 1) {
      for (int nu = 0; nu < 3; ++nu) p.L[nu] = p.L[nu + 1];
      p.L[3] = lattice[mu];
    }
    p.V *= lattice[mu];
  }
  NF_REQUIRE(size_t(p.V) * elem <= kFaFieldBytes,
             "%s: a chain of the lattice (%d, %d, %d, %d) does not fit the %zu KiB LDS image of the kernel", what,
             lattice[0], lattice[1], lattice[2], lattice[3], kFaFieldBytes / 1024);
  NF_REQUIRE(p.V >= kFaMinSites, "%s: a chain of %lld sites: the kernel takes lattices of %d sites or more", what,
             (long long)p.V, kFaMinSites);
  spectral_axes(p.ax, p.L);
  p.hbytes = size_t(p.ax.hsize) * elem;
  p.lds = 2 * size_t(p.V) * elem + p.hbytes;
  NF_REQUIRE(p.lds <= kFaLdsBytes,
             "%s: the image and the transform buffer of the lattice (%d, %d, %d, %d) (%zu B) and its Hartley matrices "
             "(%zu B) exceed the %zu B of LDS", what, lattice[0], lattice[1], lattice[2], lattice[3],
             2 * size_t(p.V) * elem, p.hbytes, kFaLdsBytes);
  p.ns = 1;
  while ((p.V + p.ns - 1) / p.ns > kFaMaxLanes) p.ns *= 2;
  const int lanes = int((p.V + p.ns - 1) / p.ns);
  p.nt = (lanes + kWave - 1) / kWave * kWave;
  return NF_OK;
}

struct FaArgs {
  void *phi;
  double *action_out;
  const void *pi_in;
  void *pi_out;
  double *dh_out;
  uint8_t *accept_out;
  void *record;
  int64_t C, V;
  int L[4], toff[4];             // the compressed extents and where the axis' entries start in `table`
  double w0, w2, w4, m2;
  int n_md, n_traj, record_every, force;
  uint32_t k0n, k1n, k0a, k1a;   // keys of the normal and of the accept stream
  uint64_t offset;
  HmcSteps steps;                // the scheme's update lengths (nf_sampler_core.h)
  HartleyAxes ax;
  double table[kFaMaxTable];     // shat of the compressed extents
};

template <typename T, int NS, int LANES>
__global__ __launch_bounds__(LANES) void phi4_hmc_fa_kernel(FaArgs A) {
  extern __shared__ __align__(16) unsigned char fa_lds[];
  const int tid = threadIdx.x, NT = blockDim.x;
  const int V = int(A.V);
  T *img = reinterpret_cast<T *>(fa_lds);                 // phi
  T *buf = img + V;                                       // the transform buffer
  T *hm = buf + V;                                        // the Hartley matrices
  uint32_t *slots = reinterpret_cast<uint32_t *>(buf);    // 4 words per wave, then the decision
  constexpr int PER = sizeof(T) == 4 ? 4 : 2;
  const int64_t c = blockIdx.x;
  T *__restrict__ gphi = static_cast<T *>(A.phi) + c * A.V;
  const T w0 = T(A.w0), w2x2 = T(2) * T(A.w2), w4x4 = T(4) * T(A.w4);
  const int st[4] = {A.L[3] * A.L[2] * A.L[1], A.L[3] * A.L[2], A.L[3], 1};

  // The kernel's argument segment in the constant address space: the table and the scheme's lengths are read from it at
  // variable indices (indexing the by-value copy would move the arrays into scratch).  One argument, at offset 0.
  using KernArgByte = const __attribute__((address_space(4))) unsigned char;
  using KernArgDouble = const __attribute__((address_space(4))) double;
  KernArgByte *seg = (KernArgByte *)__builtin_amdgcn_kernarg_segment_ptr();
  KernArgDouble *lens = reinterpret_cast<KernArgDouble *>(seg + offsetof(FaArgs, steps) + offsetof(HmcSteps, drift));
  KernArgDouble *table = reinterpret_cast<KernArgDouble *>(seg + offsetof(FaArgs, table));
  static_assert(offsetof(HmcSteps, kick) == offsetof(HmcSteps, drift) + NF_HMC_MAX_STAGES * sizeof(double),
                "kick follows drift");

  // Slot k of a lane is site tv + k NT (tv the lane index); a slot past the last site shadows site V - 1: it reads what
  // that site reads, and only the stores and the energy sums ask whether the slot owns its site.  Every pass starts from
  // `fresh()`: an empty asm that "writes" the lane index and the flag words keeps the index arithmetic of the 8 NS
  // neighbours and the addresses inside the pass instead of in registers across the transforms (nf_hmc.hip).
  auto site = [&](int tv, int k) { const int i = tv + k * NT; return i < V ? i : V - 1; };
  auto owns = [&](int tv, int k) { return tv + k * NT < V; };
  // w0 sum_mu shat_mu(x_mu) + M^2 at the site (= momentum) index i, in double, the axes left to right
  auto denom = [&](int i) {
    int r = i;
    const int x3 = r % A.L[3]; r /= A.L[3];
    const int x2 = r % A.L[2]; r /= A.L[2];
    const int x1 = r % A.L[1];
    const int x0 = r / A.L[1];
    const double s = ((table[A.toff[0] + x0] + table[A.toff[1] + x1]) + table[A.toff[2] + x2]) + table[A.toff[3] + x3];
    return A.w0 * s + A.m2;
  };

  // per slot one byte of wrap flags (bit 2 mu: x_mu == 0, bit 2 mu + 1: x_mu == L_mu - 1) and a(k) of the slot's index
  // (a(k) is kept for up to 8 sites per lane; beyond, the registers go to pi and a(k) is formed again in every filter)
  constexpr bool KEEP_A = NS <= 8;
  uint32_t flg[(NS + 3) / 4] = {};
  T pi[NS], ak[KEEP_A ? NS : 1];
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
    if constexpr (KEEP_A) ak[k] = T(1.0 / denom(i));
    pi[k] = T(0);
    __builtin_amdgcn_sched_barrier(0);                   // one slot's divisions at a time
  }
  for (int i = tid; i < V; i += NT) img[i] = gphi[i];     // a lane loads its own sites
  build_hartley(hm, A.ax, NT);
  __syncthreads();

  auto fresh = [&]() {
#pragma unroll
    for (int w = 0; w < (NS + 3) / 4; ++w) asm volatile("" : "+v"(flg[w]));
    int tv = tid;
    asm volatile("" : "+v"(tv));
    return tv;
  };
  auto back = [&](int i, uint32_t f, int mu) { return i + ((f >> (2 * mu)) & 1u ? st[mu] * (A.L[mu] - 1) : -st[mu]); };
  auto fwd = [&](int i, uint32_t f, int mu) { return i + ((f >> (2 * mu + 1)) & 1u ? -st[mu] * (A.L[mu] - 1) : st[mu]); };
  auto length = [&](double v) {
    if constexpr (sizeof(T) == 4)
      return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(uint32_t, float(v))));
    else
      return v;
  };
  // pi -= step * F(phi); an axis of extent 1 has no neighbours (uniform branch)
  auto kick = [&](T step) {
    const int tv = fresh();
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      const int i = site(tv, k);
      const uint32_t f = (flg[k >> 2] >> (8 * (k & 3))) & 255u;
      T nb = T(0);
#pragma unroll
      for (int mu = 0; mu < 4; ++mu)
        if (A.L[mu] > 1) nb += img[back(i, f, mu)] + img[fwd(i, f, mu)];
      pi[k] -= step * phi4_force(img[i], nb, w2x2, w4x4, w0);
      __builtin_amdgcn_sched_barrier(0);               // one slot's reads in flight at a time
    }
  };
  // (sum pi (A pi) / 2, S(phi)) over the chain, the same bits in every lane; buf holds A pi on entry and the slots on exit
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
      for (int mu = 0; mu < 4; ++mu)
        if (A.L[mu] > 1) nb += double(img[back(i, f, mu)]);
      const double p = double(img[i]), q = double(pi[k]), aq = double(buf[i]);
      const bool mine = owns(tv, k);
      kin += mine ? 0.5 * q * aq : 0.0;
      pot += mine ? phi4_site_energy(p, nb, A.w0, A.w2, A.w4) : 0.0;
      __builtin_amdgcn_sched_barrier(0);
    }
    kin = wave_sum(kin);
    pot = wave_sum(pot);
    const int lane = tid & (kWave - 1), w = tid / kWave, nw = NT / kWave;
    __syncthreads();                                     // every lane has read its A pi
    if (lane == 0) {
      const uint64_t a = __builtin_bit_cast(uint64_t, kin), b = __builtin_bit_cast(uint64_t, pot);
      slots[4 * w] = uint32_t(a); slots[4 * w + 1] = uint32_t(a >> 32);
      slots[4 * w + 2] = uint32_t(b); slots[4 * w + 3] = uint32_t(b >> 32);
    }
    __syncthreads();
    kin = 0.0;
    pot = 0.0;
    for (int j = 0; j < nw; ++j) {
      kin += __builtin_bit_cast(double, uint64_t(slots[4 * j + 1]) << 32 | slots[4 * j]);
      pot += __builtin_bit_cast(double, uint64_t(slots[4 * j + 3]) << 32 | slots[4 * j + 2]);
    }
  };

  double s_cur = 0.0;
  const int64_t ngroups = (A.V + PER - 1) / PER;
  const int nw = NT / kWave;
  const int evals = A.n_md * A.steps.stages;
  for (int t = 0; t < A.n_traj; ++t) {
    if (A.pi_in) {
      const T *__restrict__ gpi = static_cast<const T *>(A.pi_in) + c * A.V;
      const int tv = fresh();
#pragma unroll
      for (int k = 0; k < NS; ++k) pi[k] = gpi[site(tv, k)];
    }
    // The phases of a trajectory, ONE filter each, so that the two transforms of a filter are in the code once:
    //   n = -1           buf = eta;  filter with a^(-1/2);  pi = buf                       (skipped with pi_in)
    //   n = 0            buf = pi;   filter with a;  H0;  pi -= (b_s / 2) dt F
    //   n = 1 .. evals   buf = pi;   filter with a;  phi += a_j dt buf;  pi -= b_j dt F    (b_s / 2 at n = evals)
    //   n = evals + 1    buf = pi;   filter with a;  H1
    // n and every bound are uniform: every barrier below is met by the whole workgroup.  A lane writes only its own
    // sites of buf outside a transform (the draw apart, between two barriers), and reads of other lanes' sites of buf
    // (a shadow slot's) are followed by a barrier before the next write.
    const T hdt = length(A.steps.kick_half);
    double k0 = 0.0, e0 = 0.0, k1 = 0.0, e1 = 0.0;
    for (int n = A.pi_in ? 0 : -1, j = 0; n <= evals + 1; ++n) {
      const bool refresh = n < 0;
      if (refresh) {
        __syncthreads();                                 // the previous trajectory's reads of the slots are done
        const uint64_t off = A.offset + 2 * uint64_t(t);
        const PhiloxPos at{A.k0n, A.k1n, uint32_t(off), uint32_t(off >> 32)};
        for (int64_t q = tid; q < ngroups; q += NT) {
          T z[PER];
          philox_normal_group<T>(at, uint64_t(c) * uint64_t(ngroups) + uint64_t(q), z);
#pragma unroll
          for (int jj = 0; jj < PER; ++jj)
            if (q * PER + jj < A.V) buf[q * PER + jj] = z[jj];
        }
      } else {
        const int tv = fresh();
#pragma unroll
        for (int k = 0; k < NS; ++k)
          if (owns(tv, k)) buf[tv + k * NT] = pi[k];
      }
      __syncthreads();
      // ---- the filter: buf <- T diag(d) T buf; the site index between the transforms is the momentum index
      transform(buf, hm, A.ax, 1, NT);
      if constexpr (KEEP_A) {
        const int tv = fresh();
#pragma unroll
        for (int k = 0; k < NS; ++k)
          if (owns(tv, k)) {
            const int i = tv + k * NT;
            buf[i] *= refresh ? T(::sqrt(denom(i))) : ak[k];
            __builtin_amdgcn_sched_barrier(0);
          }
      } else {
        // nothing of the lane's registers is indexed: a plain loop over the lane's sites
#pragma unroll 1
        for (int i = tid; i < V; i += NT) buf[i] *= refresh ? T(::sqrt(denom(i))) : T(1.0 / denom(i));
      }
      __syncthreads();
      transform(buf, hm, A.ax, 1, NT);
      // ---- what the phase does with it
      if (refresh) {
        const int tv = fresh();
#pragma unroll
        for (int k = 0; k < NS; ++k) pi[k] = buf[site(tv, k)];
        __syncthreads();
      } else if (n == 0) {
        energy(k0, e0);
        kick(hdt);
        __syncthreads();                                 // the slots are read before the next phase writes the buffer
      } else if (n <= evals) {
        const T ta = length(lens[j]), tb = length(lens[NF_HMC_MAX_STAGES + j]);
        j = j + 1 == A.steps.stages ? 0 : j + 1;
        const int tv = fresh();
#pragma unroll
        for (int k = 0; k < NS; ++k)
          if (owns(tv, k)) img[tv + k * NT] += ta * buf[tv + k * NT];     // the lane's own sites of both
        __syncthreads();
        kick(n == evals ? hdt : tb);
      } else {
        energy(k1, e1);
      }
    }
    // ---- the decision: one lane decides, the workgroup reads it from LDS (the word behind the waves' slots)
    if (tid == 0) {
      const double dh = (k1 + e1) - (k0 + e0);
      const uint64_t offa = A.offset + 2 * uint64_t(t) + 1;
      const PhiloxPos at{A.k0a, A.k1a, uint32_t(offa), uint32_t(offa >> 32)};
      const bool ok = hmc_accepts(philox_log_uniform(at, uint64_t(c)), dh, A.force);
      A.dh_out[int64_t(t) * A.C + c] = dh;
      A.accept_out[int64_t(t) * A.C + c] = uint8_t(ok);
      slots[4 * nw] = uint32_t(ok);
    }
    __syncthreads();
    const bool ok = slots[4 * nw] != 0;
    s_cur = ok ? e1 : e0;
    const int tg = fresh();
    if (t + 1 == A.n_traj && A.pi_out) {
      T *__restrict__ gpo = static_cast<T *>(A.pi_out) + c * A.V;
#pragma unroll
      for (int k = 0; k < NS; ++k)
        if (owns(tg, k)) gpo[tg + k * NT] = pi[k];
    }
    // the chain in HBM is written only on accept and read back on reject: a rejected chain keeps its bits, and a lane
    // reads back what it stored itself or what nobody has written in this launch
#pragma unroll
    for (int k = 0; k < NS; ++k)
      if (owns(tg, k)) {
        const int i = tg + k * NT;
        if (ok) gphi[i] = img[i];
        else img[i] = gphi[i];
      }
    if (A.record && (t + 1) % A.record_every == 0) {
      T *__restrict__ rec = static_cast<T *>(A.record) + (int64_t((t + 1) / A.record_every - 1) * A.C + c) * A.V;
#pragma unroll
      for (int k = 0; k < NS; ++k)
        if (owns(tg, k)) rec[tg + k * NT] = img[tg + k * NT];
    }
  }
  if (tid == 0) A.action_out[c] = s_cur;
}

template <typename T, int NS, int LANES>
static int launch_fa(const FaArgs &A, const FaPlan &p, hipStream_t s) {
  auto kern = phi4_hmc_fa_kernel<T, NS, LANES>;
  if (p.lds > 64 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                          int(p.lds)) != hipSuccess) {
    (void)hipGetLastError();
    set_error("nf_phi4_hmc_fa: cannot raise the dynamic LDS limit to %zu B", p.lds);
    return NF_ELAUNCH;
  }
  hipLaunchKernelGGL(kern, dim3(unsigned(A.C)), dim3(unsigned(p.nt)), p.lds, s, A);
  return check_launch("nf_phi4_hmc_fa");
}

template <typename T>
static int dispatch_fa(const FaArgs &A, const FaPlan &p, hipStream_t s) {
  switch (p.ns) {
    case 1: return p.nt <= 256 ? launch_fa<T, 1, 256>(A, p, s) : launch_fa<T, 1, kFaMaxLanes>(A, p, s);
    case 2: return launch_fa<T, 2, kFaMaxLanes>(A, p, s);
    case 4: return launch_fa<T, 4, kFaMaxLanes>(A, p, s);
    case 8: return launch_fa<T, 8, kFaMaxLanes>(A, p, s);
    case 16: return launch_fa<T, 16, kFaMaxLanes>(A, p, s);
    case 32:
      if constexpr (sizeof(T) == 4) return launch_fa<T, 32, kFaMaxLanes>(A, p, s);   // 8-byte fields end at 16 sites per lane
  }
  set_error("nf_phi4_hmc_fa: no kernel for %d sites per lane", p.ns);
  return NF_EINVAL;
}

}  // namespace nf

using namespace nf;

extern "C" int nf_phi4_hmc_fa_supported(const int32_t *lattice, int dtype) {
  FaPlan p;
  return fa_plan("nf_phi4_hmc_fa_supported", lattice, dtype, p) == NF_OK ? 1 : 0;
}

extern "C" int nf_phi4_hmc_fa_plan(const int32_t *lattice, int dtype, int n_md, int stages, nf_hmc_fa_plan *out) {
  NF_REQUIRE(out != nullptr, "nf_phi4_hmc_fa_plan: out is NULL");
  NF_REQUIRE(n_md >= 1 && stages >= 1 && stages <= NF_HMC_MAX_STAGES,
             "nf_phi4_hmc_fa_plan: n_md (%d) must be >= 1 and stages (%d) in 1 .. %d", n_md, stages, NF_HMC_MAX_STAGES);
  FaPlan p;
  const int rc = fa_plan("nf_phi4_hmc_fa_plan", lattice, dtype, p);
  if (rc) return rc;
  out->sites_per_lane = p.ns;
  out->lanes = p.nt;
  out->phi_in_lds = 1;
  out->pi_in_lds = 0;
  out->lds_bytes = int64_t(p.lds);
  out->matrix_bytes = int64_t(p.hbytes);
  out->filters = int64_t(n_md) * stages + 3;
  return NF_OK;
}

extern "C" int nf_phi4_hmc_fa_table(const int32_t *lattice, double *out) {
  NF_REQUIRE(lattice != nullptr && out != nullptr, "nf_phi4_hmc_fa_table: NULL pointer argument");
  int L[4];
  for (int mu = 0; mu < 4; ++mu) {
    NF_REQUIRE(lattice[mu] >= 1, "nf_phi4_hmc_fa_table: lattice extents must be >= 1");
    L[mu] = lattice[mu];
  }
  fa_table(L, out);
  return NF_OK;
}

extern "C" int nf_phi4_hmc_fa(void *phi, double *action_out, const void *pi_in, void *pi_out, double *dh_out,
                              uint8_t *accept_out, void *record, int record_every, int64_t C, const int32_t *lattice,
                              double w0, double w2, double w4, int n_md, double dt, int n_traj, int force_accept,
                              uint64_t seed, uint64_t offset, int dtype, void *stream, const nf_hmc_scheme *scheme,
                              double fa_mass_sq) {
  const char *what = "nf_phi4_hmc_fa";
  HmcSteps steps;
  int rc = hmc_steps(what, scheme, dt, steps);           // the scheme first, as the other launchers do
  if (rc) return rc;
  const HmcCall Kc{phi, action_out, pi_in, pi_out, dh_out, accept_out, record, record_every, C, n_md, n_traj,
                   force_accept != 0, seed, offset};
  rc = hmc_call_checks(what, Kc);
  FaPlan p;
  if (!rc) rc = fa_plan(what, lattice, dtype, p);
  if (rc) return rc;
  // nf_phi4_hmc's cap with a filter counted as NF_HMC_FA_MD_STEPS MD steps: n_md s force evaluations and n_md s + 3
  // filters per trajectory
  const int64_t per_step = (p.V > 256 ? p.V : 256) * ((C + 1023) / 1024);
  const int64_t evals = int64_t(n_md) * steps.stages;
  const int64_t work = (evals + int64_t(NF_HMC_FA_MD_STEPS) * (evals + 3)) * int64_t(n_traj) * per_step;
  NF_REQUIRE(work <= NF_HMC_MAX_WORK,
             "%s: (n_md s + NF_HMC_FA_MD_STEPS (n_md s + 3)) n_traj max(V, 256) ceil(C / 1024) = %lld (s = %d stages) "
             "exceeds NF_HMC_MAX_WORK (%lld): split the run into several launches", what, (long long)work, steps.stages,
             (long long)NF_HMC_MAX_WORK);
  // the operator last, so that every refusal above can be met without a launch behind it
  NF_REQUIRE(std::isfinite(fa_mass_sq), "%s: fa_mass_sq (%g) is not finite", what, fa_mass_sq);
  NF_REQUIRE(fa_mass_sq > 0.0, "%s: fa_mass_sq (%g) must be > 0: a(k) = 1 / (w0 khat^2 + M^2) at k = 0", what, fa_mass_sq);
  NF_REQUIRE(w0 >= 0.0, "%s: w0 (%g) must be >= 0: a(k) = 1 / (w0 khat^2 + M^2) must stay positive", what, w0);
  FaArgs A{};
  A.phi = phi; A.action_out = action_out; A.pi_in = pi_in; A.pi_out = pi_out; A.dh_out = dh_out; A.accept_out = accept_out;
  A.record = record; A.C = C; A.V = p.V;
  for (int mu = 0, at = 0; mu < 4; ++mu) {
    A.L[mu] = p.L[mu];
    A.toff[mu] = at;
    at += p.L[mu];
  }
  fa_table(p.L, A.table);
  A.w0 = w0; A.w2 = w2; A.w4 = w4; A.m2 = fa_mass_sq; A.steps = steps; A.ax = p.ax;
  A.n_md = n_md; A.n_traj = n_traj; A.record_every = record_every; A.force = force_accept != 0;
  const PhiloxPos kn = philox_pos(seed, NF_PHILOX_KEY_DOMAIN, offset), ka = philox_pos(seed, NF_PHILOX_ACCEPT_DOMAIN, offset);
  A.k0n = kn.k0; A.k1n = kn.k1; A.k0a = ka.k0; A.k1a = ka.k1;
  A.offset = offset;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return dtype == NF_F32 ? dispatch_fa<float>(A, p, s) : dispatch_fa<double>(A, p, s);
}

// nf_sampler_core.h -- what nf_normal_sample (nf_endpoints.hip), nf_mcmc.hip, nf_hmc.hip and nf_hmc_tiled.hip share,
// stated ONCE: Philox4x32-10, a stream position, the normal draw of a group and the accept uniform (the counter layouts
// of include/normflow_hip.h), the HMC accept rule, the replica-exchange rule of the coupling ladders, the draws and the
// bond test of the cluster sweep (nf_cluster.hip), the phi^4 site terms, the entry checks of the HMC kernels and the update lengths of their integration schemes.
#pragma once
#include <cmath>

#include "nf_internal.h"

namespace nf {

// ---------------------------------------------------------------- Philox4x32-10
// Counter-based generator (Salmon et al., SC'11): the four output words of one counter under one key, no state in memory.
__device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
    const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
    c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
}

// fp64 uniform in (0, 1] from 53 bits of two output words: ((ra << 21 ^ rb >> 11) + 1) 2^-53
__device__ __forceinline__ double philox_u53(uint32_t ra, uint32_t rb) {
  const uint64_t a = (uint64_t(ra) << 21) ^ (uint64_t(rb) >> 11);
  return (double(a) + 1.0) * 1.1102230246251565e-16;
}

// Box-Muller on the output words of one Philox call: four standard normals (fp32) or two (fp64), the layout of
// nf_normal_sample (include/normflow_hip.h)
template <typename T>
__device__ __forceinline__ void philox_normals(const uint32_t (&c)[4], T (&z)[sizeof(T) == 4 ? 4 : 2]) {
  if constexpr (sizeof(T) == 4) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const float u1 = (float(c[2 * h] >> 8) + (float(c[2 * h] & 255u) + 1.0f) * 0.00390625f) * 5.9604644775390625e-08f;   // (r + 1) 2^-32, no rounding to 0 or above 1
      const float u2 = float(c[2 * h + 1]) * 2.3283064365386963e-10f;
      const float rho = __builtin_sqrtf(-2.0f * logf(u1 > 1.0f ? 1.0f : u1));
      float sn, cs;
      sincospif(2.0f * u2, &sn, &cs);        // exact range reduction (the argument is in half-turns); the kernel stays near its HBM floor
      z[2 * h] = rho * cs;
      z[2 * h + 1] = rho * sn;
    }
  } else {
    const uint64_t d = (uint64_t(c[2]) << 21) ^ (uint64_t(c[3]) >> 11);
    const double u1 = philox_u53(c[0], c[1]), u2 = double(d) * 1.1102230246251565e-16;
    const double rho = ::sqrt(-2.0 * ::log(u1));
    double sn, cs;
    ::sincos(6.283185307179586 * u2, &sn, &cs);
    z[0] = rho * cs;
    z[1] = rho * sn;
  }
}

// One position of one stream: the key (a seed in a key domain) and the kernel offset, the two high words of every counter.
struct PhiloxPos { uint32_t k0, k1, o0, o1; };

// The one place that folds a domain (NF_PHILOX_*_DOMAIN) into a seed.
inline PhiloxPos philox_pos(uint64_t seed, uint32_t domain, uint64_t offset) {
  return PhiloxPos{uint32_t(seed), uint32_t(seed >> 32) ^ domain, uint32_t(offset), uint32_t(offset >> 32)};
}

// The normals of Philox group g at `pos`: for chain (sample) c of V sites, g = c ngroups + q holds the sites q PER + j
// (PER = 4 in fp32, 2 in fp64; ngroups = ceil(V / PER)).  The draw of nf_normal_sample, whoever makes it.
template <typename T>
__device__ __forceinline__ void philox_normal_group(const PhiloxPos &pos, uint64_t g, T (&z)[sizeof(T) == 4 ? 4 : 2]) {
  uint32_t r[4] = {uint32_t(g), uint32_t(g >> 32), pos.o0, pos.o1};
  philox4x32_10(r, pos.k0, pos.k1);
  philox_normals<T>(r, z);
}

// log u, u in (0, 1], of index i (a chain, or a row of the independence sampler) at `pos`: the accept uniform.
__device__ __forceinline__ double philox_log_uniform(const PhiloxPos &pos, uint64_t i) {
  uint32_t r[4] = {uint32_t(i), uint32_t(i >> 32), pos.o0, pos.o1};
  philox4x32_10(r, pos.k0, pos.k1);
  return ::log(philox_u53(r[0], r[1]));
}

// `pos` moved on by n kernel offsets
inline PhiloxPos philox_pos_after(const PhiloxPos &pos, uint64_t n) {
  const uint64_t off = (uint64_t(pos.o1) << 32 | pos.o0) + n;
  return PhiloxPos{pos.k0, pos.k1, uint32_t(off), uint32_t(off >> 32)};
}

// ---------------------------------------------------------------- the cluster sweep (nf_cluster.hip, include/normflow_hip.h)
// The four output words of index i at `pos`: ONE Philox call under the counter (lo32 i, hi32 i, lo32 offset, hi32 offset).
__device__ __forceinline__ void philox_words(const PhiloxPos &pos, uint64_t i, uint32_t (&r)[4]) {
  r[0] = uint32_t(i); r[1] = uint32_t(i >> 32); r[2] = pos.o0; r[3] = pos.o1;
  philox4x32_10(r, pos.k0, pos.k1);
}

// The bond uniform of one output word: (r + 0.5) 2^-32, in (0, 1) and exact in double
__device__ __forceinline__ double philox_u32_mid(uint32_t r) { return (double(r) + 0.5) * 2.3283064365386963e-10; }

// Is the link between the sites holding a and b active under the uniform u?  t = (w0 a) b left to right in double; a NaN
// or a zero makes no bond, either sign of w0 is legal.
__device__ __forceinline__ bool cluster_bond(double w0, double a, double b, double u) {
  const double t = (w0 * a) * b;
  return t > 0.0 && u < -::expm1(-2.0 * t);
}

// Does the cluster with label rho of chain c flip?  The top bit of word 0 at the sweep's SECOND offset (`flip_pos`), i = c V + rho.
__device__ __forceinline__ bool cluster_flips(const PhiloxPos &flip_pos, uint64_t i) {
  uint32_t r[4];
  philox_words(flip_pos, i, r);
  return (r[0] >> 31) != 0;
}

// the site with the sign bit of v flipped: a NaN flips its sign bit too
__device__ __forceinline__ float flip_sign(float v) { return __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, v) ^ 0x80000000u); }
__device__ __forceinline__ double flip_sign(double v) {
  return __builtin_bit_cast(double, __builtin_bit_cast(uint64_t, v) ^ 0x8000000000000000ull);
}

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
  return v;      // valid in lane 0
}
__device__ __forceinline__ int wave_max_int(int v) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v = max(v, __shfl_down(v, off, kWave));
  return v;
}

// The HMC decision on dh = H1 - H0: a NaN energy difference rejects
__device__ __forceinline__ bool hmc_accepts(double logu, double dh, bool force) { return force || logu < -dh; }

// The replica-exchange decision between the chains a (on rung k) and b (on rung k + 1) of a coupling ladder.  S is linear
// in (w0, w2, w4): S = w2 Q + w4 P - w0 Lam with Q = sum phi^2, P = sum phi^4, Lam = the sum of the links, so
// Delta = [S_k(a) + S_{k+1}(b)] - [S_k(b) + S_{k+1}(a)]; the swap is accepted iff log u < Delta.  d* = rung k minus rung k + 1.
__device__ __forceinline__ double ladder_delta(double dw0, double dw2, double dw4, double dQ, double dP, double dLam) {
  return dw2 * dQ + dw4 * dP - dw0 * dLam;
}

// ---------------------------------------------------------------- phi^4 site terms of the HMC kernels
// F(phi)(x) = 2 w2 phi + 4 w4 phi^3 - w0 nb, nb the sum of the 2 d neighbours
template <typename T> __device__ __forceinline__ T phi4_force(T p, T nb, T w2x2, T w4x4, T w0) {
  return w2x2 * p + w4x4 * p * p * p - w0 * nb;
}

// The site's share of S(phi) = sum (w2 + w4 phi^2) phi^2 - w0 phi sum_mu phi(x - mu), nb_back the sum of the d backward
// neighbours: in double on values cast to double (explicit fma: the arithmetic does not depend on how the compiler contracts)
__device__ __forceinline__ double phi4_site_energy(double p, double nb_back, double w0, double w2, double w4) {
  const double p2 = p * p;
  return __builtin_fma(__builtin_fma(w4, p2, w2), p2, -(w0 * p) * nb_back);
}

// A value every lane of the workgroup holds, moved into scalar registers: a ladder's coefficients come from memory, not
// from the kernel's arguments, and must not cost a vector register each.
__device__ __forceinline__ double uniform_scalar(double v) {
  const uint64_t b = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = __builtin_amdgcn_readfirstlane(uint32_t(b)), hi = __builtin_amdgcn_readfirstlane(uint32_t(b >> 32));
  return __builtin_bit_cast(double, uint64_t(hi) << 32 | lo);
}

// ---------------------------------------------------------------- host side
// The call of nf_phi4_hmc and nf_phi4_hmc_tiled, and the checks the two entry points share.
struct HmcCall {
  void *phi;
  double *action_out;
  const void *pi_in;
  void *pi_out;
  double *dh_out;
  uint8_t *accept_out;
  void *record;
  int record_every;
  int64_t C;
  int n_md, n_traj, force;
  uint64_t seed, offset;
};
inline int hmc_call_checks(const char *what, const HmcCall &K) {
  NF_REQUIRE(K.phi && K.action_out && K.dh_out && K.accept_out, "%s: NULL pointer argument", what);
  NF_REQUIRE(K.C >= 1 && K.C <= 65535, "%s: C (%lld) must be in 1 .. 65535", what, (long long)K.C);
  NF_REQUIRE(K.n_md >= 1 && K.n_traj >= 1 && K.record_every >= 1,
             "%s: n_md (%d), n_traj (%d) and record_every (%d) must be >= 1", what, K.n_md, K.n_traj, K.record_every);
  NF_REQUIRE(!K.pi_in || K.n_traj == 1, "%s: pi_in replaces the momenta of ONE trajectory (n_traj = %d)", what, K.n_traj);
  return NF_OK;
}

// The validity conditions of an integration scheme (include/normflow_hip.h, "integration schemes"), in the order the
// header states them; the message names the broken one.
inline int hmc_scheme_checks(const char *what, const nf_hmc_scheme *sc) {
  NF_REQUIRE(sc != nullptr, "%s: scheme is NULL", what);
  const int s = sc->stages;
  NF_REQUIRE(s >= 1 && s <= NF_HMC_MAX_STAGES, "%s: scheme: stages (%d) must be in 1 .. %d", what, s, NF_HMC_MAX_STAGES);
  double sa = 0.0, sb = 0.0;
  for (int j = 0; j < s; ++j) {
    NF_REQUIRE(std::isfinite(sc->a[j]) && std::isfinite(sc->b[j]), "%s: scheme: weight %d (a = %g, b = %g) is not finite",
               what, j + 1, sc->a[j], sc->b[j]);
    sa += sc->a[j];
    sb += sc->b[j];
  }
  NF_REQUIRE(std::fabs(sa - 1.0) <= 1e-12, "%s: scheme: the drift weights sum to %.17g, not to 1 (sum a)", what, sa);
  NF_REQUIRE(std::fabs(sb - 1.0) <= 1e-12, "%s: scheme: the kick weights sum to %.17g, not to 1 (sum b)", what, sb);
  for (int j = 0; j < s; ++j)
    NF_REQUIRE(std::fabs(sc->a[j] - sc->a[s - 1 - j]) <= 1e-12,
               "%s: scheme: the drift weights are not symmetric (a_%d = %.17g, a_%d = %.17g)", what, j + 1, sc->a[j], s - j,
               sc->a[s - 1 - j]);
  for (int j = 0; j + 1 < s; ++j)
    NF_REQUIRE(std::fabs(sc->b[j] - sc->b[s - 2 - j]) <= 1e-12,
               "%s: scheme: the kick weights are not symmetric (b_%d = %.17g, b_%d = %.17g)", what, j + 1, sc->b[j],
               s - 1 - j, sc->b[s - 2 - j]);
  return NF_OK;
}

// The lengths of a trajectory's updates as the kernels take them: the doubles a_j dt, b_j dt and (b_s / 2) dt, formed here
// and nowhere else (the kernels cast them to the field type), so that the fused and the tiled kernels move by the same
// bits.  Leapfrog: 1 dt and 0.5 dt are exact, the lengths the kernels always took.
struct HmcSteps {
  int stages;
  double drift[NF_HMC_MAX_STAGES], kick[NF_HMC_MAX_STAGES], kick_half;
};
// `sc` NULL: leapfrog.
inline int hmc_steps(const char *what, const nf_hmc_scheme *sc, double dt, HmcSteps &st) {
  st = HmcSteps{};
  if (sc == nullptr) {
    st.stages = 1;
    st.drift[0] = st.kick[0] = dt;
    st.kick_half = 0.5 * dt;
    return NF_OK;
  }
  const int rc = hmc_scheme_checks(what, sc);
  if (rc) return rc;
  st.stages = sc->stages;
  for (int j = 0; j < sc->stages; ++j) {
    st.drift[j] = sc->a[j] * dt;
    st.kick[j] = sc->b[j] * dt;
  }
  st.kick_half = 0.5 * sc->b[sc->stages - 1] * dt;
  return NF_OK;
}

// What the ladder entry points add to them: chain c of the C = K R chains is in replica set c / K.
inline int hmc_ladder_checks(const char *what, const double *coef, int K, const int32_t *rung, int64_t C) {
  NF_REQUIRE(coef != nullptr && rung != nullptr, "%s: coef or rung is NULL", what);
  NF_REQUIRE(K >= 1, "%s: K (%d) must be >= 1", what, K);
  NF_REQUIRE(C % K == 0, "%s: C (%lld) is not a multiple of K (%d)", what, (long long)C, K);
  return NF_OK;
}

}  // namespace nf

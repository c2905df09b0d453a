// nf_cluster_modes_tiled_core.h -- the phase arithmetic and the pass / partial-slot arithmetic of nf_cluster_modes_tiled
// (include/normflow_hip.h, "cluster modes with the chains, the labels and the int64 slots in HBM"), stated ONCE for
// nf_cluster_modes_tiled.hip, so that it also compiles as plain host C++ (tests/cluster_modes_tiled_main.cpp holds it
// against brute-force 64-bit arithmetic under the sanitizers).
// The phase.  j(x) = (sum_mu m_mu x_mu) mod N with m_mu < N <= 2^16 and x_mu < L_mu <= N <= 2^16.  A product m_mu x_mu is
// below 2^32 and exact in unsigned 32-bit arithmetic, the sum of four of them is not: an extent may reach 65536.  So every
// product is reduced mod N BEFORE the axes are added; the four residues add up to less than 4 N <= 2^18 and are reduced
// once more.  The result is the integer that 64-bit arithmetic gives.
// The reduction.  t mod N for any t < 2^32 and 2 <= N <= 2^16 without a division: with M = floor(2^32 / N) (made once on
// the host), q = floor(t M / 2^32) is floor(t / N) or one less, because t (2^32 / N - M) / 2^32 < t / 2^32 < 1; so
// t - q N is in 0 .. 2 N - 1 and one conditional subtraction ends it.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define NF_CMT_FN __host__ __device__ __forceinline__
#else
#define NF_CMT_FN inline
#endif

namespace nf {

constexpr int kCmtMaxPass = 16;                     // quantities per pass
constexpr int kCmtTable = 512;                      // H: entries of the claim-add-flush table

// M = floor(2^32 / N), 2 <= N <= 65536: at most 2^31
NF_CMT_FN uint32_t cmt_magic(uint32_t N) { return uint32_t((uint64_t(1) << 32) / N); }

// t mod N, any t < 2^32, M = cmt_magic(N)
NF_CMT_FN uint32_t cmt_mod(uint32_t t, uint32_t N, uint32_t M) {
  const uint32_t q = uint32_t((uint64_t(t) * M) >> 32);              // one high multiply
  const uint32_t r = t - q * N;                                      // 0 .. 2 N - 1
  return r >= N ? r - N : r;
}

// j(x) of the site with the coordinates x0 .. x3 < 2^16 at the momentum with m0 .. m3 < N
NF_CMT_FN uint32_t cmt_phase(uint32_t m0, uint32_t m1, uint32_t m2, uint32_t m3, uint32_t x0, uint32_t x1, uint32_t x2,
                             uint32_t x3, uint32_t N, uint32_t M) {
  const uint32_t s = cmt_mod(m0 * x0, N, M) + cmt_mod(m1 * x1, N, M) + cmt_mod(m2 * x2, N, M) + cmt_mod(m3 * x3, N, M);
  return cmt_mod(s, N, M);
}

// per_pass in force (0: min(Q, 16)) and the passes; the caller has checked 0 <= per_pass <= min(Q, 16)
NF_CMT_FN int cmt_per_pass(int Q, int per_pass) { return per_pass ? per_pass : (Q < kCmtMaxPass ? Q : kCmtMaxPass); }
NF_CMT_FN int cmt_passes(int Q, int per_pass) { return (Q + per_pass - 1) / per_pass; }
// the quantities of pass number `pass`: first index and count
NF_CMT_FN int cmt_pass_first(int pass, int per_pass) { return pass * per_pass; }
NF_CMT_FN int cmt_pass_count(int Q, int pass, int per_pass) {
  const int left = Q - pass * per_pass;
  return left < per_pass ? left : per_pass;
}
// the place of a sum among the Q + 1 partials of a chain: a^2 at 0, a^4 at 1, quantity q >= 1 at q + 1
NF_CMT_FN int cmt_partial_of(int qid) { return qid ? qid + 1 : 0; }
constexpr int kCmtPartialA4 = 1;
// bytes of the scatter kernel's table for a pass of n quantities
NF_CMT_FN int64_t cmt_lds_bytes(int n) { return int64_t(kCmtTable) * (4 + 8 * int64_t(n)); }

}  // namespace nf

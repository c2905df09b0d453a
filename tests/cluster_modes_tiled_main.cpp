// The phase arithmetic and the pass / partial-slot arithmetic of nf_cluster_modes_tiled
// (normflow__amd/csrc/nf_cluster_modes_tiled_core.h) as a stand-alone host program, against brute-force 64-bit arithmetic
// written from the rule in include/normflow_hip.h ("cluster modes with the chains, the labels and the int64 slots in HBM"):
//   cmt_mod      for every N in 2 .. 65536 at the edges of every range of t and at drawn values of t < 2^32
//   cmt_phase    over ALL sites of every lattice with extents in 1 .. 6 at drawn momenta, and over the corner sites of
//                (65536, 4), (65536,) and (65535, 15) at the corner momenta; on the last N = 65535 is no power of two and
//                sum m x passes 2^32, so a 32-bit sum gives another residue
//   the passes   for every Q in 2 .. 1025 and every legal per_pass: consecutive, complete, no more than per_pass each, and
//                every sum has a place of its own among the Q + 1 partials
// Built and run by tests/test_cluster_modes_tiled_host.py with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdint>
#include <vector>

#include "../normflow__amd/csrc/nf_cluster_modes_core.h"
#include "../normflow__amd/csrc/nf_cluster_modes_tiled_core.h"

namespace {

long long wrong = 0, mods = 0, sites = 0, corners = 0, plans = 0, wrapped = 0, differs32 = 0;
uint64_t state = 0x9e3779b97f4a7c15ull;

uint32_t draw() {                       // splitmix64
  uint64_t z = (state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return uint32_t((z ^ (z >> 31)) >> 16);
}

void expect(bool ok, const char *what, long long a, long long b) {
  if (!ok && wrong++ < 20) std::printf("MISMATCH %s at %lld, %lld\n", what, a, b);
}

void mod_of(uint32_t N) {
  const uint32_t M = nf::cmt_magic(N);
  expect(uint64_t(M) == (uint64_t(1) << 32) / N, "magic", N, M);
  const uint64_t top = (uint64_t(1) << 32) - 1;
  std::vector<uint64_t> ts = {0, 1, uint64_t(N) - 1, N, uint64_t(N) + 1, 2 * uint64_t(N) - 1, 2 * uint64_t(N), 4 * uint64_t(N) - 1,
                              top, top - 1, top - N, top - N + 1, top / N * N, top / N * N - 1, (top / N - 1) * N,
                              uint64_t(N - 1) * (N - 1), uint64_t(65535) * 65535};
  for (int i = 0; i < 48; ++i) ts.push_back((uint64_t(draw()) << 16 ^ draw()) & top);
  for (uint64_t t : ts) {
    if (t > top) continue;
    expect(nf::cmt_mod(uint32_t(t), N, M) == uint32_t(t % N), "mod", N, (long long)t);
    ++mods;
  }
}

// the rule: j(x) = (sum_mu m_mu x_mu) mod N, in 64 bits
uint32_t brute(const uint32_t *m, const uint32_t *x, uint32_t N) {
  uint64_t s = 0;
  for (int mu = 0; mu < 4; ++mu) s += uint64_t(m[mu]) * x[mu];
  if (s >= (uint64_t(1) << 32)) {
    ++wrapped;
    if (uint32_t(s) % N != uint32_t(s % N)) ++differs32;             // what an unsigned 32-bit sum would have given
  }
  return uint32_t(s % N);
}

void site(const int32_t *lat, const uint32_t *m, const uint32_t *x, uint32_t N, uint32_t M, long long &count) {
  for (int mu = 0; mu < 4; ++mu) {
    expect(uint64_t(m[mu]) * x[mu] < (uint64_t(1) << 32), "a product below 2^32", m[mu], x[mu]);
    expect(m[mu] < N && x[mu] < uint32_t(lat[mu]), "m < N, x < L", m[mu], x[mu]);
  }
  expect(nf::cmt_phase(m[0], m[1], m[2], m[3], x[0], x[1], x[2], x[3], N, M) == brute(m, x, N), "phase", x[0], x[3]);
  ++count;
}

void all_sites(const int32_t *lat) {
  const long long N = nf::cm_lcm(lat);
  if (N < 2) return;
  const uint32_t M = nf::cmt_magic(uint32_t(N));
  for (int rep = 0; rep < 4; ++rep) {
    uint32_t m[4], x[4];
    for (int mu = 0; mu < 4; ++mu) m[mu] = uint32_t((draw() % uint32_t(lat[mu])) * (N / lat[mu]));
    for (x[0] = 0; x[0] < uint32_t(lat[0]); ++x[0])
      for (x[1] = 0; x[1] < uint32_t(lat[1]); ++x[1])
        for (x[2] = 0; x[2] < uint32_t(lat[2]); ++x[2])
          for (x[3] = 0; x[3] < uint32_t(lat[3]); ++x[3]) site(lat, m, x, uint32_t(N), M, sites);
  }
}

// 0, 1, 2, L / 2, L - 2, L - 1 of an axis (those below L)
std::vector<uint32_t> edge(int L) {
  std::vector<uint32_t> v;
  for (long long c : {0ll, 1ll, 2ll, 3ll, (long long)L / 2, (long long)L - 2, (long long)L - 1})
    if (c >= 0 && c < L) v.push_back(uint32_t(c));
  return v;
}

void corner_sites(const int32_t *lat) {
  const long long N = nf::cm_lcm(lat);
  const uint32_t M = nf::cmt_magic(uint32_t(N));
  std::vector<uint32_t> e[4];
  for (int mu = 0; mu < 4; ++mu) e[mu] = edge(lat[mu]);
  uint32_t n[4], m[4], x[4];
  for (uint32_t n0 : e[0]) for (uint32_t n1 : e[1]) for (uint32_t n2 : e[2]) for (uint32_t n3 : e[3]) {
    n[0] = n0; n[1] = n1; n[2] = n2; n[3] = n3;
    for (int mu = 0; mu < 4; ++mu) m[mu] = uint32_t(n[mu] * (N / lat[mu]));
    for (uint32_t x0 : e[0]) for (uint32_t x1 : e[1]) for (uint32_t x2 : e[2]) for (uint32_t x3 : e[3]) {
      x[0] = x0; x[1] = x1; x[2] = x2; x[3] = x3;
      site(lat, m, x, uint32_t(N), M, corners);
    }
  }
}

void plan_of(int Q, int per_pass) {
  const int pp = nf::cmt_per_pass(Q, per_pass), passes = nf::cmt_passes(Q, pp);
  expect(pp >= 1 && pp <= nf::kCmtMaxPass && pp <= Q && (per_pass == 0 || pp == per_pass), "per_pass in force", Q, per_pass);
  expect(per_pass != 0 || pp == (Q < 16 ? Q : 16), "per_pass 0 is min(Q, 16)", Q, per_pass);
  expect(passes == (Q + pp - 1) / pp && (passes - 1) * pp < Q && passes * pp >= Q, "passes", Q, per_pass);
  std::vector<int> place(size_t(Q) + 1, 0);                          // the Q + 1 partials of a chain
  int next = 0;
  for (int pass = 0; pass < passes; ++pass) {
    const int q0 = nf::cmt_pass_first(pass, pp), n = nf::cmt_pass_count(Q, pass, pp);
    expect(q0 == next && n >= 1 && n <= pp, "consecutive passes", Q, pass);
    expect(nf::cmt_lds_bytes(n) == 512ll * (4 + 8 * n), "lds", Q, n);
    for (int j = 0; j < n; ++j) {
      const int at = nf::cmt_partial_of(q0 + j);
      expect(at >= 0 && at <= Q, "a partial inside the chain's", Q, q0 + j);
      if (at >= 0 && at <= Q) ++place[size_t(at)];
      if (q0 + j == 0) ++place[size_t(nf::kCmtPartialA4)];
    }
    next = q0 + n;
  }
  expect(next == Q, "complete", Q, per_pass);
  for (int at = 0; at <= Q; ++at) expect(place[size_t(at)] == 1, "every partial written once", Q, at);
  ++plans;
}

}  // namespace

int main() {
  for (uint32_t N = 2; N <= 65536; ++N) mod_of(N);
  long long lattices = 0;
  int32_t lat[4];
  for (lat[0] = 1; lat[0] <= 6; ++lat[0])
    for (lat[1] = 1; lat[1] <= 6; ++lat[1])
      for (lat[2] = 1; lat[2] <= 6; ++lat[2])
        for (lat[3] = 1; lat[3] <= 6; ++lat[3], ++lattices) all_sites(lat);
  const int32_t big[3][4] = {{1, 1, 65536, 4}, {1, 1, 1, 65536}, {1, 1, 65535, 15}};
  for (const auto &b : big) corner_sites(b);
  {                                     // the case of the tests: m = (65535, 49152) at x = (65535, 3) on (65536, 4)
    const uint32_t m[4] = {0, 0, 65535, 49152}, x[4] = {0, 0, 65535, 3};
    expect(uint64_t(m[2]) * x[2] + uint64_t(m[3]) * x[3] == 4294983681ull, "the sum of the case", 0, 0);
    site(big[0], m, x, 65536, nf::cmt_magic(65536), corners);
  }
  for (int Q = 2; Q <= 1025; ++Q)
    for (int pp = 0; pp <= (Q < 16 ? Q : 16); ++pp) plan_of(Q, pp);
  expect(wrapped > 0 && differs32 > 0, "sums above 2^32 were met, and some where 32 bits give another residue", wrapped, differs32);
  std::printf("mods = %lld lattices = %lld sites = %lld corners = %lld above 2^32 = %lld (32-bit differs: %lld) plans = %lld wrong = %lld\n",
              mods, lattices, sites, corners, wrapped, differs32, plans, wrong);
  std::printf(wrong ? "FAIL\n" : "PASS\n");
  return wrong ? 1 : 0;
}

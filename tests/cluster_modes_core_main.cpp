// The momenta and the quantity table of the cluster modes (normflow__amd/csrc/nf_cluster_modes_core.h) as a stand-alone
// host program: cm_lcm, cm_reduce, cm_self_conjugate, cm_describe, cm_check and cm_row_ok against a brute-force enumeration
// written from the rule in include/normflow_hip.h ("cluster modes"), for every lattice with extents in 1 .. 6 and lists
// drawn from a fixed generator, with every single-field corruption of a table refused.  Built and run by
// tests/test_cluster_modes_host.py with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdint>
#include <vector>

#include "../normflow__amd/csrc/nf_cluster_modes_core.h"

namespace {

long long wrong = 0, tables = 0, rows_checked = 0, corrupted = 0;
uint64_t state = 0x9e3779b97f4a7c15ull;

uint32_t draw() {                       // splitmix64
  uint64_t z = (state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return uint32_t((z ^ (z >> 31)) >> 16);
}

void expect(bool ok, const char *what, const int32_t *lat, int p) {
  if (!ok && wrong++ < 20) std::printf("MISMATCH %s: lattice (%d, %d, %d, %d) at %d\n", what, lat[0], lat[1], lat[2], lat[3], p);
}

void one(const int32_t *lat, int P) {
  // the rule, enumerated
  long long N = 1;
  for (int mu = 0; mu < 4; ++mu) {
    long long a = N, b = lat[mu];
    while (b) { const long long t = a % b; a = b; b = t; }
    N = N / a * lat[mu];
  }
  expect(nf::cm_lcm(lat) == N, "lcm", lat, 0);
  std::vector<int32_t> modes(size_t(4 * P));
  for (int p = 0; p < P; ++p)
    for (int mu = 0; mu < 4; ++mu) {
      const int L = lat[mu];
      int n = L == 1 ? 0 : int(draw() % uint32_t(4 * L)) - 2 * L;       // negative components too
      if (L > 1 && draw() % 4 == 0) n = (L % 2 == 0 && draw() % 2) ? L / 2 : 0;     // the self-conjugate values
      modes[size_t(4 * p + mu)] = n;
    }
  std::vector<std::vector<int>> want;
  for (int p = 0; p < P; ++p) {
    int n[4], m[4];
    bool sc = true;
    for (int mu = 0; mu < 4; ++mu) {
      n[mu] = ((modes[size_t(4 * p + mu)] % lat[mu]) + lat[mu]) % lat[mu];
      expect(nf::cm_reduce(modes[size_t(4 * p + mu)], lat[mu]) == n[mu] && n[mu] >= 0 && n[mu] < lat[mu], "reduce", lat, p);
      m[mu] = int(n[mu] * (N / lat[mu]));
      if ((2 * n[mu]) % lat[mu] != 0) sc = false;
    }
    expect(nf::cm_self_conjugate(n, lat) == (sc ? 1 : 0), "self-conjugate", lat, p);
    want.push_back({m[0], m[1], m[2], m[3], 0, 2 + p, sc ? 1 : 0, p});
    if (!sc) want.push_back({m[0], m[1], m[2], m[3], 1, 2 + p, 0, p});
  }
  std::vector<int32_t> desc(size_t(8 * (1 + 2 * P)), -7);
  int Q = -1, Nout = -1, bad = -1;
  const int e = nf::cm_describe(lat, modes.data(), P, desc.data(), &Q, &Nout, &bad);
  if (N == 1) {
    expect(e == nf::kCmNoAxis, "N = 1 is refused", lat, 0);
    return;
  }
  expect(e == nf::kCmOk && Q == 1 + int(want.size()) && Nout == int(N), "Q and N", lat, P);
  if (e != nf::kCmOk || Q != 1 + int(want.size())) return;
  int Q2 = -1, N2 = -1;
  expect(nf::cm_describe(lat, modes.data(), P, nullptr, &Q2, &N2, &bad) == nf::kCmOk && Q2 == Q && N2 == Nout, "count only", lat, P);
  for (int f = 0; f < 8; ++f) expect(desc[size_t(f)] == (f == 7 ? 2 + P : 0), "row 0", lat, f);
  for (int q = 1; q < Q; ++q) {
    for (int f = 0; f < 8; ++f) expect(desc[size_t(8 * q + f)] == want[size_t(q - 1)][size_t(f)], "row", lat, q);
    // m_mu x_mu summed over the axes stays below 2^32
    unsigned long long top = 0;
    for (int mu = 0; mu < 4; ++mu) top += (unsigned long long)desc[size_t(8 * q + mu)] * (unsigned long long)(lat[mu] - 1);
    expect(top < (1ull << 32), "phase sum", lat, q);
    ++rows_checked;
  }
  expect(nf::cm_check(lat, desc.data(), Q, Nout, &bad) == nf::kCmOk, "check accepts", lat, bad);
  for (int q = 0; q < Q; ++q) expect(nf::cm_row_ok(desc.data(), q, Q, Nout, 2 + P) == 1, "row_ok accepts", lat, q);
  ++tables;
  // every single-field corruption is refused by cm_check; those that could reach memory also by cm_row_ok
  for (int q = 0; q < Q; ++q)
    for (int f = 0; f < 8; ++f) {
      const int32_t keep = desc[size_t(8 * q + f)];
      const int32_t tries[3] = {keep + 1, -1, int32_t(Nout + 5 + P)};
      for (int32_t v : tries) {
        if (v == keep) continue;
        if (f < 4 && v == keep + 1 && Nout == 2) continue;       // extents 1 and 2 only: m + 1 is another momentum's
        desc[size_t(8 * q + f)] = v;
        expect(nf::cm_check(lat, desc.data(), Q, Nout, &bad) != nf::kCmOk, "check refuses", lat, 8 * q + f);
        const bool memory = q > 0 && ((f < 4 && (v < 0 || v >= Nout)) || (f == 5 && (v < 2 || v >= 2 + P)) || (f == 4 && v != 0 && v != 1));
        if (memory) {
          int ok = 1;
          for (int r = 0; r < Q; ++r) ok &= nf::cm_row_ok(desc.data(), r, Q, Nout, desc[7]);
          expect(ok == 0, "row_ok refuses", lat, 8 * q + f);
        }
        ++corrupted;
      }
      desc[size_t(8 * q + f)] = keep;
    }
  expect(nf::cm_check(lat, desc.data(), Q - 1 < 2 ? 1 : Q - 1, Nout, &bad) != nf::kCmOk || Q - 1 < 2, "a short table", lat, Q);
  expect(nf::cm_check(lat, desc.data(), Q, Nout + 1, &bad) != nf::kCmOk, "another N", lat, Q);
}

}  // namespace

int main() {
  long long lattices = 0;
  int32_t lat[4];
  for (lat[0] = 1; lat[0] <= 6; ++lat[0])
    for (lat[1] = 1; lat[1] <= 6; ++lat[1])
      for (lat[2] = 1; lat[2] <= 6; ++lat[2])
        for (lat[3] = 1; lat[3] <= 6; ++lat[3]) {
          for (int P = 1; P <= 5; ++P) one(lat, P);
          ++lattices;
        }
  // the limits: P, an axis of extent 1, a large lcm
  const int32_t big[4] = {1, 251, 256, 257}, unit[4] = {1, 1, 4, 4}, ok[4] = {1, 1, 256, 255};
  std::vector<int32_t> many(size_t(4 * 513), 0);
  int Q, N, bad;
  int32_t m1[4] = {0, 1, 0, 0};
  if (nf::cm_describe(big, many.data(), 1, nullptr, &Q, &N, &bad) != nf::kCmLargeN) { ++wrong; std::printf("MISMATCH large N\n"); }
  if (nf::cm_describe(ok, many.data(), 1, nullptr, &Q, &N, &bad) != nf::kCmOk || N != 65280 || Q != 2) { ++wrong; std::printf("MISMATCH N = 65280\n"); }
  if (nf::cm_describe(unit, many.data(), 0, nullptr, &Q, &N, &bad) != nf::kCmCount) { ++wrong; std::printf("MISMATCH P = 0\n"); }
  if (nf::cm_describe(unit, many.data(), 513, nullptr, &Q, &N, &bad) != nf::kCmCount) { ++wrong; std::printf("MISMATCH P = 513\n"); }
  if (nf::cm_describe(unit, many.data(), 512, nullptr, &Q, &N, &bad) != nf::kCmOk || Q != 513) { ++wrong; std::printf("MISMATCH P = 512\n"); }
  if (nf::cm_describe(unit, m1, 1, nullptr, &Q, &N, &bad) != nf::kCmUnitAxis) { ++wrong; std::printf("MISMATCH unit axis\n"); }
  std::printf("lattices = %lld tables = %lld rows = %lld corruptions = %lld wrong = %lld\n", lattices, tables, rows_checked, corrupted, wrong);
  std::printf(wrong == 0 ? "PASS\n" : "FAIL\n");
  return wrong == 0 ? 0 : 1;
}

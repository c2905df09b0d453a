// nf_cluster_modes_core.h -- the momenta and the quantity table of the cluster modes (include/normflow_hip.h, "cluster
// modes"), stated ONCE for nf_cluster_modes.hip, so that it also compiles as plain host C++
// (tests/cluster_modes_core_main.cpp holds it against a brute-force enumeration under the sanitizers).
//   N        the lcm of the extents > 1 (1 if there is none: refused by the callers; above 65536: refused too)
//   n mod L  every component reduced to 0 .. L_mu - 1; m_mu = (n_mu mod L_mu) (N / L_mu), so that the phase index of a site
//            is j(x) = (sum_mu m_mu x_mu) mod N
//   self-conjugate: 2 n_mu = 0 mod L_mu on every axis; such a momentum has an R and no I
// The quantities, in order: A (index 0), then per momentum in list order R, I; R alone for a self-conjugate momentum.
// Q = 1 + sum_n (2 - [n self-conjugate]); the row has 2 + P columns: sum a^2, sum a^4, then one per momentum.
// The table `desc` is (Q, 8) int32, row = quantity:
//   [0 .. 3]  m_0 .. m_3                  (row 0: 0)
//   [4]       component: 0 = R, 1 = I     (row 0: 0)
//   [5]       column of the quantity's momentum, 2 + its place in the list       (row 0: 0)
//   [6]       1 for an R without an I (self-conjugate), else 0                   (row 0: 0)
//   [7]       the momentum's place in the list, 0 .. P - 1                       (row 0: the row length 2 + P)
// On the lattices of the kernel m_mu < 2^16 and x_mu < 2^14: sum_mu m_mu x_mu < 2^32, unsigned 32-bit arithmetic is exact.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define NF_CM_FN __host__ __device__ __forceinline__
#else
#define NF_CM_FN inline
#endif

namespace nf {

constexpr int kCmMaxModes = 512;                    // P
constexpr int kCmMaxN = 65536;                      // N
constexpr int kCmRow = 8;                           // int32 per row of desc
enum { kCmM = 0, kCmComp = 4, kCmCol = 5, kCmROnly = 6, kCmMode = 7 };

// why a momentum list or a table is refused
enum CmError {
  kCmOk = 0,
  kCmNoAxis,          // every extent is 1: N = 1
  kCmLargeN,          // N > 65536
  kCmCount,           // P outside 1 .. 512
  kCmUnitAxis,        // a non-zero component on an axis of extent 1
  kCmQuantities,      // Q outside 2 .. 1 + 2 x 512, or not the table's
  kCmRowZero,         // row 0 is not (0, 0, 0, 0, 0, 0, 0, 2 + P)
  kCmM_,              // an m_mu outside 0 .. N - 1 or no multiple of N / L_mu
  kCmComponent,       // a component outside {0, 1}, or an I that does not follow its R
  kCmColumn,          // a column outside 2 .. 1 + P or out of order
  kCmConjugate,       // the "R without I" flag is not the momentum's
};

NF_CM_FN long long cm_gcd(long long a, long long b) {
  while (b) {
    const long long t = a % b;
    a = b;
    b = t;
  }
  return a;
}

// the lcm of the extents > 1; stops growing once it is above 65536 (any such value is refused)
NF_CM_FN long long cm_lcm(const int32_t *lattice) {
  long long N = 1;
  for (int mu = 0; mu < 4; ++mu) {
    const long long L = lattice[mu];
    if (L > 1 && N <= kCmMaxN) N = N / cm_gcd(N, L) * L;
  }
  return N;
}

NF_CM_FN int cm_reduce(long long n, int L) {
  const long long r = n % L;
  return int(r < 0 ? r + L : r);
}

// n[4] reduced, lattice[4]
NF_CM_FN int cm_self_conjugate(const int *n, const int32_t *lattice) {
  for (int mu = 0; mu < 4; ++mu)
    if ((2 * (long long)n[mu]) % lattice[mu] != 0) return 0;
  return 1;
}

// Q of a list of P momenta modes (P, 4) on lattice[4] (extents >= 1), N and -- where desc is not NULL -- the 1 + 2 P rows
// at most of the table.  Returns a CmError; *bad is the place in the list of the momentum that caused it.
NF_CM_FN int cm_describe(const int32_t *lattice, const int32_t *modes, int P, int32_t *desc, int *Q, int *N, int *bad) {
  *Q = 0;
  *N = 0;
  *bad = 0;
  const long long lcm = cm_lcm(lattice);
  if (lcm == 1) return kCmNoAxis;
  if (lcm > kCmMaxN) return kCmLargeN;
  if (P < 1 || P > kCmMaxModes) return kCmCount;
  *N = int(lcm);
  int q = 1;
  if (desc) {
    for (int f = 0; f < kCmRow; ++f) desc[f] = 0;
    desc[kCmMode] = 2 + P;
  }
  for (int p = 0; p < P; ++p) {
    int n[4];
    for (int mu = 0; mu < 4; ++mu) {
      if (lattice[mu] == 1 && modes[4 * p + mu] != 0) {
        *bad = p;
        return kCmUnitAxis;
      }
      n[mu] = cm_reduce(modes[4 * p + mu], lattice[mu]);
    }
    const int sc = cm_self_conjugate(n, lattice);
    for (int comp = 0; comp < (sc ? 1 : 2); ++comp, ++q) {
      if (!desc) continue;
      int32_t *row = desc + size_t(q) * kCmRow;
      for (int mu = 0; mu < 4; ++mu) row[kCmM + mu] = int32_t(n[mu] * (lcm / lattice[mu]));
      row[kCmComp] = comp;
      row[kCmCol] = 2 + p;
      row[kCmROnly] = sc;
      row[kCmMode] = p;
    }
  }
  *Q = q;
  return kCmOk;
}

// A table (Q, 8) against the rule: kCmOk iff it is what cm_describe gives for SOME list of momenta on lattice[4] with this
// N.  *bad is the row that failed.
NF_CM_FN int cm_check(const int32_t *lattice, const int32_t *desc, int Q, int N, int *bad) {
  *bad = 0;
  const long long lcm = cm_lcm(lattice);
  if (lcm == 1) return kCmNoAxis;
  if (lcm > kCmMaxN || N != int(lcm)) return kCmLargeN;
  if (Q < 2 || Q > 1 + 2 * kCmMaxModes) return kCmQuantities;
  for (int f = 0; f < kCmMode; ++f)
    if (desc[f] != 0) return kCmRowZero;
  const int P = desc[kCmMode] - 2;
  if (P < 1 || P > kCmMaxModes) return kCmRowZero;
  int p = 0, q = 1;
  while (q < Q) {
    const int32_t *row = desc + size_t(q) * kCmRow;
    *bad = q;
    int n[4];
    for (int mu = 0; mu < 4; ++mu) {
      const int m = row[kCmM + mu], scale = N / lattice[mu];
      if (lattice[mu] == 1 && m != 0) return kCmUnitAxis;
      if (m < 0 || m >= N || m % scale != 0) return kCmM_;
      n[mu] = m / scale;
    }
    if (row[kCmComp] != 0) return kCmComponent;
    if (p >= P || row[kCmCol] != 2 + p || row[kCmMode] != p) return kCmColumn;
    const int sc = cm_self_conjugate(n, lattice);
    if (row[kCmROnly] != sc) return kCmConjugate;
    ++q;
    if (!sc) {                                        // the I of the same momentum follows
      if (q >= Q) return kCmQuantities;
      const int32_t *im = row + kCmRow;
      *bad = q;
      for (int mu = 0; mu < 4; ++mu)
        if (im[kCmM + mu] != row[kCmM + mu]) return kCmM_;
      if (im[kCmComp] != 1) return kCmComponent;
      if (im[kCmCol] != 2 + p || im[kCmMode] != p) return kCmColumn;
      if (im[kCmROnly] != 0) return kCmConjugate;
      ++q;
    }
    ++p;
  }
  *bad = 0;
  if (p != P) return kCmRowZero;
  return kCmOk;
}

// What a kernel holds a row to before it uses it, from the fields alone: everything that is indexed with is in range and
// an I follows its R.  ncols = 2 + P of row 0.  (cm_check is the full rule; this is its part that guards memory.)
NF_CM_FN int cm_row_ok(const int32_t *desc, int q, int Q, int N, int ncols) {
  const int32_t *row = desc + size_t(q) * kCmRow;
  if (q == 0) return ncols >= 3 && ncols <= 1 + Q && ncols <= 2 + kCmMaxModes;
  for (int mu = 0; mu < 4; ++mu)
    if (row[kCmM + mu] < 0 || row[kCmM + mu] >= N) return 0;
  if (row[kCmCol] < 2 || row[kCmCol] >= ncols) return 0;
  if (row[kCmComp] == 0) return row[kCmROnly] == 1 || (row[kCmROnly] == 0 && q + 1 < Q && row[kCmRow + kCmComp] == 1);
  if (row[kCmComp] != 1 || q < 2) return 0;
  const int32_t *re = row - kCmRow;
  return re[kCmComp] == 0 && re[kCmROnly] == 0 && re[kCmCol] == row[kCmCol];
}

}  // namespace nf

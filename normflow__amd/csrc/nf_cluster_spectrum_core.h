// nf_cluster_spectrum_core.h -- the quantities of the cluster spectrum (include/normflow_hip.h, "cluster spectrum"), stated
// ONCE for nf_cluster_spectrum.hip and nf_cluster_spectrum_tiled.hip, so that it also compiles as plain host C++
// (tests/cluster_spectrum_core_main.cpp holds every descriptor against a brute-force enumeration under the sanitizers).
// The quantities, in order: A (index 0), then per axis in order and per k = 1 .. K_mu ascending R, I; R alone at the
// Nyquist momentum 2 k = L_mu.  Q = 1 + sum_mu (2 K_mu - [2 K_mu = L_mu]); the row has 2 + sum_mu K_mu columns: sum a^2,
// sum a^4, then one per (mu, k), none for an axis of extent 1.
//   cs_layout     K_mu from kmax, and per axis the site stride, the extent, the offset of its rows in the twiddle table, and
//                 the PREFIX COUNTS: qpre[mu] quantities after A and cpre[mu] columns after the two of A in front of axis mu
//   cs_quantity   index qid >= 1 -> axis, k, component, column, Nyquist, by integer arithmetic on qid and the prefix
//                 counts; the per-axis fields are picked by selects on the axis number (constant indices), so that in a
//                 kernel nothing in registers is indexed dynamically.  With a wave-uniform qid all of it is wave-uniform.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define NF_CS_FN __host__ __device__ __forceinline__
#else
#define NF_CS_FN inline
#endif

namespace nf {

struct CsLayout {
  int K[4], stride[4], extent[4], off[4];
  int qpre[4];                   // quantities (after A) in front of axis mu
  int cpre[4];                   // columns (after the two of A) in front of axis mu
  int nq, ncols;                 // Q, and 2 + sum K_mu
};

// lattice[4] with extents >= 1 and V = their product (< 2^31); kmax >= 0, 0: all momenta
NF_CS_FN void cs_layout(const int32_t *lattice, int kmax, long long V, CsLayout &p) {
  int stride = int(V), off = 0, nq = 0, nc = 0;
  for (int mu = 0; mu < 4; ++mu) {
    const int L = lattice[mu];
    stride /= L;
    const int K = L == 1 ? 0 : (kmax == 0 || kmax > L / 2 ? L / 2 : kmax);
    p.K[mu] = K;
    p.stride[mu] = stride;
    p.extent[mu] = L;
    p.off[mu] = off;
    p.qpre[mu] = nq;
    p.cpre[mu] = nc;
    nq += 2 * K - (K > 0 && 2 * K == L ? 1 : 0);
    nc += K;
    off += L;
  }
  p.nq = 1 + nq;
  p.ncols = 2 + nc;
}

// the descriptor of quantity qid >= 1: the axis is the last whose prefix count is <= qid - 1 (an axis without quantities
// shares its prefix with the next one that has some, and the comparisons step over it)
struct CsQuantity {
  int stride, extent, off, k, comp, col;
  int axis, nyquist;             // nyquist: 2 k = L_mu, the quantity is an R without an I
};

// A: anything with the per-axis arrays stride, extent, off, qpre and cpre of cs_layout (a kernel's argument struct)
template <class A>
NF_CS_FN CsQuantity cs_quantity(const A &a, int qid) {
  const int r = qid - 1;
  const int mu = (r >= a.qpre[1] ? 1 : 0) + (r >= a.qpre[2] ? 1 : 0) + (r >= a.qpre[3] ? 1 : 0);
#define NF_CS_PICK(f) (mu == 1 ? a.f[1] : mu == 2 ? a.f[2] : mu == 3 ? a.f[3] : a.f[0])
  CsQuantity d{NF_CS_PICK(stride), NF_CS_PICK(extent), NF_CS_PICK(off), 0, 0, NF_CS_PICK(cpre), mu, 0};
  const int pre = NF_CS_PICK(qpre);
#undef NF_CS_PICK
  const int local = r - pre;
  d.k = (local >> 1) + 1;
  d.comp = local & 1;
  d.col += 2 + (local >> 1);
  d.nyquist = 2 * d.k == d.extent ? 1 : 0;
  return d;
}

}  // namespace nf

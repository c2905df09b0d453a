// nf_cluster_union.h -- the lock-free union of nf_cluster_tiled.hip's merge phase, stated ONCE so that it also compiles
// as plain host C++ (tests/cluster_union_main.cpp runs it on std::atomic<int> from several threads under the sanitizers).
// `lab` is a forest over the sites 0 .. V - 1 of one chain, lab[z] = the parent of z, a root labels itself.  Invariants,
// those of nf_cluster.hip: lab[z] <= z, lab[z] is a site of z's cluster, and a label only ever decreases.
// Memory is reached through two wrappers of the policy A alone:
//   A::load(p)          a relaxed atomic load
//   A::fetch_min(p, v)  a relaxed atomic minimum that returns the value it found
// A stale load shows an older, larger, still valid label; the value fetch_min returns is the truth of that moment.
//   uf_root    follows lab from x to a site that labels itself.  The chain of labels strictly decreases (lab[z] <= z and
//              the walk stops at lab[z] == z), so it ends within V - 1 steps; the bound `V` is there so that a bug cannot
//              become a hang.  It writes nothing: while unions run, a site may only be lowered by the lane that goes on
//              to join what the old label led to (uf_unite below).  Lowering a path to the root found ("compression") from
//              here would cut the one edge that a finished union left between two trees.
//   uf_unite   joins the trees of a and b.  With the roots ordered hi > lo: old = fetch_min(&lab[hi], lo).  old == hi: hi
//              was a root and now hangs under lo, done.  Otherwise another lane hooked hi first, under old < hi; lab[hi]
//              is now min(old, lo), both of the cluster, and what is left to join is the pair (root of old, root of lo).
//              Bound of the loop: both members of the new pair are below hi (old < hi, lo < hi, a root is at most its
//              start), so hi strictly decreases from at most V - 1 and stays >= 1 while the roots differ: AT MOST V - 1
//              ATOMICS per call, whatever the other lanes do.  No lane waits for another: no spin, no flag, no ticket.
// Both return false when a bound was hit (it cannot happen).
#pragma once

#if defined(__HIPCC__)
#define NF_UF_FN __device__ __forceinline__
#else
#define NF_UF_FN inline
#endif

namespace nf {

template <class A>
NF_UF_FN bool uf_root(typename A::cell *lab, int x, int V, int &root) {
  int l = x, n = A::load(&lab[l]);
  for (int step = 0; n != l; ++step) {
    if (step >= V) {
      root = l;
      return false;
    }
    l = n;
    n = A::load(&lab[l]);
  }
  root = l;
  return true;
}

template <class A>
NF_UF_FN bool uf_unite(typename A::cell *lab, int a, int b, int V) {
  int ra, rb;
  if (!uf_root<A>(lab, a, V, ra) || !uf_root<A>(lab, b, V, rb)) return false;
  for (int it = 0; it < V; ++it) {
    if (ra == rb) return true;
    const int hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
    const int old = A::fetch_min(&lab[hi], lo);
    if (old == hi) return true;
    if (!uf_root<A>(lab, old, V, ra) || !uf_root<A>(lab, lo, V, rb)) return false;
  }
  return false;
}

}  // namespace nf

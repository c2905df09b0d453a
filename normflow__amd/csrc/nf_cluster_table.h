// nf_cluster_table.h -- the claim-add-flush table of nf_cluster_moments_tiled.hip's scatter kernel, stated ONCE so that it
// also compiles as plain host C++ (tests/cluster_moments_table_main.cpp runs it on std::atomic from several threads under
// the sanitizers).  A workgroup sums on chip what its sites add to the int64 slots of their labels, and sends ONE add per
// (label, quantity) to the slot arrays in HBM: adds to one HBM word from all over the chip go one after the other, and in
// the ordered phase one label holds most of the lattice.
// The table is direct-mapped: H entries (a power of two), entry h = label & (H - 1); keys[h] is -1 (free) or the label
// that claimed the entry, sums[j H + h] the entry's sum of quantity j.  Memory is reached through the policy A alone:
//   A::claim(p, label)   an atomic compare-and-swap of *p from -1 to label that returns the value it found
//   A::load(p)           a relaxed load of a key
//   A::add_table(p, v)   a relaxed 64-bit integer add to a sum of the table
//   A::read_table(p)     a relaxed load of a sum of the table
//   A::add_out(p, v)     a relaxed 64-bit integer add to a slot outside the table, nothing returned
// The steps, with a barrier of the table's users between them:
//   table_clear   keys = -1, sums = 0
//   table_claim   the entry of `label` if it is free or already the label's, else -1: the entry belongs to another label
//   table_add     v to the entry's sum of quantity j, or, without an entry, straight to out[label]
//   table_flush   every claimed entry sends its non-zero sums to out_j[key]
// The sums are integers: which labels hit, which miss and the order of the flush cannot change a bit of the slots, only
// the number of adds that leave the table.  Nothing waits for anything: no spin, no lock.
#pragma once

#if defined(__HIPCC__)
#define NF_CT_FN __device__ __forceinline__
#else
#define NF_CT_FN inline
#endif

namespace nf {

template <class A>
NF_CT_FN void table_clear(typename A::key *keys, typename A::sum *sums, int H, int nq, int tid, int nt) {
  for (int e = tid; e < H; e += nt) A::init_key(&keys[e]);
  for (int e = tid; e < nq * H; e += nt) A::init_sum(&sums[e]);
}

template <class A>
NF_CT_FN int table_claim(typename A::key *keys, int H, int label) {
  const int h = label & (H - 1);
  const int found = A::claim(&keys[h], label);
  return found == -1 || found == label ? h : -1;
}

template <class A>
NF_CT_FN void table_add(typename A::sum *sums, int H, int h, int j, typename A::sum *out, int label, long long v) {
  if (v == 0) return;
  if (h >= 0)
    A::add_table(&sums[j * H + h], static_cast<unsigned long long>(v));
  else
    A::add_out(&out[label], static_cast<unsigned long long>(v));
}

// out_j = out + j * out_stride: the slot array of quantity j
template <class A>
NF_CT_FN void table_flush(typename A::key *keys, typename A::sum *sums, int H, int nq, typename A::sum *out,
                          long long out_stride, int tid, int nt) {
  for (int e = tid; e < H; e += nt) {
    const int key = A::load(&keys[e]);
    if (key < 0) continue;
    for (int j = 0; j < nq; ++j) {
      const unsigned long long v = A::read_table(&sums[j * H + e]);
      if (v) A::add_out(&out[j * out_stride + key], v);
    }
  }
}

}  // namespace nf

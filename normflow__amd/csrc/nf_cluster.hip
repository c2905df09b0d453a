// nf_cluster.hip -- one Swendsen-Wang sweep of the embedded Ising signs of phi^4 chains (Brower-Tamayo; MI355X-side
// extension, no counterpart in the reference).  phi = s |phi|: between the sites x and y = x + mu the bond is active with
// probability 1 - exp(-2 t), t = w0 phi(x) phi(y) > 0; the connected components of the active links are the clusters, and
// every cluster flips its sign with probability 1/2.  The rule, its Philox draws and the label convention are stated in
// include/normflow_hip.h; the draws and the bond test are nf_sampler_core.h's.
// One workgroup per chain, for the lattices of nf_phi4_hmc (V sizeof(T) <= 64 KiB), with that kernel's lane map: lane
// `tid` of the NT lanes owns the sites tid + k NT (k < NS) and keeps their phi in registers.  LDS holds one int32 label and
// one byte per site (bits 0 .. 3: the forward link along axis mu is active; bits 4 .. 7: x_mu is the last site of its axis,
// so the forward neighbour wraps).  Labelling is label equivalence with hooking and pointer jumping:
//   a round = for every active forward link (x, y) with lab[x] != lab[y]: lo = the smaller, hi = the larger label;
//             ds_min lab[the site that held hi] <- lo (the label travels the link) and ds_min lab[hi] <- lo (hi's whole
//             tree follows) | barrier | every site chases lab[lab[..]] to a site that labels itself | barrier.
// Invariants: lab[x] <= x, lab[x] is a site of x's cluster, and a label only ever decreases.  So the chase ends (the chain
// of labels strictly decreases), a round in which no link saw two labels is a fixed point, and the fixed point is unique:
// labels constant on a cluster, equal to a site of it that labels itself, below every site of it -- the smallest site
// index, whatever the schedule of the lanes was.  After r rounds lab[x] is at most the smallest index within r links of
// x (the first ds_min alone gives that), so V - 1 rounds reach the fixed point and round V sees it: the loop runs at most
// V rounds, and a chain that has not settled then is left untouched with rounds = -1 (it cannot happen; the bound is there
// so that a bug cannot become a hang).  Every barrier is in uniform control flow: the loop's exit is a flag in LDS that
// every lane reads between the same two barriers.
// Then the labels go to registers, the label array is reused for the clusters' sizes (integer ds_add), and every site takes
// its cluster's flip bit and, where set, stores phi back with the sign bit flipped: plain vector stores, nothing else of
// phi is written.  Integer atomics on LDS only: the same inputs give the same bits.
// nf_phi4_cluster_ladder is the same kernel compiled with LADDER, as nf_hmc.hip's: the workgroup of chain c takes w0 from
// row rung[c] of the ladder's table, once, into scalar registers, and writes its stats at the rung-ordered row
// (c / K) K + rung[c]; phi, the labels and the Philox indices stay at c.  A chain on rung k has nf_phi4_cluster's bits at w0_k.
#include <type_traits>

#include "nf_sampler_core.h"

namespace nf {

constexpr int kClMaxLanes = 1024;
constexpr size_t kClScratchBytes = 256;            // the loop's two flags and the three sums, in front of the labels

struct ClusterPlan {
  int64_t V;
  int L[4];            // the caller's extents
  int ns, nt;          // nf_phi4_hmc's lane map: sites per lane and lanes per chain
  size_t lab_bytes;    // 4 V, rounded up to 16
  size_t lds;          // kClScratchBytes + lab_bytes + V rounded up to 16
};

static int cluster_plan(const char *what, const int32_t *lattice, int dtype, ClusterPlan &p) {
  NF_REQUIRE(lattice != nullptr, "%s: lattice is NULL", what);
  NF_REQUIRE(dtype == NF_F32 || dtype == NF_F64, "%s: unsupported dtype %d", what, dtype);
  for (int mu = 0; mu < 4; ++mu) {
    NF_REQUIRE(lattice[mu] >= 1, "%s: lattice extents must be >= 1", what);
    p.L[mu] = lattice[mu];
  }
  nf_hmc_plan hp;
  if (nf_phi4_hmc_plan(lattice, dtype, &hp) != NF_OK) {
    set_error("%s: a chain of the lattice (%d, %d, %d, %d) is outside the class of nf_phi4_hmc (V sizeof <= 64 KiB), which is "
              "the class of the cluster kernel", what, lattice[0], lattice[1], lattice[2], lattice[3]);
    return NF_EINVAL;
  }
  p.V = int64_t(lattice[0]) * lattice[1] * lattice[2] * lattice[3];
  p.ns = hp.sites_per_lane;
  p.nt = hp.lanes;
  p.lab_bytes = (size_t(p.V) * 4 + 15) & ~size_t(15);
  p.lds = kClScratchBytes + p.lab_bytes + ((size_t(p.V) + 15) & ~size_t(15));
  return NF_OK;
}

struct ClusterArgs {
  void *phi;
  int32_t *stats, *labels;
  int V;
  int L[4];
  int lab_bytes;
  double w0;
  PhiloxPos bond_pos, flip_pos;
};

// What LADDER adds (nf_phi4_cluster_ladder): the table of the K rungs' coefficients and the rung every chain holds, as
// nf_hmc.hip's HmcLadderArgs; w0 is unused
struct ClusterLadderArgs : ClusterArgs {
  const double *coef;   // (K, 3): row k starts with the w0 of rung k
  const int32_t *rung;  // (C): the rung of chain c, clamped into 0 .. K - 1 by the kernel
  int K;
};

template <bool LADDER>
using ClusterKernelArgs = std::conditional_t<LADDER, ClusterLadderArgs, ClusterArgs>;

template <typename T, int NS, bool LADDER>
__global__ __launch_bounds__(kClMaxLanes) void phi4_cluster_kernel(ClusterKernelArgs<LADDER> A) {
  extern __shared__ __align__(16) unsigned char cl_lds[];
  volatile int *s_flag = reinterpret_cast<volatile int *>(cl_lds);     // [2]: did round r (mod 2) see a link with two labels
  int *s_sum = reinterpret_cast<int *>(cl_lds) + 2;                   // clusters, sites flipped, the largest cluster
  int *lab = reinterpret_cast<int *>(cl_lds + kClScratchBytes);
  uint8_t *bnd = cl_lds + kClScratchBytes + A.lab_bytes;
  const int tid = threadIdx.x, NT = blockDim.x, V = A.V;
  const int64_t c = blockIdx.x;
  const uint64_t i0 = uint64_t(c) * uint64_t(V);
  T *__restrict__ gphi = static_cast<T *>(A.phi) + c * int64_t(V);
  const int st[4] = {A.L[1] * A.L[2] * A.L[3], A.L[2] * A.L[3], A.L[3], 1};
  // the step to the forward neighbour along mu from a site at the end of its axis; 0 for an axis of extent 1 (no link)
  const int wrap[4] = {-st[0] * (A.L[0] - 1), -st[1] * (A.L[1] - 1), -st[2] * (A.L[2] - 1), -st[3] * (A.L[3] - 1)};
  auto fwd = [&](int x, uint32_t b, int mu) { return x + ((b >> (4 + mu)) & 1u ? wrap[mu] : st[mu]); };
  // LADDER: the chain's w0 is that of row rung[c] of the table, read once into scalar registers, and its stats row is the
  // rung-ordered (c / K) K + rung[c]; phi, the labels and the Philox indices stay at c
  double lw0 = 0.0;
  int64_t oc = c;
  if constexpr (LADDER) {
    const int r = min(max(int(A.rung[c]), 0), A.K - 1);
    lw0 = uniform_scalar(A.coef[3 * int64_t(r)]);
    oc = c / A.K * A.K + r;
  }

  // ---- bonds: one Philox call per site, word mu for the link (x, mu); phi(x) stays in a register for the flip
  T phi[NS];
  if (tid < 5) reinterpret_cast<int *>(cl_lds)[tid] = 0;
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    const int x = tid + k * NT;
    phi[k] = T(0);
    if (x < V) {
      int r = x;
      const int x3 = r % A.L[3]; r /= A.L[3];
      const int x2 = r % A.L[2]; r /= A.L[2];
      const int x1 = r % A.L[1];
      const int x0 = r / A.L[1];
      const int xs[4] = {x0, x1, x2, x3};
      uint32_t w[4];
      philox_words(A.bond_pos, i0 + uint64_t(x), w);
      const T p = gphi[x];
      phi[k] = p;
      uint32_t b = 0;
#pragma unroll
      for (int mu = 0; mu < 4; ++mu) {
        if (A.L[mu] > 1) {
          if (xs[mu] == A.L[mu] - 1) b |= 16u << mu;
          const T q = gphi[fwd(x, b, mu)];
          if (cluster_bond(LADDER ? lw0 : A.w0, double(p), double(q), philox_u32_mid(w[mu]))) b |= 1u << mu;
        }
      }
      lab[x] = x;
      bnd[x] = uint8_t(b);
    }
  }
  __syncthreads();

  // ---- labels: at most V rounds (see the head of the file)
  int rounds = 0;
  bool settled = false;
  for (int r = 0; r < V; ++r) {
    bool changed = false;
#pragma unroll 1
    for (int k = 0; k < NS; ++k) {
      const int x = tid + k * NT;
      if (x < V) {
        const uint32_t b = bnd[x];
#pragma unroll
        for (int mu = 0; mu < 4; ++mu) {
          if ((b >> mu) & 1u) {
            const int y = fwd(x, b, mu);
            const int lx = lab[x], ly = lab[y];
            if (lx != ly) {
              changed = true;
              const int lo = min(lx, ly), hi = max(lx, ly);
              atomicMin(&lab[lx < ly ? y : x], lo);
              atomicMin(&lab[hi], lo);
            }
          }
        }
      }
    }
    if (changed) s_flag[r & 1] = 1;
    __syncthreads();
#pragma unroll 1
    for (int k = 0; k < NS; ++k) {
      const int x = tid + k * NT;
      if (x < V) {
        const int l0 = lab[x];
        int l = l0, n = lab[l];
        while (n != l) {      // n < l: lab[z] <= z everywhere, so the chase strictly decreases and ends
          l = n;
          n = lab[l];
        }
        if (l != l0) lab[x] = l;
      }
    }
    const bool any = s_flag[r & 1] != 0;
    if (tid == 0) s_flag[(r + 1) & 1] = 0;      // last read before this round's first barrier
    __syncthreads();
    ++rounds;
    if (!any) {
      settled = true;
      break;
    }
  }

  // ---- sizes, flips, sums.  `settled` is the same in every lane.
  int mine[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    const int x = tid + k * NT;
    mine[k] = x < V ? lab[x] : 0;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    const int x = tid + k * NT;
    if (x < V) lab[x] = 0;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    const int x = tid + k * NT;
    if (x < V) atomicAdd(&lab[mine[k]], 1);
  }
  __syncthreads();
  int ncl = 0, nfl = 0, big = 0;
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    const int x = tid + k * NT;
    if (x < V) {
      const int l = mine[k];
      if (l == x) {
        ++ncl;
        big = max(big, lab[x]);
      }
      if (A.labels) A.labels[c * int64_t(V) + x] = l;
      if (settled && cluster_flips(A.flip_pos, i0 + uint64_t(l))) {
        ++nfl;
        gphi[x] = flip_sign(phi[k]);
      }
    }
  }
  ncl = wave_sum_int(ncl);
  nfl = wave_sum_int(nfl);
  big = wave_max_int(big);
  if ((tid & (kWave - 1)) == 0) {
    atomicAdd(&s_sum[0], ncl);
    atomicAdd(&s_sum[1], nfl);
    atomicMax(&s_sum[2], big);
  }
  __syncthreads();
  if (tid == 0) {
    int32_t *row = A.stats + 4 * oc;
    row[0] = settled ? s_sum[0] : 0;
    row[1] = settled ? s_sum[1] : 0;
    row[2] = settled ? s_sum[2] : 0;
    row[3] = settled ? rounds : -1;
  }
}

template <typename T, int NS, bool LADDER>
static int launch_cluster(const char *what, const ClusterKernelArgs<LADDER> &A, int64_t C, const ClusterPlan &p, hipStream_t s) {
  auto kern = phi4_cluster_kernel<T, NS, LADDER>;
  if (p.lds > 64 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                          int(p.lds)) != hipSuccess) {
    (void)hipGetLastError();
    set_error("%s: cannot raise the dynamic LDS limit to %zu B", what, p.lds);
    return NF_ELAUNCH;
  }
  hipLaunchKernelGGL(kern, dim3(unsigned(C)), dim3(unsigned(p.nt)), p.lds, s, A);
  return check_launch(what);
}

template <typename T, bool LADDER>
static int dispatch_cluster(const char *what, const ClusterKernelArgs<LADDER> &A, int64_t C, const ClusterPlan &p, hipStream_t s) {
  switch (p.ns) {
    case 1: return launch_cluster<T, 1, LADDER>(what, A, C, p, s);
    case 2: return launch_cluster<T, 2, LADDER>(what, A, C, p, s);
    case 4: return launch_cluster<T, 4, LADDER>(what, A, C, p, s);
    case 8: return launch_cluster<T, 8, LADDER>(what, A, C, p, s);
    case 16:
      if constexpr (sizeof(T) == 4) return launch_cluster<T, 16, LADDER>(what, A, C, p, s);     // 8-byte fields end at 8 sites per lane
  }
  set_error("%s: no kernel for %d sites per lane", what, p.ns);
  return NF_EINVAL;
}

// nf_phi4_cluster (coef == NULL, not a ladder call) and nf_phi4_cluster_ladder (ladder: w0 unused)
static int cluster_entry(const char *what, bool ladder, void *phi, int32_t *stats, int32_t *labels_out, int64_t C,
                         const int32_t *lattice, double w0, const double *coef, int K, const int32_t *rung, uint64_t seed,
                         uint64_t offset, int dtype, void *stream) {
  NF_REQUIRE(phi && stats, "%s: phi or stats is NULL", what);
  NF_REQUIRE(C >= 1 && C <= 65535, "%s: C (%lld) must be in 1 .. 65535", what, (long long)C);
  ClusterPlan p;
  int rc = cluster_plan(what, lattice, dtype, p);
  if (!rc && ladder) rc = hmc_ladder_checks(what, coef, K, rung, C);
  if (rc) return rc;
  ClusterLadderArgs A{};
  A.phi = phi; A.stats = stats; A.labels = labels_out;
  A.V = int(p.V);
  for (int mu = 0; mu < 4; ++mu) A.L[mu] = p.L[mu];
  A.lab_bytes = int(p.lab_bytes);
  A.w0 = w0;
  A.bond_pos = philox_pos(seed, NF_PHILOX_CLUSTER_DOMAIN, offset);
  A.flip_pos = philox_pos_after(A.bond_pos, 1);
  A.coef = coef; A.rung = rung; A.K = K;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (ladder) return dtype == NF_F32 ? dispatch_cluster<float, true>(what, A, C, p, s) : dispatch_cluster<double, true>(what, A, C, p, s);
  return dtype == NF_F32 ? dispatch_cluster<float, false>(what, A, C, p, s) : dispatch_cluster<double, false>(what, A, C, p, s);
}

// The sweep's draws, element-wise: u (n, 4) = the bond uniforms of index i, flip (n) = the flip bit of index i as a label
constexpr int kDrawLanes = 256;
__global__ __launch_bounds__(kDrawLanes) void cluster_draws_kernel(double *u, uint8_t *flip, int64_t n, PhiloxPos bond_pos,
                                                                   PhiloxPos flip_pos) {
  for (int64_t i = int64_t(blockIdx.x) * kDrawLanes + threadIdx.x; i < n; i += int64_t(gridDim.x) * kDrawLanes) {
    uint32_t w[4];
    philox_words(bond_pos, uint64_t(i), w);
#pragma unroll
    for (int mu = 0; mu < 4; ++mu) u[4 * i + mu] = philox_u32_mid(w[mu]);
    flip[i] = uint8_t(cluster_flips(flip_pos, uint64_t(i)));
  }
}

}  // namespace nf

using namespace nf;

extern "C" int nf_phi4_cluster_supported(const int32_t *lattice, int dtype) {
  ClusterPlan p;
  return cluster_plan("nf_phi4_cluster_supported", lattice, dtype, p) == NF_OK ? 1 : 0;
}

extern "C" int nf_phi4_cluster_plan(const int32_t *lattice, int dtype, nf_cluster_plan *out) {
  NF_REQUIRE(out != nullptr, "nf_phi4_cluster_plan: out is NULL");
  ClusterPlan p;
  const int rc = cluster_plan("nf_phi4_cluster_plan", lattice, dtype, p);
  if (rc) return rc;
  out->sites_per_lane = p.ns;
  out->lanes = p.nt;
  out->lds_bytes = int64_t(p.lds);
  return NF_OK;
}

extern "C" int nf_phi4_cluster(void *phi, int32_t *stats, int32_t *labels_out, int64_t C, const int32_t *lattice, double w0,
                               uint64_t seed, uint64_t offset, int dtype, void *stream) {
  return cluster_entry("nf_phi4_cluster", false, phi, stats, labels_out, C, lattice, w0, nullptr, 0, nullptr, seed, offset,
                       dtype, stream);
}

extern "C" int nf_phi4_cluster_ladder(void *phi, int32_t *stats, int32_t *labels_out, int64_t C, const int32_t *lattice,
                                      const double *coef, int K, const int32_t *rung, uint64_t seed, uint64_t offset,
                                      int dtype, void *stream) {
  return cluster_entry("nf_phi4_cluster_ladder", true, phi, stats, labels_out, C, lattice, 0.0, coef, K, rung, seed, offset,
                       dtype, stream);
}

extern "C" int nf_phi4_cluster_draws(double *u_out, uint8_t *flip_out, int64_t C, const int32_t *lattice, uint64_t seed,
                                     uint64_t offset, void *stream) {
  const char *what = "nf_phi4_cluster_draws";
  NF_REQUIRE(u_out && flip_out, "%s: u_out or flip_out is NULL", what);
  NF_REQUIRE(lattice != nullptr, "%s: lattice is NULL", what);
  NF_REQUIRE(C >= 1 && C <= 65535, "%s: C (%lld) must be in 1 .. 65535", what, (long long)C);
  int64_t V = 1;
  for (int mu = 0; mu < 4; ++mu) {
    NF_REQUIRE(lattice[mu] >= 1, "%s: lattice extents must be >= 1", what);
    V *= lattice[mu];
    NF_REQUIRE(V < (int64_t(1) << 31), "%s: the lattice (%d, %d, %d, %d) has 2^31 sites or more", what, lattice[0], lattice[1],
               lattice[2], lattice[3]);
  }
  const int64_t n = C * V;
  const int64_t blocks = (n + kDrawLanes - 1) / kDrawLanes;
  const PhiloxPos bond_pos = philox_pos(seed, NF_PHILOX_CLUSTER_DOMAIN, offset);
  hipLaunchKernelGGL(cluster_draws_kernel, dim3(unsigned(blocks < kMaxBlocksX ? blocks : kMaxBlocksX)), dim3(kDrawLanes), 0,
                     static_cast<hipStream_t>(stream), u_out, flip_out, n, bond_pos, philox_pos_after(bond_pos, 1));
  return check_launch(what);
}

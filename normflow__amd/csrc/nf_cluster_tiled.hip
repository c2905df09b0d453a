// nf_cluster_tiled.hip -- nf_cluster.hip's Swendsen-Wang sweep for chains that live in HBM: many workgroups per chain, any
// lattice of 1 to 4 axes with V < 2^31 (32^3, 16^4, 32^4, 48^4, ...).  The rule, its Philox draws and the label convention
// are stated in include/normflow_hip.h ("cluster updates"); the draws, the bond test and the flip bit are
// nf_sampler_core.h's, the lock-free union is nf_cluster_union.h's.  The labels are the unique fixed point "smallest site
// index of the cluster", so the result is nf_phi4_cluster's bit for bit, whatever the tiles and the schedule were.
// A chain is cut into TILES, runs of tile_sites consecutive site indices (the last may be short, a tile may be cut in the
// middle of a row).  A forward link (x, mu) is LOCAL iff its other end lies in the same run -- links that wrap around an
// axis included -- and because a tile is a run, a label minus the tile's first index is its LDS slot.
// Four launches in a line on the stream, after one memset of the per-chain flags:
//   1. local   one workgroup per (chain, tile): Philox per site, phi(x) and its forward neighbours from HBM, one bond byte
//              per site in nf_cluster.hip's encoding (bits 0 .. 3 active, bits 4 .. 7 wrap); the tile's local links are
//              labelled in LDS by nf_cluster.hip's rounds (hooking by ds_min, pointer jumping, every barrier in uniform
//              control flow), AT MOST n ROUNDS for a tile of n sites (a label travels at least one link per round, the
//              argument of nf_cluster.hip on the tile's own graph).  Labels (as site indices of the chain) and bond bytes
//              go to the workspace, the chain's size array is zeroed, tile 0 zeroes the chain's stats row.
//   2. merge   one lane per site: every active link of the site that crosses tiles unites the two trees of the label array
//              in HBM by uf_unite (nf_cluster_union.h): chase both ends to roots, hi > lo, old = atomicMin(&lab[hi], lo),
//              done if old == hi, else go on with (root of old, root of lo).  AT MOST V - 1 ATOMICS per link (hi strictly
//              decreases; derived in nf_cluster_union.h) and at most V steps per chase (the labels strictly decrease).
//              No lane ever waits for another workgroup: no spin, no flag, no ticket.  The L2s of the XCDs are not
//              coherent within a launch, so every read of the label array here is a relaxed agent-scope atomic load and
//              every write an agent-scope atomic minimum; a stale read shows an older, larger, still valid label, and the
//              minimum's return value corrects it.  That the labels are final rests on the kernel boundary after this
//              launch, not on fences.
//   3. flatten every site chases to its root (at most V steps; plain loads, the forest is final), stores it (to labels_out
//              too) and adds 1 to its root's slot of the size array: integer atomics, one per distinct root of a wave's
//              64 sites, the wave's commonest root once per wave.
//   4. flip    every site takes its root's flip bit and, where set, stores phi back with the sign bit flipped: plain vector
//              stores, nothing else of phi is written.  Clusters, sites flipped and the largest cluster are integer
//              reductions into stats (C, 4).
// A chain on which any bound is hit sets its flag; phase 4 then leaves its phi untouched and writes (0, 0, 0, -1), as
// nf_phi4_cluster does.  It cannot happen: the bounds are there so that a bug cannot become a hang.  Otherwise
// stats[c, 3] = the number of tiles of a chain (>= 1).  It is not a round count: how many rounds phase 1 takes depends on
// the order in which the lanes' ds_min land, and every column of stats is to be a pure function of the inputs.  The most
// rounds that a tile of the chain took stay in the workspace's flags, for whoever wants to look.
// Workspace, per call: labels (C, V) int32 | sizes (C, V) int32 | flags (C, 2) int32 (bound hit, most local rounds) | bond
// bytes (C, V).  Integer atomics only: the same inputs give the same bits.
// nf_phi4_cluster_tiled_ladder compiles phases 1 and 4 a second time with LADDER: phase 1 takes w0 from row rung[c] of the
// ladder's table, and both address the stats row (c / K) K + rung[c]; everything else, the launches included, is the same.
#include <type_traits>

#include "nf_sampler_core.h"
#include "nf_cluster_union.h"

namespace nf {

constexpr int kCtMaxLanes = 1024;                  // phase 1: a tile's workgroup
constexpr int kCtLanes = 256;                      // phases 2 .. 4
constexpr int kCtSitesPerLane = 16;                // phases 3 and 4: a workgroup owns 4096 consecutive sites
constexpr int kCtBlockSites = kCtLanes * kCtSitesPerLane;
constexpr size_t kCtScratchBytes = 256;            // the loop's two flags, in front of the labels
constexpr int kCtMaxTileSites = 32704;             // 256 + 5 x 32704 = 163776 <= 160 KiB
constexpr int kCtDefaultTileSites = 16384;         // tools/cluster_bench.py --tiled (README, "Cluster updates")
constexpr size_t kCtAlign = 16;
constexpr size_t kCtMaxLds = kCtScratchBytes + 5 * size_t(kCtMaxTileSites);      // both arrays are multiples of 16 there
static_assert(kCtMaxTileSites % 16 == 0 && kCtMaxLds <= 160 * 1024, "the largest tile must fit the LDS of a CU");

struct ClusterTiledPlan {
  int64_t V;
  int L[4];
  int ts;              // the tile_sites in force: min(the request or the default, V)
  int64_t tiles;       // per chain
  int nt;              // lanes of a tile's workgroup
  size_t lab_bytes;    // 4 ts, rounded up to 16
  size_t lds;          // kCtScratchBytes + lab_bytes + ts rounded up to 16
};

static int cluster_tiled_plan(const char *what, const int32_t *lattice, int dtype, int64_t tile_sites, ClusterTiledPlan &p) {
  NF_REQUIRE(lattice != nullptr, "%s: lattice is NULL", what);
  NF_REQUIRE(dtype == NF_F32 || dtype == NF_F64, "%s: unsupported dtype %d", what, dtype);
  p.V = 1;
  for (int mu = 0; mu < 4; ++mu) {
    NF_REQUIRE(lattice[mu] >= 1, "%s: lattice extents must be >= 1", what);
    p.L[mu] = lattice[mu];
    p.V *= lattice[mu];
    NF_REQUIRE(p.V < (int64_t(1) << 31), "%s: the lattice (%d, %d, %d, %d) has 2^31 sites or more", what, lattice[0], lattice[1],
               lattice[2], lattice[3]);
  }
  NF_REQUIRE(tile_sites >= 0 && tile_sites <= kCtMaxTileSites,
             "%s: tile_sites (%lld) must be 0 (the default, %d) or 1 .. %d, what the LDS holds", what, (long long)tile_sites,
             kCtDefaultTileSites, kCtMaxTileSites);
  const int64_t ts = tile_sites ? tile_sites : kCtDefaultTileSites;
  p.ts = int(ts < p.V ? ts : p.V);
  p.tiles = (p.V + p.ts - 1) / p.ts;
  const int nt = (p.ts + kWave - 1) / kWave * kWave;
  p.nt = nt < kCtMaxLanes ? nt : kCtMaxLanes;
  NF_REQUIRE(p.tiles * p.nt < (int64_t(1) << 32), "%s: %lld tiles of %d sites are more than one launch takes (tiles x lanes < 2^32)",
             what, (long long)p.tiles, p.ts);
  p.lab_bytes = (size_t(p.ts) * 4 + 15) & ~size_t(15);
  p.lds = kCtScratchBytes + p.lab_bytes + ((size_t(p.ts) + 15) & ~size_t(15));
  return NF_OK;
}

static size_t cluster_tiled_workspace(int64_t C, int64_t V) {
  const size_t n = size_t(C) * size_t(V);
  return 4 * n + 4 * n + 8 * size_t(C) + n;
}

struct ClusterTiledArgs {
  void *phi;
  int32_t *stats, *labels_out;
  int *lab, *size, *flags;
  uint8_t *bnd;
  int V, ts, tiles;
  int L[4];
  int lab_bytes;
  double w0;
  PhiloxPos bond_pos, flip_pos;
};

// What LADDER adds (nf_phi4_cluster_tiled_ladder), as nf_cluster.hip's ClusterLadderArgs; w0 is unused.  Phase 1 takes w0
// from row rung[c] of the table and phases 1 and 4 address the chain's stats row by the rung; phases 2 and 3 are the plain
// kernels.  `rung` is not written between the launches of a call, so every workgroup of a chain reads the same rung.
struct ClusterTiledLadderArgs : ClusterTiledArgs {
  const double *coef;   // (K, 3): row k starts with the w0 of rung k
  const int32_t *rung;  // (C): the rung of chain c, clamped into 0 .. K - 1 by the kernels
  int K;
};

template <bool LADDER>
using ClusterTiledKernelArgs = std::conditional_t<LADDER, ClusterTiledLadderArgs, ClusterTiledArgs>;

// The rung of chain c, clamped, and its rung-ordered stats row (c / K) K + rung
__device__ __forceinline__ int ladder_rung(const ClusterTiledLadderArgs &A, int64_t c) { return min(max(int(A.rung[c]), 0), A.K - 1); }
__device__ __forceinline__ int64_t ladder_row(const ClusterTiledLadderArgs &A, int64_t c) { return c / A.K * A.K + ladder_rung(A, c); }

// The label array in HBM as nf_cluster_union.h sees it
struct DeviceAtomics {
  typedef int cell;
  static __device__ __forceinline__ int load(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  static __device__ __forceinline__ int fetch_min(int *p, int v) {
    return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
};

// The same array once the unions are done (phase 3): plain loads
struct FinalForest {
  typedef int cell;
  static __device__ __forceinline__ int load(const int *p) { return *p; }
};

// The steps to the forward neighbours: st[mu] inside an axis, wrap[mu] from its last site (0 for an axis of extent 1)
struct Steps {
  int st[4], wrap[4];
  __device__ __forceinline__ explicit Steps(const int (&L)[4]) {
    st[0] = L[1] * L[2] * L[3]; st[1] = L[2] * L[3]; st[2] = L[3]; st[3] = 1;
#pragma unroll
    for (int mu = 0; mu < 4; ++mu) wrap[mu] = -st[mu] * (L[mu] - 1);
  }
  __device__ __forceinline__ int fwd(int x, uint32_t b, int mu) const { return x + ((b >> (4 + mu)) & 1u ? wrap[mu] : st[mu]); }
};

// ---------------------------------------------------------------- phase 1: bonds and the labels of the tile's local links
template <typename T, bool LADDER>
__global__ __launch_bounds__(kCtMaxLanes) void cluster_tiled_local_kernel(ClusterTiledKernelArgs<LADDER> A) {
  extern __shared__ __align__(16) unsigned char ct_lds[];
  volatile int *s_flag = reinterpret_cast<volatile int *>(ct_lds);     // [2]: did round r (mod 2) see a link with two labels
  int *lab = reinterpret_cast<int *>(ct_lds + kCtScratchBytes);        // slot s holds the site t0 + s
  uint8_t *bnd = ct_lds + kCtScratchBytes + A.lab_bytes;
  const int tid = threadIdx.x, NT = blockDim.x, V = A.V;
  const int64_t c = blockIdx.y;
  const int t0 = int(int64_t(blockIdx.x) * A.ts);                     // < V: there are ceil(V / ts) tiles
  const int n = min(A.ts, V - t0);
  const uint64_t i0 = uint64_t(c) * uint64_t(V);
  const T *__restrict__ gphi = static_cast<const T *>(A.phi) + c * int64_t(V);
  const Steps S(A.L);
  // LADDER: the w0 of the chain's rung, read once into scalar registers, and the rung-ordered stats row
  double lw0 = 0.0;
  int64_t oc = c;
  if constexpr (LADDER) {
    lw0 = uniform_scalar(A.coef[3 * int64_t(ladder_rung(A, c))]);
    oc = ladder_row(A, c);
  }

  if (tid < 2) s_flag[tid] = 0;
  for (int s = tid; s < n; s += NT) {
    const int x = t0 + s;
    int r = x;
    const int x3 = r % A.L[3]; r /= A.L[3];
    const int x2 = r % A.L[2]; r /= A.L[2];
    const int x1 = r % A.L[1];
    const int x0 = r / A.L[1];
    const int xs[4] = {x0, x1, x2, x3};
    uint32_t w[4];
    philox_words(A.bond_pos, i0 + uint64_t(x), w);
    const T p = gphi[x];
    uint32_t b = 0;
#pragma unroll
    for (int mu = 0; mu < 4; ++mu) {
      if (A.L[mu] > 1) {
        if (xs[mu] == A.L[mu] - 1) b |= 16u << mu;
        const T q = gphi[S.fwd(x, b, mu)];
        if (cluster_bond(LADDER ? lw0 : A.w0, double(p), double(q), philox_u32_mid(w[mu]))) b |= 1u << mu;
      }
    }
    lab[s] = s;
    bnd[s] = uint8_t(b);
  }
  __syncthreads();

  // nf_cluster.hip's rounds on the links with both ends in [t0, t0 + n): at most n rounds
  int rounds = 0;
  bool settled = false;
  for (int r = 0; r < n; ++r) {
    bool changed = false;
    for (int s = tid; s < n; s += NT) {
      const uint32_t b = bnd[s];
#pragma unroll
      for (int mu = 0; mu < 4; ++mu) {
        if ((b >> mu) & 1u) {
          const int sy = S.fwd(t0 + s, b, mu) - t0;
          if (unsigned(sy) < unsigned(n)) {
            const int lx = lab[s], ly = lab[sy];
            if (lx != ly) {
              changed = true;
              const int lo = min(lx, ly), hi = max(lx, ly);
              atomicMin(&lab[lx < ly ? sy : s], lo);
              atomicMin(&lab[hi], lo);
            }
          }
        }
      }
    }
    if (changed) s_flag[r & 1] = 1;
    __syncthreads();
    for (int s = tid; s < n; s += NT) {
      const int l0 = lab[s];
      int l = l0, m = lab[l];
      while (m != l) {        // m < l: lab[z] <= z everywhere, so the chase strictly decreases and ends
        l = m;
        m = lab[l];
      }
      if (l != l0) lab[s] = l;
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

  const int64_t g0 = c * int64_t(V) + t0;
  for (int s = tid; s < n; s += NT) {
    A.lab[g0 + s] = t0 + lab[s];
    A.bnd[g0 + s] = bnd[s];
    A.size[g0 + s] = 0;
  }
  if (tid == 0) {
    if (!settled) atomicOr(&A.flags[2 * c], 1);
    atomicMax(&A.flags[2 * c + 1], rounds);
    if (blockIdx.x == 0) {
      int32_t *row = A.stats + 4 * oc;
      row[0] = 0; row[1] = 0; row[2] = 0; row[3] = 0;
    }
  }
}

// ---------------------------------------------------------------- phase 2: the links that cross tiles
__global__ __launch_bounds__(kCtLanes) void cluster_tiled_merge_kernel(ClusterTiledArgs A) {
  const int64_t xx = int64_t(blockIdx.x) * kCtLanes + threadIdx.x;
  if (xx >= A.V) return;
  const int x = int(xx), V = A.V;
  const int64_t c = blockIdx.y;
  const uint32_t b = A.bnd[c * int64_t(V) + x];
  if ((b & 15u) == 0) return;
  int *lab = A.lab + c * int64_t(V);
  const Steps S(A.L);
  const int t0 = x / A.ts * A.ts;
  bool ok = true;
#pragma unroll
  for (int mu = 0; mu < 4; ++mu) {
    if ((b >> mu) & 1u) {
      const int y = S.fwd(x, b, mu);
      if (unsigned(y - t0) >= unsigned(A.ts)) ok &= uf_unite<DeviceAtomics>(lab, x, y, V);
    }
  }
  if (!ok) atomicOr(&A.flags[2 * c], 1);
}

// ---------------------------------------------------------------- phase 3: every site's root, the clusters' sizes
// A workgroup owns kCtBlockSites consecutive sites, lane tid the sites tid + k kCtLanes.  Adds to one word from all over the
// chip cost about 0.1 us each, one after the other, and near the critical point most sites share ONE root: so a wave adds
// once per distinct root of its 64 sites, and carries the count of the root that fills most of the wave (`held`) across
// its kCtSitesPerLane turns.  `held`, `nheld` and every value that steers the loops are the same in all lanes of a wave.
__global__ __launch_bounds__(kCtLanes) void cluster_tiled_flatten_kernel(ClusterTiledArgs A) {
  const int V = A.V, lane = threadIdx.x & (kWave - 1);
  const int64_t c = blockIdx.y;
  const int64_t x0 = int64_t(blockIdx.x) * kCtBlockSites + threadIdx.x;
  int *lab = A.lab + c * int64_t(V);
  int *size = A.size + c * int64_t(V);
  int held = -1, nheld = 0;
  for (int k = 0; k < kCtSitesPerLane; ++k) {
    const int64_t xx = x0 + int64_t(k) * kCtLanes;
    const bool live = xx < V;
    const int x = int(xx);
    int root = -1;
    if (live) {
      // the forest is final here, so plain loads and stores do: no root changes any more, and storing a site's root over
      // its label only shortens the chases of the other lanes -- the old and the new label (a 4-byte store does not
      // tear) are both valid steps of a chase that ends at the same root
      if (!uf_root<FinalForest>(lab, x, V, root)) atomicOr(&A.flags[2 * c], 1);
      if (lab[x] != root) lab[x] = root;
      if (A.labels_out) A.labels_out[c * int64_t(V) + x] = root;
    }
    unsigned long long todo = __ballot(live);
    while (todo) {               // at most 64 turns: every turn takes its leader out of `todo`
      const int leader = __ffsll(todo) - 1;
      const int r0 = __shfl(root, leader, kWave);
      const unsigned long long same = __ballot(live && root == r0) & todo;
      const int n = __popcll(same);
      if (r0 == held) {
        nheld += n;
      } else if (held < 0 || n >= kWave / 2) {
        if (held >= 0 && lane == 0) atomicAdd(&size[held], nheld);
        held = r0;
        nheld = n;
      } else if (lane == leader) {
        atomicAdd(&size[r0], n);
      }
      todo &= ~same;
    }
  }
  if (held >= 0 && lane == 0) atomicAdd(&size[held], nheld);
}

// ---------------------------------------------------------------- phase 4: flips and stats
template <typename T, bool LADDER>
__global__ __launch_bounds__(kCtLanes) void cluster_tiled_flip_kernel(ClusterTiledKernelArgs<LADDER> A) {
  __shared__ int s_sum[3];
  const int tid = threadIdx.x, V = A.V;
  const int64_t c = blockIdx.y;
  const int64_t x0 = int64_t(blockIdx.x) * kCtBlockSites + tid;
  const bool bad = A.flags[2 * c] != 0;       // final since phase 3 ended; the same in every lane of the chain
  if (tid < 3) s_sum[tid] = 0;
  __syncthreads();
  int ncl = 0, nfl = 0, big = 0;
  if (!bad) {
    T *gphi = static_cast<T *>(A.phi);
    for (int k = 0; k < kCtSitesPerLane; ++k) {
      const int64_t xx = x0 + int64_t(k) * kCtLanes;
      if (xx < V) {
        const int64_t g = c * int64_t(V) + xx;
        const int l = A.lab[g];
        if (l == int(xx)) {
          ++ncl;
          big = max(big, A.size[g]);
        }
        if (cluster_flips(A.flip_pos, uint64_t(c) * uint64_t(V) + uint64_t(l))) {
          ++nfl;
          gphi[g] = flip_sign(gphi[g]);
        }
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
    int64_t oc = c;
    if constexpr (LADDER) oc = ladder_row(A, c);
    int32_t *row = A.stats + 4 * oc;
    if (!bad) {
      if (s_sum[0]) atomicAdd(&row[0], s_sum[0]);
      if (s_sum[1]) atomicAdd(&row[1], s_sum[1]);
      if (s_sum[2]) atomicMax(&row[2], s_sum[2]);
    }
    if (blockIdx.x == 0) row[3] = bad ? -1 : A.tiles;
  }
}

template <typename T, bool LADDER>
static int launch_cluster_tiled(const char *what, const ClusterTiledKernelArgs<LADDER> &A, int64_t C, const ClusterTiledPlan &p,
                                hipStream_t s) {
  auto local = cluster_tiled_local_kernel<T, LADDER>;
  // once per instantiation and for the largest tile there is: nothing is set per sweep, or inside a stream capture that
  // is not the first call
  static const hipError_t raised = hipFuncSetAttribute(reinterpret_cast<const void *>(local),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, int(kCtMaxLds));
  if (raised != hipSuccess && p.lds > 64 * 1024) {
    (void)hipGetLastError();
    set_error("%s: cannot raise the dynamic LDS limit to %zu B", what, kCtMaxLds);
    return NF_ELAUNCH;
  }
  if (hipMemsetAsync(A.flags, 0, 8 * size_t(C), s) != hipSuccess) {
    (void)hipGetLastError();
    set_error("%s: cannot clear the flags of the workspace", what);
    return NF_ELAUNCH;
  }
  const dim3 sites(unsigned((p.V + kCtLanes - 1) / kCtLanes), unsigned(C));
  hipLaunchKernelGGL(local, dim3(unsigned(p.tiles), unsigned(C)), dim3(unsigned(p.nt)), p.lds, s, A);
  int rc = check_launch(what);
  if (rc) return rc;
  if (p.tiles > 1) {
    hipLaunchKernelGGL(cluster_tiled_merge_kernel, sites, dim3(kCtLanes), 0, s, static_cast<const ClusterTiledArgs &>(A));
    if ((rc = check_launch(what))) return rc;
  }
  const dim3 runs(unsigned((p.V + kCtBlockSites - 1) / kCtBlockSites), unsigned(C));
  hipLaunchKernelGGL(cluster_tiled_flatten_kernel, runs, dim3(kCtLanes), 0, s, static_cast<const ClusterTiledArgs &>(A));
  if ((rc = check_launch(what))) return rc;
  hipLaunchKernelGGL((cluster_tiled_flip_kernel<T, LADDER>), runs, dim3(kCtLanes), 0, s, A);
  return check_launch(what);
}

// nf_phi4_cluster_tiled (not a ladder call: coef, K and rung unused) and nf_phi4_cluster_tiled_ladder (ladder: w0 unused)
static int cluster_tiled_entry(const char *what, bool ladder, void *phi, int32_t *stats, int32_t *labels_out, int64_t C,
                               const int32_t *lattice, double w0, const double *coef, int K, const int32_t *rung, uint64_t seed,
                               uint64_t offset, int dtype, int64_t tile_sites, void *workspace, size_t workspace_bytes,
                               void *stream) {
  NF_REQUIRE(phi && stats, "%s: phi or stats is NULL", what);
  NF_REQUIRE(C >= 1 && C <= 65535, "%s: C (%lld) must be in 1 .. 65535", what, (long long)C);
  ClusterTiledPlan p;
  int rc = cluster_tiled_plan(what, lattice, dtype, tile_sites, p);
  if (!rc && ladder) rc = hmc_ladder_checks(what, coef, K, rung, C);
  if (rc) return rc;
  const size_t need = cluster_tiled_workspace(C, p.V);
  NF_REQUIRE(workspace != nullptr, "%s: workspace is NULL (%zu B needed)", what, need);
  NF_REQUIRE(workspace_bytes >= need, "%s: workspace of %zu B is too small, %zu B needed", what, workspace_bytes, need);
  NF_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % kCtAlign == 0, "%s: workspace is not aligned to %zu B", what, kCtAlign);
  const size_t n = size_t(C) * size_t(p.V);
  ClusterTiledLadderArgs A{};
  A.phi = phi; A.stats = stats; A.labels_out = labels_out;
  A.lab = static_cast<int *>(workspace);
  A.size = A.lab + n;
  A.flags = A.size + n;
  A.bnd = reinterpret_cast<uint8_t *>(A.flags + 2 * size_t(C));
  A.V = int(p.V);
  A.ts = p.ts;
  A.tiles = int(p.tiles);
  for (int mu = 0; mu < 4; ++mu) A.L[mu] = p.L[mu];
  A.lab_bytes = int(p.lab_bytes);
  A.w0 = w0;
  A.bond_pos = philox_pos(seed, NF_PHILOX_CLUSTER_DOMAIN, offset);
  A.flip_pos = philox_pos_after(A.bond_pos, 1);
  A.coef = coef; A.rung = rung; A.K = K;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (ladder) {
    return dtype == NF_F32 ? launch_cluster_tiled<float, true>(what, A, C, p, s)
                           : launch_cluster_tiled<double, true>(what, A, C, p, s);
  }
  return dtype == NF_F32 ? launch_cluster_tiled<float, false>(what, A, C, p, s)
                         : launch_cluster_tiled<double, false>(what, A, C, p, s);
}

}  // namespace nf

using namespace nf;

extern "C" int nf_phi4_cluster_tiled_supported(const int32_t *lattice, int dtype, int64_t tile_sites) {
  ClusterTiledPlan p;
  return cluster_tiled_plan("nf_phi4_cluster_tiled_supported", lattice, dtype, tile_sites, p) == NF_OK ? 1 : 0;
}

extern "C" int nf_phi4_cluster_tiled_plan(const int32_t *lattice, int dtype, int64_t tile_sites, nf_cluster_tiled_plan *out) {
  NF_REQUIRE(out != nullptr, "nf_phi4_cluster_tiled_plan: out is NULL");
  ClusterTiledPlan p;
  const int rc = cluster_tiled_plan("nf_phi4_cluster_tiled_plan", lattice, dtype, tile_sites, p);
  if (rc) return rc;
  out->tiles = p.tiles;
  out->tile_sites = p.ts;
  out->lanes = p.nt;
  out->lds_bytes = int64_t(p.lds);
  return NF_OK;
}

extern "C" size_t nf_phi4_cluster_tiled_workspace(int64_t C, const int32_t *lattice, int64_t tile_sites) {
  ClusterTiledPlan p;
  if (C < 1 || C > 65535 || cluster_tiled_plan("nf_phi4_cluster_tiled_workspace", lattice, NF_F32, tile_sites, p) != NF_OK) return 0;
  return cluster_tiled_workspace(C, p.V);
}

extern "C" int nf_phi4_cluster_tiled(void *phi, int32_t *stats, int32_t *labels_out, int64_t C, const int32_t *lattice,
                                     double w0, uint64_t seed, uint64_t offset, int dtype, int64_t tile_sites, void *workspace,
                                     size_t workspace_bytes, void *stream) {
  return cluster_tiled_entry("nf_phi4_cluster_tiled", false, phi, stats, labels_out, C, lattice, w0, nullptr, 0, nullptr, seed,
                             offset, dtype, tile_sites, workspace, workspace_bytes, stream);
}

extern "C" int nf_phi4_cluster_tiled_ladder(void *phi, int32_t *stats, int32_t *labels_out, int64_t C, const int32_t *lattice,
                                            const double *coef, int K, const int32_t *rung, uint64_t seed, uint64_t offset,
                                            int dtype, int64_t tile_sites, void *workspace, size_t workspace_bytes,
                                            void *stream) {
  return cluster_tiled_entry("nf_phi4_cluster_tiled_ladder", true, phi, stats, labels_out, C, lattice, 0.0, coef, K, rung,
                             seed, offset, dtype, tile_sites, workspace, workspace_bytes, stream);
}

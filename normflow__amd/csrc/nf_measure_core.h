// nf_measure_core.h -- what the two measure kernels share (nf_measure.hip: a row or a segment of planes per workgroup;
// nf_measure_tiled.hip: a brick of a row per workgroup): the team and LDS constants, the staging of an image and
// measure_image, the one definition of every sum of an LDS image.
#pragma once
#include "nf_internal.h"

namespace nf {

constexpr int kMsMaxLanes = 512;
constexpr int kMsPackedSites = 256;               // rows up to this many sites are packed, one wave per row
constexpr int kMsWideTeam = 4096;                 // images beyond this many sites get 512 lanes
// The ONE team rule: the lanes that share an image of `sites` sites.  ms_image_team for an image that has a workgroup
// to itself (a resident row, a segment, a brick), ms_row_team for a whole row (a packed row gets one wave).  The fused
// HMC kernel (nf_hmc.hip) measures its LDS image by ms_row_team's lanes, which is why its rows are nf_lattice_measure's.
constexpr int ms_image_team(int64_t sites) { return sites > kMsWideTeam ? kMsMaxLanes : kBlock; }
constexpr int ms_row_team(int64_t sites) { return sites <= kMsPackedSites ? kWave : ms_image_team(sites); }
constexpr int kMsMaxStripes = 16;                 // stripes per slice, at most: the serial tail of a slice sum
constexpr size_t kMsRed = kMsMaxLanes / kWave * 8;               // doubles: 7 sums per wave
constexpr size_t kMsScratch = (kMsRed + kMsMaxLanes) * sizeof(double);   // ... and one stripe partial per lane
constexpr size_t kMsLdsBudget = 160 * 1024;
constexpr int64_t kMsMaxGroups = (int64_t(1) << 24) - 1;

template <typename T, int W>
__device__ __forceinline__ void stage_w(const T *src, T *img) {
  if constexpr (W == 1) *img = *src;
  else if constexpr (sizeof(T) == 4) *reinterpret_cast<float4 *>(img) = *reinterpret_cast<const float4 *>(src);
  else *reinterpret_cast<double2 *>(img) = *reinterpret_cast<const double2 *>(src);
}

// Every statistic of one image of E[0] x E[1] x E[2] x E[3] sites in LDS, by the `nt` lanes of a team (this lane is `tl`).
// Lext[mu] is the extent of the lattice's axis: no neighbour is read and no stripe summed along an axis of extent 1, its
// one slice entry is the sum of phi.  With `halo` != NULL axis a0 is cut: the image holds E[a0] < Lext[a0] of its planes
// and halo is the plane before them; otherwise every axis wraps inside the image.  HALO2 (a compile-time flag: without
// it the routine is what it was before there were bricks): with `halo1` != NULL axis a1 > a0 is cut as well (the axes
// before a0 and between the two have extent 1) and the image is part of ONE plane, E[a0] = 1: E[a1] < Lext[a1] of its
// sub-planes; halo is the same sub-planes of the plane before, halo1 the sub-plane before them in the image's own plane.
// dst: the 7 scalars, then the slice sums at off[]; written when `live`.  red / sp: the workgroup's reduction slots,
// `wave0` the team's first wave and `sp0` its first lane in them.  Every lane of the workgroup must call it (barriers),
// with the same E, Lext, a0 and a1.
template <typename T, bool HALO2>
__device__ __forceinline__ void measure_image(const T *img, const T *halo, const T *halo1, const int (&E)[4],
                                              const int (&Lext)[4], const int (&off)[4], int a0, int a1, int tl, int nt,
                                              int wave0, int sp0, double *red, double *sp, double *dst, bool live) {
  int str[4];
  str[3] = 1;
#pragma unroll
  for (int mu = 2; mu >= 0; --mu) str[mu] = str[mu + 1] * E[mu + 1];
  const int n = str[0] * E[0];
  // coordinates of site tl and of the stride nt, in the mixed radix of E
  int c[4], d[4];
  {
    int r = tl, s = nt;
#pragma unroll
    for (int mu = 3; mu >= 1; --mu) {
      c[mu] = r % E[mu]; r /= E[mu];
      d[mu] = s % E[mu]; s /= E[mu];
    }
    c[0] = r; d[0] = s;
  }
  double q[7] = {0, 0, 0, 0, 0, 0, 0};
  for (int i = tl; i < n; i += nt) {
    const double x = double(img[i]), x2 = x * x;
    q[0] += x;
    q[1] = fma(x, x, q[1]);
    q[2] = fma(x2, x2, q[2]);
#pragma unroll
    for (int mu = 0; mu < 4; ++mu)
      if (Lext[mu] > 1) {
        double nb;
        if (c[mu] > 0) nb = double(img[i - str[mu]]);
        else if (halo != nullptr && mu == a0) nb = double(halo[i]);       // axes before a0 have extent 1: i < plane
        else if (HALO2 && halo1 != nullptr && mu == a1) nb = double(halo1[i]);    // one plane: i < a sub-plane's sites
        else nb = double(img[i + (E[mu] - 1) * str[mu]]);
        q[3 + mu] = fma(x, nb, q[3 + mu]);
      }
#pragma unroll
    for (int mu = 3; mu >= 1; --mu) {
      c[mu] += d[mu];
      if (c[mu] >= E[mu]) { c[mu] -= E[mu]; ++c[mu - 1]; }
    }
    c[0] += d[0];
  }
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    q[k] = wave_sum(q[k]);
    if (lane == 0) red[w * 8 + k] = q[k];
  }
  __syncthreads();
  if (tl == 0 && live) {
    const int nw = nt / kWave;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      double r = 0;
      for (int i = 0; i < nw; ++i) r += red[(wave0 + i) * 8 + k];
      dst[k] = r;
      if (k == 0) {
#pragma unroll
        for (int mu = 0; mu < 4; ++mu)
          if (Lext[mu] == 1) dst[7 + off[mu]] = r;
      }
    }
  }
  // slice sums
#pragma unroll
  for (int mu = 0; mu < 4; ++mu) {
    if (Lext[mu] == 1) continue;
    const int Em = E[mu], inner = str[mu];
    int M = inner;                                       // sites of a slice
#pragma unroll
    for (int nu = 0; nu < 4; ++nu)
      if (nu < mu) M *= E[nu];
    int J = nt / Em < kMsMaxStripes ? nt / Em : kMsMaxStripes;
    if (J > M / 4) J = M / 4;
    if (J < 1) J = 1;
    const int P = Em * J, so = J / inner, si = J % inner;
    double *out = dst + 7 + off[mu];
    for (int p = tl; p < P; p += nt) {                 // more than one turn only when Em > nt (then J = 1)
      // neighbouring lanes on neighbouring addresses: slices along the fastest axis, stripes otherwise
      const int t = inner == 1 ? p % Em : p / J, j = inner == 1 ? p / Em : p % J;
      int o = j / inner, i = j % inner;
      double acc = 0;
      for (int k = j; k < M; k += J) {
        acc += double(img[(o * Em + t) * inner + i]);
        o += so; i += si;
        if (i >= inner) { i -= inner; ++o; }
      }
      if (J == 1) { if (live) out[t] = acc; }
      else sp[sp0 + t * J + j] = acc;
    }
    if (J > 1) {                                         // Em J <= nt
      __syncthreads();
      if (tl < Em) {
        double acc = 0;
        for (int j = 0; j < J; ++j) acc += sp[sp0 + tl * J + j];
        if (live) out[tl] = acc;
      }
      __syncthreads();
    }
  }
}

}  // namespace nf

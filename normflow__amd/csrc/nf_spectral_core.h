// nf_spectral_core.h -- the separable real Hartley transform of a field held in LDS, on the f32 / f64 matrix cores: what
// nf_spectral.hip (the power-spectrum filter of FFTNet_ / PSDBlock_) and nf_hmc_fa.hip (the kinetic operator of the
// Fourier-accelerated HMC) share, stated ONCE.  With H_N[k, n] = (cos(2 pi k n / N) + sin(2 pi k n / N)) / sqrt(N) (real,
// symmetric, orthogonal) and T = H_{N_1} x ... x H_{N_d}, `transform` replaces the field by T field, in place, one axis
// pass per axis of extent > 1; the layout of the passes and of the matrices is described at the head of nf_spectral.hip.
// The workgroup may have any number of whole waves: every routine takes it (`nthreads`, a multiple of kWave, uniform),
// every wave of the workgroup must call it, and an axis pass ends with its one barrier.
#pragma once
#include "nf_internal.h"

namespace nf {

constexpr int kSpecMaxAxis = 64;

// The axes of a transform: lengths (leading 1s), element strides of a row-major field, and where the axis' Hartley matrix
// lies in LDS.  Filled by spectral_axes (nf_spectral.hip, host).
struct HartleyAxes {
  int n[4], stride[4];   // axis lengths (leading 1s) and element strides
  int ldh[4], hoff[4];   // row stride and element offset of the axis' Hartley matrix in LDS (equal lengths share one)
  int hsize;             // elements of all matrices
  int V;                 // sites
};

// n[4] (each 1 .. kSpecMaxAxis, checked by the caller) -> strides, matrix layout, hsize and V.  Host code, nf_spectral.hip.
void spectral_axes(HartleyAxes &p, const int n[4]);

template <typename T> struct Mfma;
template <> struct Mfma<float> {
  typedef float acc_t __attribute__((ext_vector_type(4)));
  static __device__ __forceinline__ acc_t run(float a, float b, acc_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ int row(int lane, int r) { return (lane >> 4) * 4 + r; }
};
template <> struct Mfma<double> {     // the f64 form has its own C/D map: row = lane / 16 + 4 reg
  typedef double acc_t __attribute__((ext_vector_type(4)));
  static __device__ __forceinline__ acc_t run(double a, double b, acc_t c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ int row(int lane, int r) { return (lane >> 4) + 4 * r; }
};

// H[r][c] for r, c < N, zero in the padding; the angle is reduced exactly (r c mod N) and evaluated in double.
template <typename T>
__device__ void build_hartley(T *hm, const HartleyAxes &p, int nthreads) {
  for (int a = 0; a < 4; ++a) {
    const int N = p.n[a];
    if (N == 1) continue;
    bool shared = false;
    for (int c = 0; c < a; ++c) shared |= p.n[c] == N;
    if (shared) continue;
    const int ldh = p.ldh[a], rows = (N + 15) & ~15;
    const double norm = 1.0 / ::sqrt(double(N));
    T *h = hm + p.hoff[a];
    for (int idx = threadIdx.x; idx < rows * ldh; idx += nthreads) {
      const int r = idx / ldh, c = idx - r * ldh;
      double v = 0.0;
      if (r < N && c < N) {
        double sn, cs;
        ::sincospi(2.0 * double((r * c) % N) / double(N), &sn, &cs);
        v = (cs + sn) * norm;
      }
      h[idx] = T(v);
    }
  }
}

// One axis pass, in place: every line l of the `lines` lines (element n at (l / S) N S + l % S + n S) becomes H line.
// MT = ceil(N / 16) output tiles per line group; the k loop runs over 16 MT values of n in steps of JB quads whose LDS
// loads are all issued before the first MFMA needs one (rows of H beyond N are zero).
template <typename T, int MT>
__device__ __forceinline__ void axis_pass(T *buf, const T *h, int ldh, int N, int S, int lines, int nthreads) {
  using M = Mfma<T>;
  constexpr int JB = MT <= 2 ? 4 : 2;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int col = lane & 15, kq = lane >> 4;
  const int NS = N * S;
  const int groups = (lines + 15) >> 4;
#pragma unroll 1
  for (int g = wave; g < groups; g += nthreads / kWave) {
    const int l = g * 16 + col;
    const bool valid = l < lines;
    const int q = l / S;
    const int base = valid ? q * NS + (l - q * S) : 0;
    typename M::acc_t acc[MT];
#pragma unroll
    for (int it = 0; it < MT; ++it) acc[it] = typename M::acc_t{0, 0, 0, 0};
#pragma unroll 1
    for (int k0 = 0; k0 < 4 * MT; k0 += JB) {
      T b[JB], a[JB][MT];
#pragma unroll
      for (int j = 0; j < JB; ++j) {
        const int n = 4 * (k0 + j) + kq;
        b[j] = (valid && n < N) ? buf[base + n * S] : T(0);
        const T *hrow = h + n * ldh + col;        // H is symmetric: A[i][n] = H[n][i], 16 consecutive i per row n
#pragma unroll
        for (int it = 0; it < MT; ++it) a[j][it] = hrow[16 * it];
      }
#pragma unroll
      for (int j = 0; j < JB; ++j) {
#pragma unroll
        for (int it = 0; it < MT; ++it) acc[it] = M::run(a[j][it], b[j], acc[it]);
      }
    }
#pragma unroll
    for (int it = 0; it < MT; ++it) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = 16 * it + M::row(lane, r);
        if (valid && i < N) buf[base + i * S] = acc[it][r];
      }
    }
  }
  __syncthreads();
}

// buf <- T buf for `nv` fields of p.V sites that lie one behind the other.
template <typename T>
__device__ __forceinline__ void transform(T *buf, const T *hm, const HartleyAxes &p, int nv, int nthreads) {
  for (int a = 0; a < 4; ++a) {
    const int N = p.n[a], lines = nv * (p.V / (N > 0 ? N : 1));
    const T *h = hm + p.hoff[a];
    if (N <= 1) continue;
    if (N <= 16) axis_pass<T, 1>(buf, h, p.ldh[a], N, p.stride[a], lines, nthreads);
    else if (N <= 32) axis_pass<T, 2>(buf, h, p.ldh[a], N, p.stride[a], lines, nthreads);
    else if (N <= 48) axis_pass<T, 3>(buf, h, p.ldh[a], N, p.stride[a], lines, nthreads);
    else axis_pass<T, 4>(buf, h, p.ldh[a], N, p.stride[a], lines, nthreads);
  }
}

}  // namespace nf

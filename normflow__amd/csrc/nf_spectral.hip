// nf_spectral.hip -- the power-spectrum filter of FFTNet_ / PSDBlock_ in the separable real Hartley basis, one launch,
// the sample resident in LDS between the axis passes; forward and VJP.
//
// Restates src/nn/scalar/fftflow_.py:98-176 (irfftn(rfftn(x) w, s = L)) and, with the zero-mode coefficient replaced,
// src/nn/scalar/psd_.py:17-57.  The weight w(k) = sigma(khat^2)^(-1/2) is even in every k_mu separately, so it is diagonal
// in the Hartley basis as well: with H_N[k, n] = (cos(2 pi k n / N) + sin(2 pi k n / N)) / sqrt(N) (real, symmetric,
// orthogonal) and T = H_{N_1} x ... x H_{N_d},
//     irfftn(rfftn(x) w, s = L) = T diag(w) T x        for every real x and any axis lengths, odd ones included.
// (T x)(0) = sum(x) / sqrt(V) is the number MeanFieldNet_ transforms: PSDBlock_ is this filter with that one coefficient
// replaced.
//
// The weight gradient.  gw_half[k] = sum_b sum_{k' folding onto k} (T g_b)(k') (T x_b)(k') is NOT, entry by entry, what
// autograd gives through rfftn: the Hartley modes of one symmetry orbit {(+-k_1, ..., +-k_d)} mix differently from the
// Fourier pairs {k, -k}.  The sums over each orbit agree (both bases span the same eigenspace), and every member of an
// orbit has the same khat^2, hence the same dw/dtheta: the gradient of every parameter BEHIND w (the spline of the inverse
// power spectrum, logy) is the same.  Compare parameter gradients, never the raw gw_half (it agrees only for d = 1).
//
// Layout.  A workgroup (4 waves) holds a PACK of P consecutive samples in LDS, (P, N_0, .., N_3) row-major, and walks the
// packs with a stride of the grid (persistent).  An axis pass over axis mu (length N, element stride S) sees the pack as
// P V / N lines; a wave takes 16 lines at a time as the 16 columns of v_mfma_{f32,f64}_16x16x4: B operand = the line
// values x[n], A operand = H[i][n] read from the matrix the workgroup built in LDS (double sincospi, rounded to the
// dtype; rows and columns zero-padded to the 16-tile, row stride chosen so that the four rows a wave reads sit in different
// banks), accumulators = all ceil(N / 16) output tiles of those lines, written back in place: a wave owns its lines, so a
// pass needs one barrier, at its end.  Tiny lattices pack several samples (P V / N_max >= 64 lines: a full tile per wave)
// up to 16 KiB; partial last packs and B = 1 run the same code with fewer lines.
#include "nf_spectral_core.h"

namespace nf {

constexpr int kSpecLdsBytes = 160 * 1024;     // LDS of a CU
constexpr int kSpecPackBytes = 16 * 1024;     // packs of small samples grow up to this
constexpr int kSpecGroups = 1024;             // workgroups of the filter (4 per CU)
constexpr int kSpecVjpGroups = 512;           // workgroups of the VJP: one partial gw_half each

struct SpecPlan : HartleyAxes {   // the axes and their matrices (nf_spectral_core.h), V = sites
  int Vh, nh;            // entries of w_half, N_last / 2 + 1
  int P;                 // samples per pack
  int vec;               // the field can move as 16-byte words
  int64_t B, packs;
  int grid;
  size_t lds;
};

struct SpecArgs {
  SpecPlan p;
  const void *x, *g, *w, *zero_new;
  void *y, *zero_old;
  double *partial;
  int zero_replaced;
};

// Strides, matrix layout (row stride: the 16-tile padding, plus 16 where that keeps the four rows a wave reads in different
// banks; equal lengths share one matrix), hsize and V from the lengths p.n.
void spectral_axes(HartleyAxes &p, const int n[4]) {
  int len[4];
  for (int a = 0; a < 4; ++a) len[a] = n[a];      // n may be p.n itself
  p.hsize = 0;
  int V = 1;
  for (int a = 3; a >= 0; --a) {
    p.n[a] = len[a];
    p.stride[a] = V;
    V *= len[a];
    p.ldh[a] = p.hoff[a] = 0;
  }
  p.V = V;
  for (int a = 0; a < 4; ++a) {
    if (p.n[a] == 1) continue;
    int same = -1;
    for (int c = 0; c < a; ++c)
      if (p.n[c] == p.n[a]) same = c;
    const int pad16 = (p.n[a] + 15) & ~15;
    p.ldh[a] = pad16 % 32 == 16 ? pad16 : pad16 + 16;
    if (same >= 0) {
      p.hoff[a] = p.hoff[same];
    } else {
      p.hoff[a] = p.hsize;
      p.hsize += pad16 * p.ldh[a];
    }
  }
}

static int make_plan(SpecPlan &p, const int32_t *lat, int ndim, int dtype, int for_vjp, int64_t B, const char *who) {
  NF_REQUIRE(lat != nullptr, "%s: NULL lattice", who);
  NF_REQUIRE(ndim >= 1 && ndim <= 4, "%s: %d lattice axes (1 to 4 are built)", who, ndim);
  NF_REQUIRE(dtype == NF_F32 || dtype == NF_F64, "%s: unsupported dtype %d (float32 and float64 fields)", who, dtype);
  NF_REQUIRE(B >= 0, "%s: bad batch %lld", who, (long long)B);
  p = SpecPlan{};
  int64_t V = 1;
  int nmax = 1;
  for (int a = 0; a < 4; ++a) {
    const int n = a < 4 - ndim ? 1 : lat[a - (4 - ndim)];
    NF_REQUIRE(n >= 1 && n <= kSpecMaxAxis, "%s: axis of %d sites (1 to %d fit the LDS-resident transform)", who, n,
               kSpecMaxAxis);
    p.n[a] = n;
    V *= n;
    nmax = n > nmax ? n : nmax;
  }
  const int64_t esize = dtype == NF_F32 ? 4 : 8;
  spectral_axes(p, p.n);
  const int64_t nbuf = for_vjp ? 2 : 1;
  NF_REQUIRE(nbuf * V * esize + p.hsize * esize <= kSpecLdsBytes,
             "%s: a sample of %lld sites (%lld B%s) and its Hartley matrices (%lld B) exceed the %d B of LDS; use "
             "transform='fft'", who, (long long)V, (long long)(nbuf * V * esize), for_vjp ? ", field and cotangent" : "",
             (long long)(p.hsize * esize), kSpecLdsBytes);
  p.nh = p.n[3] / 2 + 1;
  p.Vh = p.V / p.n[3] * p.nh;
  p.B = B;
  // pack rule: enough samples for 64 lines on the longest axis, more when the batch is far larger than the grid, within
  // kSpecPackBytes (and the LDS left beside the matrices); at least 1
  int64_t P = (64 * int64_t(nmax) + V - 1) / V;
  const int64_t spread = (B + kSpecGroups - 1) / kSpecGroups;
  P = P > spread ? P : spread;
  int64_t cap = kSpecPackBytes / (V * esize);
  const int64_t room = (kSpecLdsBytes - p.hsize * esize) / (nbuf * V * esize);
  cap = cap < room ? cap : room;
  P = P < cap ? P : cap;
  P = P < B ? P : B;
  p.P = int(P > 1 ? P : 1);
  p.packs = (B + p.P - 1) / p.P;
  const int64_t groups = for_vjp ? kSpecVjpGroups : kSpecGroups;
  p.grid = int(p.packs < groups ? p.packs : groups);
  p.lds = size_t(nbuf * p.P * V * esize + p.hsize * esize);
  p.vec = (V * esize) % 16 == 0;
  return NF_OK;
}

template <typename T>
__device__ __forceinline__ void copy_field(T *dst, const T *src, int ne, bool vec) {
  if (vec) {
    constexpr int W = 16 / sizeof(T);
    const uint4 *s4 = reinterpret_cast<const uint4 *>(src);
    uint4 *d4 = reinterpret_cast<uint4 *>(dst);
    for (int i = threadIdx.x; i < ne / W; i += kBlock) d4[i] = s4[i];
  } else {
    for (int i = threadIdx.x; i < ne; i += kBlock) dst[i] = src[i];
  }
}

// VJP = false: y_b = T D_b T x_b.  VJP = true: gx_b = T D_b T g_b (mode 0 dropped when zero_replaced), gzero[b] = (T g_b)(0)
// written through A.zero_old, and partial[workgroup][k] = the workgroup's share of gw_half[k].
template <typename T, bool VJP>
__global__ __launch_bounds__(kBlock, 4) void spectral_kernel(SpecArgs A) {
  extern __shared__ __align__(16) unsigned char spec_lds[];
  const SpecPlan &p = A.p;
  T *hm = reinterpret_cast<T *>(spec_lds);
  T *buf = hm + p.hsize;
  T *buf2 = buf + p.P * p.V;                      // VJP only: T x
  const T *__restrict__ w = static_cast<const T *>(A.w);
  const T *zero_new = static_cast<const T *>(A.zero_new);
  T *zero_old = static_cast<T *>(A.zero_old);
  const int V = p.V, n3 = p.n[3], nh = p.nh;
  build_hartley(hm, p, kBlock);
  __syncthreads();
  for (int64_t pk = blockIdx.x; pk < p.packs; pk += gridDim.x) {
    const int64_t b0 = pk * p.P;
    const int nv = int(p.B - b0 < p.P ? p.B - b0 : p.P), ne = nv * V;
    copy_field(buf, static_cast<const T *>(VJP ? A.g : A.x) + b0 * V, ne, p.vec);
    if (VJP) copy_field(buf2, static_cast<const T *>(A.x) + b0 * V, ne, p.vec);
    __syncthreads();
    transform(buf, hm, p, nv, kBlock);
    if (VJP) {
      transform(buf2, hm, p, nv, kBlock);
      double *part = A.partial + int64_t(blockIdx.x) * p.Vh;
      const bool first = pk == blockIdx.x;
      for (int kh = threadIdx.x; kh < p.Vh; kh += kBlock) {
        const int rest = kh / nh, kf = kh - rest * nh;
        const int v1 = rest * n3 + kf;
        const int v2 = (kf != 0 && 2 * kf != n3) ? rest * n3 + n3 - kf : -1;     // the other mode that folds onto kf
        double acc = 0.0;
        for (int s = 0; s < nv; ++s) {
          acc += double(buf[s * V + v1]) * double(buf2[s * V + v1]);
          if (v2 >= 0) acc += double(buf[s * V + v2]) * double(buf2[s * V + v2]);
        }
        if (kh == 0 && A.zero_replaced) acc = 0.0;
        part[kh] = first ? acc : part[kh] + acc;       // the workgroup's own row: same thread, same order every run
      }
      __syncthreads();
    }
    for (int v = threadIdx.x; v < V; v += kBlock) {
      const int rest = v / n3, k3 = v - rest * n3;
      const T wv = w[rest * nh + (k3 < n3 - k3 ? k3 : n3 - k3)];
      for (int s = 0; s < nv; ++s) {
        T c = buf[s * V + v];
        if (v == 0) {
          if (zero_old) zero_old[b0 + s] = c;
          if (VJP) c = A.zero_replaced ? T(0) : c * wv;
          else c = zero_new ? zero_new[b0 + s] : c * wv;
        } else {
          c *= wv;
        }
        buf[s * V + v] = c;
      }
    }
    __syncthreads();
    transform(buf, hm, p, nv, kBlock);
    copy_field(static_cast<T *>(A.y) + b0 * V, buf, ne, p.vec);
    __syncthreads();                 // the next pack's load overwrites what this store reads
  }
}

// gw_half[k] = the sum of the workgroups' partials in a fixed order: 16 modes per workgroup, 16 threads per mode that sum
// the partials j = slice, slice + 16, ... each, then the 16 slices in order.
template <typename T>
__global__ __launch_bounds__(kBlock) void spectral_reduce_kernel(const double *__restrict__ part, int groups, int Vh,
                                                                 T *__restrict__ gw) {
  __shared__ double slices[16][17];
  const int m = threadIdx.x & 15, slice = threadIdx.x >> 4;
  const int kh = blockIdx.x * 16 + m;
  double acc = 0.0;
  if (kh < Vh)
    for (int j = slice; j < groups; j += 16) acc += part[int64_t(j) * Vh + kh];
  slices[slice][m] = acc;
  __syncthreads();
  if (slice == 0 && kh < Vh) {
    double tot = 0.0;
#pragma unroll
    for (int j = 0; j < 16; ++j) tot += slices[j][m];
    gw[kh] = T(tot);
  }
}

template <typename T, bool VJP>
static int launch_spectral(const SpecArgs &A, hipStream_t s) {
  auto kern = spectral_kernel<T, VJP>;
  if (A.p.lds > 64 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                          int(A.p.lds)) != hipSuccess) {
    (void)hipGetLastError();
    set_error("spectral kernel: cannot raise the dynamic LDS limit to %zu B", A.p.lds);
    return NF_ELAUNCH;
  }
  hipLaunchKernelGGL(kern, dim3(unsigned(A.p.grid)), dim3(kBlock), A.p.lds, s, A);
  return check_launch(VJP ? "spectral vjp kernel" : "spectral kernel");
}

static bool aligned16(const void *q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

}  // namespace nf

using namespace nf;

extern "C" int nf_spectral_supported(const int32_t *lat, int ndim, int dtype, int for_vjp) {
  SpecPlan p;
  return make_plan(p, lat, ndim, dtype, for_vjp, 1, "nf_spectral_supported") == NF_OK ? 1 : 0;
}

extern "C" size_t nf_spectral_workspace_bytes(const int32_t *lat, int ndim, int64_t B, int dtype) {
  SpecPlan p;
  if (make_plan(p, lat, ndim, dtype, 1, B, "nf_spectral_workspace_bytes")) return 0;
  return size_t(p.grid) * size_t(p.Vh) * sizeof(double);
}

extern "C" int nf_spectral_filter(const void *x, const void *w_half, const void *zero_new, void *y, void *zero_old,
                                  const int32_t *lat, int ndim, int64_t B, int dtype, void *stream) {
  SpecArgs A{};
  int rc = make_plan(A.p, lat, ndim, dtype, 0, B, "nf_spectral_filter");
  if (rc) return rc;
  NF_REQUIRE(x && w_half && y, "nf_spectral_filter: NULL tensor pointer");
  if (B == 0) return NF_OK;
  A.x = x; A.w = w_half; A.zero_new = zero_new; A.y = y; A.zero_old = zero_old;
  A.p.vec = A.p.vec && aligned16(x) && aligned16(y);
  hipStream_t s = static_cast<hipStream_t>(stream);
  return dtype == NF_F32 ? launch_spectral<float, false>(A, s) : launch_spectral<double, false>(A, s);
}

extern "C" int nf_spectral_filter_vjp(const void *x, const void *g, const void *w_half, int zero_replaced, void *gx,
                                      void *gw_half, void *gzero, void *workspace, size_t workspace_bytes,
                                      const int32_t *lat, int ndim, int64_t B, int dtype, void *stream) {
  SpecArgs A{};
  int rc = make_plan(A.p, lat, ndim, dtype, 1, B, "nf_spectral_filter_vjp");
  if (rc) return rc;
  NF_REQUIRE(x && g && w_half && gx && gw_half, "nf_spectral_filter_vjp: NULL tensor pointer");
  const size_t need = size_t(A.p.grid) * size_t(A.p.Vh) * sizeof(double);
  if (need && (workspace == nullptr || workspace_bytes < need)) {
    set_error("nf_spectral_filter_vjp: workspace %zu B < %zu B needed", workspace_bytes, need);
    return NF_EWORKSPACE;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  A.x = x; A.g = g; A.w = w_half; A.y = gx; A.zero_old = gzero; A.zero_replaced = zero_replaced != 0;
  A.partial = static_cast<double *>(workspace);
  A.p.vec = A.p.vec && aligned16(x) && aligned16(g) && aligned16(gx);
  if (B > 0) {
    rc = dtype == NF_F32 ? launch_spectral<float, true>(A, s) : launch_spectral<double, true>(A, s);
    if (rc) return rc;
  }
  const unsigned blocks = unsigned((A.p.Vh + 15) / 16);
  if (dtype == NF_F32)
    hipLaunchKernelGGL(spectral_reduce_kernel<float>, dim3(blocks), dim3(kBlock), 0, s, A.partial, A.p.grid, A.p.Vh,
                       static_cast<float *>(gw_half));
  else
    hipLaunchKernelGGL(spectral_reduce_kernel<double>, dim3(blocks), dim3(kBlock), 0, s, A.partial, A.p.grid, A.p.Vh,
                       static_cast<double *>(gw_half));
  return check_launch("spectral reduce kernel");
}

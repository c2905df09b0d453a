// nf_pade.hip -- Pade11_ / Pade22_: learnable monotone maps of [0, 1] onto itself with per-channel parameters, forward,
// inverse and their VJP, each one pass over the field; and on the same pass the site-local maps of the real line:
// Tanh_ / ArcTanh_ (no parameters) and Pade32_ (one parameter per channel).
//
// Restates src/nn/scalar/modules_.py:117-222 (the reference's ~15 eager element-wise ops plus the reduction of
// Module_.sum_density, src/nn/_core.py:38-42, per direction):
//   Pade11_  f(x) = x / (x + d (1 - x)),                            log f' = log d - 2 log(x + d (1 - x));
//            inverse: x / (x + (1 - x) / d),                        log    = -log d - 2 log(x + (1 - x) / d)
//   Pade22_  f(x) = x (x + d0 (1 - x)) / (1 + s x (1 - x)),  s = d0 + d1 - 2,
//            g1 = f' = (d0 + 2 (1 - d0) x + s x^2) / (1 + s x (1 - x))^2;
//            inverse: the root x = 2y / (-b + sqrt(b^2 - 4 a y)), b = s y - d0, a = -1 - b: the reference's
//            (-b - sqrt(..)) / (2a) without its a == 0 branch (:204), and log = -log g1(x) at that x.
// No clamping: inputs outside [0, 1] give what the formulas give.
//   Tanh_    y = tanh x, log f' = -2 log cosh x = -2 (|x| + log1p(e^{-2|x|}) - ln 2)   (modules_.py:72-90: the reference's
//            log(cosh x) overflows to inf; this form is finite for every finite x and equal wherever that one is finite);
//            inverse (ArcTanh_): atanh y, log = -log(1 - y^2) = -(log1p(y) + log1p(-y)).
//   Pade32_  f(x) = x (a + x^2) / (1 + a x^2), 0 < a < 3 (modules_.py:225-274): odd, monotone, fixed points 0 and +-1;
//            f' = (a (s - 1)^2 + (3 - a)(1 + a) s) / (1 + a s)^2, s = x^2: the reference's numerator a s^2 + (3 - a^2) s + a
//            as a sum of two non-negative terms.  For |x| > 1 both are evaluated in u = 1/x, so nothing overflows.
//            inverse: the one real root of x^3 - a y x^2 + a x - y = 0 (see pade32_root), log = -log f'(x) at that root.
//
// Layout.  The field is (outer, C, inner): rows of `inner` elements, row r has channel r % C, and a sample is RS =
// outer C / B whole rows.  A work unit is (sample b, row group g, piece bx): group g holds the rows g, g + G, ... of the
// sample, which all have ONE channel (G = C when C divides RS -- channels_axis >= 1; G = 1 when RS == 1 -- channels_axis
// 0, where the channel is the sample).  So a unit reads its channel's parameters once, its log-det partial belongs to one
// sample and its parameter-cotangent partial to one channel: both reductions are fixed-order, with no atomics, and the
// results are bitwise reproducible.  Element offsets are 64-bit.
#include "nf_internal.h"

namespace nf {

constexpr int kPadeUnroll = 4;                 // loads a thread issues before it uses the first (memory-level parallelism)
constexpr int64_t kPadeTargetUnits = 32768;    // 128 workgroups per CU: enough to stream; few partials to reduce

struct PadePlan {
  int64_t B, C, inner;
  int64_t RS;         // rows per sample
  int64_t G;          // row groups per sample (one channel each)
  int64_t P;          // element stride between consecutive rows of a group: G * inner
  int64_t nk;         // elements per (sample, group): RS / G * inner
  int64_t chunk;      // elements per unit: kBlock * iters
  int64_t blocks_x;   // units per (sample, group)
  int64_t units;      // B * G * blocks_x; unit u = (b * blocks_x + bx) * G + g
  int64_t step_q, step_r;   // a thread's step of kBlock elements inside a group: step_q rows and step_r elements
};

struct PadeArgs {
  PadePlan p;
  const void *x, *d0, *d1, *log0, *grad_y, *grad_logj;
  void *y, *logj, *grad_x;
  double *partial;    // map: one double per unit (per-sample mode); vjp: two per unit
};

static int make_plan(PadePlan &p, int64_t B, int64_t outer, int64_t C, int64_t inner, const char *who) {
  NF_REQUIRE(B >= 0 && outer >= 0 && C >= 1 && inner >= 0, "%s: bad sizes B=%lld outer=%lld C=%lld inner=%lld", who,
             (long long)B, (long long)outer, (long long)C, (long long)inner);
  p = PadePlan{};
  p.B = B; p.C = C; p.inner = inner; p.G = 1;
  if (B == 0) return NF_OK;
  NF_REQUIRE((outer * C) % B == 0, "%s: a sample must be whole rows (B=%lld does not divide outer*C=%lld)", who,
             (long long)B, (long long)(outer * C));
  p.RS = outer * C / B;
  NF_REQUIRE(p.RS % C == 0 || p.RS == 1, "%s: rows per sample %lld is neither a multiple of C=%lld nor 1", who,
             (long long)p.RS, (long long)C);
  p.G = (p.RS % C == 0) ? C : 1;
  p.P = p.G * inner;
  p.nk = p.RS / p.G * inner;
  if (p.nk == 0) return NF_OK;
  int64_t iters = 1;
  while (int64_t(kBlock) * iters < p.nk &&
         B * p.G * ((p.nk + kBlock * iters - 1) / (kBlock * iters)) > kPadeTargetUnits)
    iters *= 2;
  p.chunk = kBlock * iters;
  p.blocks_x = (p.nk + p.chunk - 1) / p.chunk;
  p.units = B * p.G * p.blocks_x;
  p.step_q = kBlock / inner;
  p.step_r = kBlock % inner;
  return NF_OK;
}

// The unit's (sample, first row, channel) and a thread's walk over its group: element k of the group (k = m inner + i)
// sits at m P + i from the group's first element.
struct PadeUnit {
  int64_t b, row0, c, k, kend;
  __device__ PadeUnit(const PadePlan &p, int64_t u) {
    const int64_t g = u % p.G, rest = u / p.G, bx = rest % p.blocks_x;
    b = rest / p.blocks_x;
    row0 = b * p.RS + g;
    c = row0 % p.C;
    k = bx * p.chunk + threadIdx.x;
    kend = bx * p.chunk + p.chunk < p.nk ? bx * p.chunk + p.chunk : p.nk;
  }
};

struct PadeWalk {
  int64_t off, i;
  __device__ PadeWalk(const PadePlan &p, int64_t k) {
    const int64_t m = k / p.inner;
    i = k - m * p.inner;
    off = m * p.P + i;
  }
  __device__ __forceinline__ void step(const PadePlan &p) {
    i += p.step_r;
    off += p.step_q * p.P + p.step_r;
    if (i >= p.inner) {
      i -= p.inner;
      off += p.P - p.inner;
    }
  }
};

template <typename T> struct RealFn;
template <> struct RealFn<float> {
  static __device__ __forceinline__ float tanh(float x) { return ::tanhf(x); }
  static __device__ __forceinline__ float atanh(float x) { return ::atanhf(x); }
  static __device__ __forceinline__ float log1p(float x) { return ::log1pf(x); }
  static __device__ __forceinline__ float exp(float x) { return ::expf(x); }
  static __device__ __forceinline__ float cbrt(float x) { return ::cbrtf(x); }
  static __device__ __forceinline__ float copysign(float x, float s) { return ::copysignf(x, s); }
};
template <> struct RealFn<double> {
  static __device__ __forceinline__ double tanh(double x) { return ::tanh(x); }
  static __device__ __forceinline__ double atanh(double x) { return ::atanh(x); }
  static __device__ __forceinline__ double log1p(double x) { return ::log1p(x); }
  static __device__ __forceinline__ double exp(double x) { return ::exp(x); }
  static __device__ __forceinline__ double cbrt(double x) { return ::cbrt(x); }
  static __device__ __forceinline__ double copysign(double x, double s) { return ::copysign(x, s); }
};

// Pade32_: f(x) and f'(x) > 0.  |x| <= 1 in s = x^2, |x| > 1 in r = 1 / x^2 (numerator and denominator divided by s or
// s^2), so both stay finite up to the largest x.  ie = 1 / (1 + a s) in either form: f(x) - y = N ie with
// N = x (a + s) - y (1 + a s).
template <typename T> __device__ __forceinline__ void pade32_eval(T x, T a, T &f, T &g, T &ie) {
  const T k = (T(3) - a) * (T(1) + a);
  if (Num<T>::abs(x) <= T(1)) {
    const T s = x * x, iden = T(1) / (T(1) + a * s), w = (x - T(1)) * (x + T(1));
    f = x * (a + s) * iden;
    g = (a * w * w + k * s) * (iden * iden);
    ie = iden;
  } else {
    const T u = T(1) / x, r = u * u, iden = T(1) / (r + a), w = (T(1) - u) * (T(1) + u);
    f = x * (a * r + T(1)) * iden;
    g = (a * w * w + k * r) * (iden * iden);
    ie = r * iden;
  }
}

// One Newton step on f(x) - y.  The step cannot move x below the noise of the residual over f', and f' is as small as
// (3 - a) / (1 + a) at |x| = 1; in fp32 the residual's numerator N is therefore formed in double (exact products of fp32
// operands, five operations), which leaves the root within an ulp or so of the exact root of the fp32 inputs.
template <typename T> __device__ __forceinline__ T pade32_newton(T x, T a, T y) {
  T f, g, ie;
  pade32_eval(x, a, f, g, ie);
  if constexpr (sizeof(T) == sizeof(float)) {
    const double xd = x, ad = a, s = xd * xd;
    const double N = xd * (ad + s) - double(y) * (1.0 + ad * s);
    return x - T(N * double(ie)) / g;
  } else {
    return x - (f - y) / g;
  }
}

// The one real root of x^3 - a y x^2 + a x - y = 0 for 0 < a < 3: odd in y, 0 at 0.  |y| <= 1: the cubic in x; |y| > 1:
// the cubic in z = x / y, z^3 - a z^2 + (a / y^2) z - 1 / y^2 = 0, whose coefficients are bounded.  Either is depressed
// (shift h = -A2 / 3: t^3 + p t + q = 0) and solved by Cardano with the larger-magnitude cube root U of -q/2 +- sqrt(D)
// and the other term as -p / (3U); D < 0 can only come from rounding near the almost-triple root (a -> 3, |y| = 1) and is
// clamped.  Two Newton steps on f(x) - y remove the cancellation of U + V (x < 1) and of D; where y^2 < 1e-4 a^3 the root's
// series y/a - (1 - a^2) (y/a)^3 / a (relative error < 1e-8) starts them instead, so tiny y keep their relative accuracy.
template <typename T> __device__ __forceinline__ T pade32_root(T y, T a) {
  const T ay = Num<T>::abs(y);
  if (!(ay > T(0))) return y;                      // +-0 (and NaN) map to themselves
  T A2, A1, A0, scale;
  if (ay <= T(1)) {
    A2 = -a * ay; A1 = a; A0 = -ay; scale = T(1);
  } else {
    const T c = (T(1) / ay) / ay;
    A2 = -a; A1 = a * c; A0 = -c; scale = ay;
  }
  const T h = -A2 * T(1.0 / 3.0);
  const T p = A1 - A2 * A2 * T(1.0 / 3.0);
  const T q = A2 * (T(2.0 / 27.0) * A2 * A2 - A1 * T(1.0 / 3.0)) + A0;
  const T hq = T(-0.5) * q, p3 = p * T(1.0 / 3.0);
  const T D = Num<T>::max(hq * hq + p3 * p3 * p3, T(0));
  const T U = RealFn<T>::cbrt(hq + RealFn<T>::copysign(Num<T>::sqrt(D), hq));
  const T t = U != T(0) ? U - p3 / U : T(0);
  T x = (t + h) * scale;
  if (ay * ay < T(1e-4) * a * a * a) {             // x << sqrt(a): U + V would cancel to noise; the series of the root
    const T z = ay / a;
    x = z - (T(1) - a * a) * z * z * z / a;
  }
  x = pade32_newton(pade32_newton(x, a, ay), a, ay);
  return RealFn<T>::copysign(x, y);
}

// The map at one element.  d is (d0, d1) for Pade22_, (d, log d) for Pade11_ and (a, -) for Pade32_; Tanh_ has none.
template <typename T, int KIND, bool INV>
__device__ __forceinline__ T pade_map(T v, T d0, T d1, T &lg) {
  if constexpr (KIND == NF_TANH) {
    if (INV) {
      lg = -(RealFn<T>::log1p(v) + RealFn<T>::log1p(-v));
      return RealFn<T>::atanh(v);
    }
    const T ax = Num<T>::abs(v);
    lg = T(-2) * ((ax - Num<T>::kLn2) + RealFn<T>::log1p(RealFn<T>::exp(T(-2) * ax)));
    return RealFn<T>::tanh(v);
  } else if constexpr (KIND == NF_PADE32) {
    const T x = INV ? pade32_root(v, d0) : v;
    T f, g, ie;
    pade32_eval(x, d0, f, g, ie);
    lg = INV ? -nf_log(g) : nf_log(g);
    return INV ? x : f;
  } else if constexpr (KIND == NF_PADE11) {
    const T den = INV ? v + (T(1) - v) / d0 : v + d0 * (T(1) - v);
    lg = (INV ? -d1 : d1) - T(2) * nf_log(den);
    return v / den;
  } else {
    const T s = d0 + d1 - T(2);
    T x = v;
    if (INV) {
      const T b = s * v - d0, a = T(-1) - b;
      x = T(2) * v / (-b + Num<T>::sqrt(b * b - T(4) * a * v));
    }
    const T den = T(1) + s * x * (T(1) - x);
    const T g1 = (d0 + T(2) * (T(1) - d0) * x + s * x * x) / (den * den);
    lg = INV ? -nf_log(g1) : nf_log(g1);
    return INV ? x : x * (x + d0 * (T(1) - x)) / den;
  }
}

template <typename T, int KIND, bool INV, bool SITES>
__global__ __launch_bounds__(kBlock) void pade_kernel(PadeArgs A) {
  __shared__ double red[kBlock / kWave];
  const PadePlan &p = A.p;
  for (int64_t u = blockIdx.x; u < p.units; u += gridDim.x) {
    PadeUnit U(p, u);
    T d0 = T(0), d1 = T(0);
    if constexpr (KIND != NF_TANH) d0 = static_cast<const T *>(A.d0)[U.c];
    if constexpr (KIND == NF_PADE11) d1 = nf_log(d0);
    if constexpr (KIND == NF_PADE22) d1 = static_cast<const T *>(A.d1)[U.c];
    const int64_t base = U.row0 * p.inner;
    const T *__restrict__ xin = static_cast<const T *>(A.x) + base;
    const T *__restrict__ l0 = SITES && A.log0 ? static_cast<const T *>(A.log0) + base : nullptr;
    T *__restrict__ out = static_cast<T *>(A.y) + base;
    T *__restrict__ site = SITES ? static_cast<T *>(A.logj) + base : nullptr;
    double acc = 0.0;
    PadeWalk w(p, U.k < U.kend ? U.k : 0);
    int64_t k = U.k;
    while (k < U.kend) {
      int64_t o[kPadeUnroll];
      T v[kPadeUnroll], l[kPadeUnroll];
#pragma unroll
      for (int j = 0; j < kPadeUnroll; ++j) {
        o[j] = -1;
        if (k < U.kend) {
          o[j] = w.off;
          v[j] = xin[w.off];
          if (SITES) l[j] = l0 ? l0[w.off] : T(0);
          k += kBlock;
          w.step(p);
        }
      }
#pragma unroll
      for (int j = 0; j < kPadeUnroll; ++j) {
        if (o[j] < 0) break;
        T lg;
        out[o[j]] = pade_map<T, KIND, INV>(v[j], d0, d1, lg);
        if (SITES) site[o[j]] = l[j] + lg;
        else acc += double(lg);
      }
    }
    if (!SITES) {
      const double tot = block_sum(acc, red);
      if (threadIdx.x == 0) A.partial[u] = tot;
      __syncthreads();              // thread 0 has read `red` before the next unit's waves write it
    }
  }
}

// VJP at one element.  x is the x-side point (forward input / inverse output): the forward map's partials there give both
// directions (inverse: implicit differentiation, as nf_distconv_vjp), so no root is recomputed.
template <typename T, int KIND, bool INV>
__device__ __forceinline__ T pade_vjp(T x, T d0, T d1, T gy, T gl, double &gd0, double &gd1) {
  T g, Lx, f0 = T(0), L0 = T(0), f1 = T(0), L1 = T(0);
  if constexpr (KIND == NF_TANH) {
    // e = e^{-2|x|}: sech^2 x = 4e / (1 + e)^2 does not cancel where tanh x rounds to +-1
    const T e = RealFn<T>::exp(T(-2) * Num<T>::abs(x)), ie = T(1) / (T(1) + e);
    g = T(4) * e * ie * ie;
    Lx = T(-2) * RealFn<T>::tanh(x);
  } else if constexpr (KIND == NF_PADE32) {
    // in s = x^2 (|x| <= 1) or r = 1 / x^2 (|x| > 1), as pade32_eval: num = a s^2 + (3 - a^2) s + a, den = 1 + a s
    const T a = d0, k = (T(3) - a) * (T(1) + a);
    if (Num<T>::abs(x) <= T(1)) {
      const T s = x * x, iden = T(1) / (T(1) + a * s), i2 = iden * iden, w = (x - T(1)) * (x + T(1));
      const T num = a * w * w + k * s, inum = T(1) / num;
      g = num * i2;
      Lx = T(2) * x * ((T(2) * a * s + T(3) - a * a) * inum - T(2) * a * iden);
      f0 = -x * w * (T(1) + s) * i2;
      L0 = (s * s - T(2) * a * s + T(1)) * inum - T(2) * s * iden;
    } else {
      const T u = T(1) / x, r = u * u, iden = T(1) / (r + a), i2 = iden * iden, w = (T(1) - u) * (T(1) + u);
      const T num = a * w * w + k * r, inum = T(1) / num;
      g = num * i2;
      Lx = T(2) * u * ((T(2) * a + (T(3) - a * a) * r) * inum - T(2) * a * iden);
      f0 = -x * w * (T(1) + r) * i2;
      L0 = (T(1) - T(2) * a * r + r * r) * inum - T(2) * iden;
    }
  } else if constexpr (KIND == NF_PADE11) {
    const T den = x + d0 * (T(1) - x), iden = T(1) / den, i2 = iden * iden;
    g = d0 * i2;
    Lx = -T(2) * (T(1) - d0) * iden;
    f0 = -x * (T(1) - x) * i2;
    L0 = T(1) / d0 - T(2) * (T(1) - x) * iden;
  } else {
    const T s = d0 + d1 - T(2), t = x * (T(1) - x);
    const T den = T(1) + s * t, iden = T(1) / den, i2 = iden * iden;
    const T num = x * (x + d0 * (T(1) - x));
    const T n1 = d0 + T(2) * (T(1) - d0) * x + s * x * x, in1 = T(1) / n1;
    g = n1 * i2;
    Lx = T(2) * ((T(1) - d0) + s * x) * in1 - T(2) * s * (T(1) - T(2) * x) * iden;
    f0 = t * (den - num) * i2;
    f1 = -num * t * i2;
    L0 = (T(1) - x) * (T(1) - x) * in1 - T(2) * t * iden;
    L1 = x * x * in1 - T(2) * t * iden;
  }
  T gin, gq, gL;
  if (!INV) {
    gin = gy * g + gl * Lx;
    gq = gy; gL = gl;
  } else {
    gin = (gy - gl * Lx) / g;
    gq = -gin; gL = -gl;
  }
  if (KIND != NF_TANH) gd0 += double(gq * f0 + gL * L0);
  if (KIND == NF_PADE22) gd1 += double(gq * f1 + gL * L1);
  return gin;
}

template <typename T, int KIND, bool INV, bool SITES>
__global__ __launch_bounds__(kBlock) void pade_vjp_kernel(PadeArgs A) {
  __shared__ double red[kBlock / kWave];
  const PadePlan &p = A.p;
  for (int64_t u = blockIdx.x; u < p.units; u += gridDim.x) {
    PadeUnit U(p, u);
    const T d0 = KIND != NF_TANH ? static_cast<const T *>(A.d0)[U.c] : T(0);
    const T d1 = KIND == NF_PADE22 ? static_cast<const T *>(A.d1)[U.c] : T(0);
    const int64_t base = U.row0 * p.inner;
    const T *__restrict__ xin = static_cast<const T *>(A.x) + base;
    const T *__restrict__ gyp = static_cast<const T *>(A.grad_y) + base;
    const T *__restrict__ glp = static_cast<const T *>(A.grad_logj) + (SITES ? base : U.b);
    T *__restrict__ gx = static_cast<T *>(A.grad_x) + base;
    const T gl_sample = SITES ? T(0) : glp[0];
    double gd0 = 0.0, gd1 = 0.0;
    PadeWalk w(p, U.k < U.kend ? U.k : 0);
    int64_t k = U.k;
    while (k < U.kend) {
      int64_t o[kPadeUnroll];
      T v[kPadeUnroll], gy[kPadeUnroll], gl[kPadeUnroll];
#pragma unroll
      for (int j = 0; j < kPadeUnroll; ++j) {
        o[j] = -1;
        if (k < U.kend) {
          o[j] = w.off;
          v[j] = xin[w.off];
          gy[j] = gyp[w.off];
          gl[j] = SITES ? glp[w.off] : gl_sample;
          k += kBlock;
          w.step(p);
        }
      }
#pragma unroll
      for (int j = 0; j < kPadeUnroll; ++j) {
        if (o[j] < 0) break;
        gx[o[j]] = pade_vjp<T, KIND, INV>(v[j], d0, d1, gy[j], gl[j], gd0, gd1);
      }
    }
    const double t0 = block_sum(gd0, red);
    __syncthreads();
    const double t1 = block_sum(gd1, red);
    if (threadIdx.x == 0) {
      A.partial[2 * u] = t0;
      A.partial[2 * u + 1] = t1;
    }
    __syncthreads();
  }
}

// Stage 2: grad_d[c] and grad_d[C + c] = the sums of the partials of channel c's units, in a fixed order.
__global__ __launch_bounds__(kBlock) void pade_channel_reduce_kernel(PadePlan p, const double *__restrict__ part,
                                                                     double *__restrict__ grad_d) {
  __shared__ double red[kBlock / kWave];
  const int64_t c = blockIdx.x;
  // units of channel c: G == C -> g = c for every (b, bx); G == 1 -> the samples b with b % C == c (RS == 1 or C == 1)
  const int64_t nb = p.B == 0 ? 0 : (p.G == p.C ? p.B : (p.B - c + p.C - 1) / p.C);
  const int64_t n = nb * p.blocks_x;
  double a0 = 0.0, a1 = 0.0;
  for (int64_t j = threadIdx.x; j < n; j += kBlock) {
    int64_t u;
    if (p.G == p.C) {
      u = j * p.G + c;
    } else {
      const int64_t q = j / p.blocks_x;
      u = (c + q * p.C) * p.blocks_x + (j - q * p.blocks_x);
    }
    a0 += part[2 * u];
    a1 += part[2 * u + 1];
  }
  const double t0 = block_sum(a0, red);
  __syncthreads();
  const double t1 = block_sum(a1, red);
  if (threadIdx.x == 0) {
    grad_d[c] = t0;
    grad_d[p.C + c] = t1;
  }
}

static unsigned pade_grid(const PadePlan &p) { return unsigned(p.units < kMaxBlocksX ? p.units : kMaxBlocksX); }

template <typename T, int KIND, bool INV>
static void launch_map(const PadeArgs &A, bool sites, hipStream_t s) {
  if (sites) hipLaunchKernelGGL((pade_kernel<T, KIND, INV, true>), dim3(pade_grid(A.p)), dim3(kBlock), 0, s, A);
  else hipLaunchKernelGGL((pade_kernel<T, KIND, INV, false>), dim3(pade_grid(A.p)), dim3(kBlock), 0, s, A);
}

template <typename T, int KIND, bool INV>
static void launch_vjp(const PadeArgs &A, bool sites, hipStream_t s) {
  if (sites) hipLaunchKernelGGL((pade_vjp_kernel<T, KIND, INV, true>), dim3(pade_grid(A.p)), dim3(kBlock), 0, s, A);
  else hipLaunchKernelGGL((pade_vjp_kernel<T, KIND, INV, false>), dim3(pade_grid(A.p)), dim3(kBlock), 0, s, A);
}

template <typename T, int KIND>
static void dispatch_kind(bool vjp, const PadeArgs &A, int inverse, bool st, hipStream_t s) {
  if (vjp) inverse ? launch_vjp<T, KIND, true>(A, st, s) : launch_vjp<T, KIND, false>(A, st, s);
  else inverse ? launch_map<T, KIND, true>(A, st, s) : launch_map<T, KIND, false>(A, st, s);
}

template <typename T>
static void dispatch(bool vjp, const PadeArgs &A, int kind, int inverse, int per_site, hipStream_t s) {
  const bool st = per_site != 0;
  switch (kind) {
    case NF_TANH: dispatch_kind<T, NF_TANH>(vjp, A, inverse, st, s); break;
    case NF_PADE11: dispatch_kind<T, NF_PADE11>(vjp, A, inverse, st, s); break;
    case NF_PADE22: dispatch_kind<T, NF_PADE22>(vjp, A, inverse, st, s); break;
    default: dispatch_kind<T, NF_PADE32>(vjp, A, inverse, st, s); break;
  }
}

static int check_common(const char *who, int kind, int dtype, const void *x, const void *d0, const void *d1,
                        int64_t C) {
  NF_REQUIRE(kind == NF_TANH || kind == NF_PADE11 || kind == NF_PADE22 || kind == NF_PADE32,
             "%s: kind %d is none of NF_TANH, NF_PADE11, NF_PADE22, NF_PADE32", who, kind);
  NF_REQUIRE(dtype == NF_F32 || dtype == NF_F64, "%s: unsupported dtype %d", who, dtype);
  NF_REQUIRE(x && (d0 || kind == NF_TANH) && (d1 || kind != NF_PADE22), "%s: NULL tensor pointer", who);
  NF_REQUIRE(kind != NF_TANH || C == 1, "%s: NF_TANH has no channels (C=%lld, must be 1)", who, (long long)C);
  return NF_OK;
}

}  // namespace nf

using namespace nf;

extern "C" size_t nf_pade_workspace_bytes(int64_t B, int64_t outer, int64_t C, int64_t inner) {
  PadePlan p;
  if (make_plan(p, B, outer, C, inner, "nf_pade_workspace_bytes")) return 0;
  return size_t(p.units) * 2 * sizeof(double);
}

extern "C" int nf_pade(const void *x, const void *d0, const void *d1, const void *log0, void *y, void *logj, int64_t B,
                       int64_t outer, int64_t C, int64_t inner, int kind, int inverse, int per_site, void *workspace,
                       size_t workspace_bytes, int dtype, void *stream) {
  int rc = check_common("nf_pade", kind, dtype, x, d0, d1, C);
  if (rc) return rc;
  NF_REQUIRE(y && logj, "nf_pade: NULL tensor pointer");
  PadeArgs A{};
  rc = make_plan(A.p, B, outer, C, inner, "nf_pade");
  if (rc) return rc;
  const size_t need = per_site ? 0 : size_t(A.p.units) * sizeof(double);
  if (need && (workspace == nullptr || workspace_bytes < need)) {
    set_error("nf_pade: workspace %zu B < %zu B needed", workspace_bytes, need);
    return NF_EWORKSPACE;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  A.x = x; A.d0 = d0; A.d1 = d1; A.log0 = log0; A.y = y; A.logj = logj;
  A.partial = static_cast<double *>(workspace);
  if (A.p.units > 0) {
    if (dtype == NF_F32) dispatch<float>(false, A, kind, inverse, per_site, s);
    else dispatch<double>(false, A, kind, inverse, per_site, s);
    rc = check_launch("pade kernel");
    if (rc || per_site) return rc;
  } else if (per_site) {
    return NF_OK;
  }
  const int64_t n_part = A.p.G * A.p.blocks_x;
  return dtype == NF_F32 ? launch_finalize<float>(A.partial, n_part, log0, logj, B, s)
                         : launch_finalize<double>(A.partial, n_part, log0, logj, B, s);
}

extern "C" int nf_pade_vjp(const void *x, const void *d0, const void *d1, const void *grad_y, const void *grad_logj,
                           void *grad_x, double *grad_d, int64_t B, int64_t outer, int64_t C, int64_t inner, int kind,
                           int inverse, int per_site, void *workspace, size_t workspace_bytes, int dtype, void *stream) {
  int rc = check_common("nf_pade_vjp", kind, dtype, x, d0, d1, C);
  if (rc) return rc;
  NF_REQUIRE(grad_y && grad_logj && grad_x && grad_d, "nf_pade_vjp: NULL tensor pointer");
  PadeArgs A{};
  rc = make_plan(A.p, B, outer, C, inner, "nf_pade_vjp");
  if (rc) return rc;
  const size_t need = size_t(A.p.units) * 2 * sizeof(double);
  if (need && (workspace == nullptr || workspace_bytes < need)) {
    set_error("nf_pade_vjp: workspace %zu B < %zu B needed", workspace_bytes, need);
    return NF_EWORKSPACE;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  A.x = x; A.d0 = d0; A.d1 = d1; A.grad_y = grad_y; A.grad_logj = grad_logj; A.grad_x = grad_x;
  A.partial = static_cast<double *>(workspace);
  if (A.p.units > 0) {
    if (dtype == NF_F32) dispatch<float>(true, A, kind, inverse, per_site, s);
    else dispatch<double>(true, A, kind, inverse, per_site, s);
    rc = check_launch("pade vjp kernel");
    if (rc) return rc;
  }
  hipLaunchKernelGGL(pade_channel_reduce_kernel, dim3(unsigned(C)), dim3(kBlock), 0, s, A.p,
                     static_cast<const double *>(workspace), grad_d);
  return check_launch("pade channel reduce kernel");
}

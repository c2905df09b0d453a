// nf_rqs_core.h -- device-side core of the rational-quadratic splines: the ONE statement of a segment between two knots
// (value, cancellation-free inverse root, derivative g, point and cotangent block of the VJPs), of the reflection /
// linear-tail frame of a coupling and of a softmax numerator; and, on them, the coupling's site functions: logits of one
// site (in registers or in an LDS column) -> knots -> bin -> value, log|derivative| and VJP.  Used by the stand-alone
// coupling kernels (nf_rqs.hip), the conv kernels' fused epilogues, K4 (nf_distconv.hip) and nf_spline_eval.
// Reference lines restated: see the header of nf_rqs.hip.
#pragma once
#include <hip/hip_fp16.h>
#include "nf_internal.h"

namespace nf {

// The options of one spline family as the device code sees them.
struct RqsParams {
  double xlo, xhi, ylo, yhi;
  const void *fx, *fy;       // optional fixed knot coordinates (m values of T), LDS-column kernels only
  int m, el, er;
};

// ------------------------------------------------------------ parameter columns
template <typename T, int C> struct RegCol {   // static m: logits live in VGPRs
  T v[C];
  __device__ __forceinline__ T &operator[](int i) { return v[i]; }
};
template <typename T> struct LdsCol {          // runtime m: one LDS column per lane
  T *p;                                        // row stride = blockDim.x (a multiple of 64):
  int stride;                                  // bank = lane % 32 for every row, conflict-free
  __device__ __forceinline__ T &operator[](int i) const { return p[i * stride]; }
};

template <typename T> struct Pair2;   // two adjacent sites as one 8/16-byte access
template <> struct Pair2<float> { typedef float2 type; };
template <> struct Pair2<double> { typedef double2 type; };
template <> struct Pair2<__half> { typedef __half2 type; };

template <typename T> struct Site {   // what the scan selects for one site
  T x0, y0, bw, bh, c0, c1, xe, ye;
  int j;
};

// Channel layout of the logits: [x widths (m-1) | y heights (m-1) | derivatives (m)], where
// the x (y) block is absent when knots_x (knots_y) is fixed (couplings_.py:236-262).
struct ChanMap { int ox, oy, od; };
__device__ __forceinline__ ChanMap chan_map(int m, bool fixx, bool fixy) {
  const int nb = m - 1;
  ChanMap c;
  c.ox = 0;
  c.oy = fixx ? 0 : nb;
  c.od = (fixx ? 0 : nb) + (fixy ? 0 : nb);
  return c;
}

// One rational-quadratic segment between two knots: left knot (x0, y0), width bw, height bh, end derivatives d0, d1
// (spline.py:185-220).  With th in [0, 1] the place in the bin, sl = bh / bw and curv = d0 + d1 - 2 sl:
//   y = y0 + bh (sl th^2 + d0 t1) / den,   g = dy/dx = sl^2 P / den^2,   t1 = th (1 - th),   den = sl + curv t1.
// Every kernel that evaluates, inverts or differentiates a segment does it through the functions below.
template <typename T> struct RqSeg { T x0, y0, bw, bh, d0, d1; };

// SHARE_RCP selects between two roundings of the same quotients.  false: every quotient is a division (rqs_site, K4,
// nf_spline_eval).  true: quotients that share a divisor share its correctly rounded reciprocal -- ibw for the slope and
// for theta, iden for the quotients by den (K5h's mover, where a division is ~10 instructions it has to hide in an MFMA
// phase, and the VJPs of the coupling kernels).  The flag exists because making the two one would change either the
// headline kernel's outputs or its instruction count, and neither is a refactor's to change.
template <typename T> struct RqAt { T sl, curv, th, om, t1, den; };   // what value and derivative share at th
template <typename T> __device__ __forceinline__ RqAt<T> rq_at(const RqSeg<T> &s, T sl, T curv, T th) {
  RqAt<T> a;
  a.sl = sl; a.curv = curv; a.th = th;
  a.om = T(1) - th; a.t1 = th * a.om;
  a.den = sl + curv * a.t1;
  return a;
}
// ... at the point x of the segment
template <typename T, bool SHARE_RCP> __device__ __forceinline__ RqAt<T> rq_at_x(const RqSeg<T> &s, T x) {
  const T ibw = T(1) / s.bw;
  const T sl = SHARE_RCP ? s.bh * ibw : s.bh / s.bw;
  const T curv = s.d0 + s.d1 - T(2) * sl;
  const T th = SHARE_RCP ? (x - s.x0) * ibw : (x - s.x0) / s.bw;
  return rq_at(s, sl, curv, th);
}
// ... at the point whose value is y (spline.py:222-287).  The two conscious departures from the reference's arithmetic
//  live here and nowhere else: the root of a2 th^2 - bb th + a0 = 0 in [0, 1] is written so that neither
// branch cancels, and the discriminant is clamped at 0 (rounding can take it below for a value on a knot).
template <typename T, bool SHARE_RCP> __device__ __forceinline__ RqAt<T> rq_at_y(const RqSeg<T> &s, T y) {
  const T sl = SHARE_RCP ? s.bh * (T(1) / s.bw) : s.bh / s.bw;
  const T curv = s.d0 + s.d1 - T(2) * sl;
  const T eta = (y - s.y0) / s.bh;
  const T a2 = -curv * eta + s.d0 - sl;
  const T bb = a2 + sl;              // = -a1
  const T a0 = sl * eta;
  const T disc = Num<T>::sqrt(Num<T>::max(bb * bb - T(4) * a0 * a2, T(0)));
  const T th = (bb >= T(0)) ? T(2) * a0 / (bb + disc) : (bb - disc) / (T(2) * a2);
  return rq_at(s, sl, curv, th);
}
template <typename T> __device__ __forceinline__ T rq_P(const RqSeg<T> &s, const RqAt<T> &a) {    // g = sl^2 P / den^2
  return s.d1 * a.th * a.th + T(2) * a.sl * a.t1 + s.d0 * a.om * a.om;
}
template <typename T, bool SHARE_RCP> __device__ __forceinline__ T rq_deriv(const RqSeg<T> &s, const RqAt<T> &a) {
  const T P = rq_P(s, a), iden = T(1) / a.den;
  return SHARE_RCP ? a.sl * a.sl * P * (iden * iden) : a.sl * a.sl * P / (a.den * a.den);
}
template <typename T, bool SHARE_RCP> __device__ __forceinline__ T rq_y(const RqSeg<T> &s, const RqAt<T> &a) {
  const T num = a.sl * a.th * a.th + s.d0 * a.t1;
  return SHARE_RCP ? s.y0 + s.bh * num * (T(1) / a.den) : s.y0 + s.bh * num / a.den;
}
template <typename T> __device__ __forceinline__ T rq_x(const RqSeg<T> &s, const RqAt<T> &a) { return s.x0 + s.bw * a.th; }

// x -> y and y -> x, with g = dy/dx at x.  (Only the forward quotients by den share a reciprocal.)
template <typename T, bool SHARE_RCP = false> __device__ __forceinline__ T rq_fwd(const RqSeg<T> &s, T x, T &g) {
  const RqAt<T> a = rq_at_x<T, SHARE_RCP>(s, x);
  g = rq_deriv<T, SHARE_RCP>(s, a);
  return rq_y<T, SHARE_RCP>(s, a);
}
template <typename T, bool SHARE_RCP = false> __device__ __forceinline__ T rq_inv(const RqSeg<T> &s, T y, T &g) {
  const RqAt<T> a = rq_at_y<T, SHARE_RCP>(s, y);
  g = rq_deriv<T, false>(s, a);
  return rq_x(s, a);
}

// What the coupling VJPs need at the point x of a segment, recomputed in the forward direction with shared
// reciprocals: g, and Lth = dL/dth for L = log g.
template <typename T> struct RqPoint : RqAt<T> { T ibw, iden, iP, num, P, g, Lth; };
template <typename T> __device__ __forceinline__ RqPoint<T> rq_point(const RqSeg<T> &s, T x) {
  RqPoint<T> p;
  static_cast<RqAt<T> &>(p) = rq_at_x<T, true>(s, x);
  p.num = p.sl * p.th * p.th + s.d0 * p.t1;
  p.P = rq_P<T>(s, p);
  p.ibw = T(1) / s.bw; p.iden = T(1) / p.den; p.iP = T(1) / p.P;
  p.g = p.sl * p.sl * p.P * p.iden * p.iden;
  const T Pp = T(2) * (s.d1 * p.th + p.sl * (T(1) - T(2) * p.th) - s.d0 * p.om);
  p.Lth = Pp * p.iP - T(2) * p.curv * (T(1) - T(2) * p.th) * p.iden;
  return p;
}

// Cotangents of theta, the slope, the end derivatives, the bin height and the bin width from gy (on the segment's value)
// and gl (on log g).  The callers turn (thb, wb, hb) into the cotangents of their own coordinates.
template <typename T> struct RqCot { T thb, slb, d0b, d1b, hb, wb; };
template <typename T> __device__ __forceinline__ RqCot<T> rq_cotangents(const RqSeg<T> &s, const RqPoint<T> &p, T gy, T gl) {
  const T th = p.th, t1 = p.t1, den = p.den, num = p.num, iP = p.iP, ibw = p.ibw, iden = p.iden, i2 = iden * iden;
  RqCot<T> c;
  c.thb = gy * p.g * s.bw + gl * p.Lth;
  c.slb = gy * s.bh * (th * th * den - num * (T(1) - T(2) * t1)) * i2 +
          gl * (T(2) / p.sl + T(2) * t1 * iP - T(2) * (T(1) - T(2) * t1) * iden);
  c.d0b = gy * s.bh * t1 * (den - num) * i2 + gl * (p.om * p.om * iP - T(2) * t1 * iden);
  c.d1b = -gy * s.bh * num * t1 * i2 + gl * (th * th * iP - T(2) * t1 * iden);
  c.hb = gy * num * iden + c.slb * ibw;
  c.wb = -(c.thb * th + c.slb * p.sl) * ibw;
  return c;
}

// The frame around the segments of a coupling: the limits, the point reflection through an end knot
// (NF_EXTRAP_ANTI: the argument is reflected on the way in, the value on the way out), the tangent-line tails
// (NF_EXTRAP_LINEAR) and log|derivative| = +-log g.  INV=false: x -> y; INV=true: y -> x.
template <typename T, bool INV> struct RqFrame {
  T xlo, W, ylo, H, in_lo, in_hi, out_lo, out_hi;
  bool refl_l, refl_r;
  __device__ __forceinline__ RqFrame(const RqsParams &A, T v)      // v: the argument as it comes
      : xlo(T(A.xlo)), W(T(A.xhi) - T(A.xlo)), ylo(T(A.ylo)), H(T(A.yhi) - T(A.ylo)) {
    in_lo = INV ? ylo : xlo; in_hi = INV ? ylo + H : xlo + W;
    out_lo = INV ? xlo : ylo; out_hi = INV ? xlo + W : ylo + H;
    refl_l = (A.el == NF_EXTRAP_ANTI) && (v < in_lo);
    refl_r = (A.er == NF_EXTRAP_ANTI) && (v > in_hi);
  }
  __device__ __forceinline__ T reflected(T v) const {   // the argument the bins and eval() see
    return refl_l ? T(2) * in_lo - v : (refl_r ? T(2) * in_hi - v : v);
  }
  // The bin the scan selected for the (reflected) v, or a tail beyond the end knots.
  template <bool SHARE_RCP>
  __device__ __forceinline__ void eval(const RqsParams &A, const Site<T> &b, T v, T &val, T &logd) const {
    const T xe = b.xe, ye = b.ye;
    const bool tail_l = (A.el == NF_EXTRAP_LINEAR) && !(in_lo < v);
    const bool tail_r = (A.er == NF_EXTRAP_LINEAR) && ((INV ? ye : xe) < v);
    const RqSeg<T> s{b.x0, b.y0, b.bw, b.bh, softplus2(b.c0), softplus2(b.c1)};
    T g;
    if (!INV) {
      val = rq_fwd<T, SHARE_RCP>(s, v, g);
      val = tail_l ? ylo + s.d0 * (v - xlo) : (tail_r ? ye + s.d1 * (v - xe) : val);
    } else {
      val = rq_inv<T, SHARE_RCP>(s, v, g);
      val = tail_l ? xlo + (v - ylo) / s.d0 : (tail_r ? xe + (v - ye) / s.d1 : val);
    }
    g = tail_l ? s.d0 : (tail_r ? s.d1 : g);
    logd = INV ? -nf_log(g) : nf_log(g);
    val = refl_l ? T(2) * out_lo - val : (refl_r ? T(2) * out_hi - val : val);
  }
};

// One softmax numerator, exp(logit - max) as an exp2: the term of scan_bins' x and y blocks and of rqs_knots_kernel.
// (The max / sum loops around it stay where they run: moved into a function of their own they are optimised before they
// are inlined, and the run-time-m instances of the coupling kernels then no longer compile to the same instructions.)
template <typename T> __device__ __forceinline__ T softmax_term(T logit, T amax) {
  return Num<T>::exp2((logit - amax) * Num<T>::kLog2e);
}

// Softmax numerators in place, then the predicated bin scan.  On return the x and y logit
// blocks of `a` hold exp(logit - max); sa/sb their sums.  With fixed knot coordinates (only
// reachable in the LDS-column kernel, MT == 0) bin widths come from the fixed array.
template <typename T, int MT, bool ON_Y, typename Col>
__device__ __forceinline__ Site<T> scan_bins(Col &a, const RqsParams &A, T v, T xlo, T W, T ylo, T H, T &sa,
                                             T &sb) {
  const int m = MT > 0 ? MT : A.m;
  const int nb = m - 1;
  const T *fx = MT > 0 ? nullptr : static_cast<const T *>(A.fx);
  const T *fy = MT > 0 ? nullptr : static_cast<const T *>(A.fy);
  const ChanMap cm = chan_map(m, fx != nullptr, fy != nullptr);
  sa = T(1);
  sb = T(1);
  if (!fx) {
    T amax = a[cm.ox];
#pragma unroll
    for (int k = 1; k < nb; ++k) amax = Num<T>::max(amax, a[cm.ox + k]);
    sa = T(0);
#pragma unroll
    for (int k = 0; k < nb; ++k) {
      const T e = softmax_term(a[cm.ox + k], amax);
      a[cm.ox + k] = e;
      sa += e;
    }
  }
  if (!fy) {
    T bmax = a[cm.oy];
#pragma unroll
    for (int k = 1; k < nb; ++k) bmax = Num<T>::max(bmax, a[cm.oy + k]);
    sb = T(0);
#pragma unroll
    for (int k = 0; k < nb; ++k) {
      const T e = softmax_term(a[cm.oy + k], bmax);
      a[cm.oy + k] = e;
      sb += e;
    }
  }
  const T wx = W / sa, wy = H / sb;
  Site<T> s;
  T cx = xlo, cy = ylo;
  s.x0 = xlo; s.y0 = ylo;
  s.bw = fx ? fx[1] - fx[0] : a[cm.ox] * wx;
  s.bh = fy ? fy[1] - fy[0] : a[cm.oy] * wy;
  s.c0 = a[cm.od]; s.c1 = a[cm.od + 1]; s.j = 0;
  cx = fx ? fx[1] : cx + s.bw;
  cy = fy ? fy[1] : cy + s.bh;
#pragma unroll
  for (int k = 1; k < nb; ++k) {
    const T wk = fx ? fx[k + 1] - fx[k] : a[cm.ox + k] * wx;
    const T hk = fy ? fy[k + 1] - fy[k] : a[cm.oy + k] * wy;
    const bool sel = (ON_Y ? cy : cx) < v;   // knot k strictly below the value
    s.x0 = sel ? cx : s.x0;
    s.y0 = sel ? cy : s.y0;
    s.bw = sel ? wk : s.bw;
    s.bh = sel ? hk : s.bh;
    s.c0 = sel ? a[cm.od + k] : s.c0;
    s.c1 = sel ? a[cm.od + k + 1] : s.c1;
    s.j = sel ? k : s.j;
    cx = fx ? fx[k + 1] : cx + wk;
    cy = fy ? fy[k + 1] : cy + hk;
  }
  s.xe = cx; s.ye = cy;   // last knot as accumulated (the reference's cumsum end)
  return s;
}

// Value and log|derivative| of the map at one site.  INV=false: v is x, returns y
// and log(dy/dx).  INV=true: v is y, returns x and log(dx/dy) = -log g.
template <typename T, int MT, bool INV, typename Col>
__device__ __forceinline__ void rqs_site(Col &a, const RqsParams &A, T v, T &val, T &logd) {
  const RqFrame<T, INV> F(A, v);
  v = F.reflected(v);
  T sa, sb;
  const Site<T> s = scan_bins<T, MT, INV>(a, A, v, F.xlo, F.W, F.ylo, F.H, sa, sb);
  F.template eval<false>(A, s, v, val, logd);
}

// VJP at one site.  `x` is the point on the x axis (forward input, or inverse
// output).  gout / glog are the cotangents of (value, log-det) of the map selected
// by INV.  Writes the C parameter cotangents back into `a` and returns grad_in.
template <typename T, int MT, bool INV, typename Col>
__device__ __forceinline__ T rqs_site_vjp(Col &a, const RqsParams &A, T x, T gout, T glog) {
  const int m = MT > 0 ? MT : A.m;
  const int nb = m - 1;
  const RqFrame<T, false> F(A, x);     // the chain is re-run in its forward direction: reflect on the x axis
  const T v = F.reflected(x);
  const T xlo = F.xlo, W = F.W, ylo = F.ylo, H = F.H;
  const T sgn = (F.refl_l || F.refl_r) ? T(-1) : T(1);
  T sa, sb;
  const Site<T> s = scan_bins<T, MT, false>(a, A, v, xlo, W, ylo, H, sa, sb);
  const bool tail_l = (A.el == NF_EXTRAP_LINEAR) && !(xlo < v);
  const bool tail_r = (A.er == NF_EXTRAP_LINEAR) && (s.xe < v);
  const bool tail = tail_l || tail_r;
  T sg0, sg1;
  const T d0 = softplus2(s.c0, &sg0), d1 = softplus2(s.c1, &sg1);
  const RqSeg<T> seg{s.x0, s.y0, s.bw, s.bh, d0, d1};
  RqPoint<T> p = rq_point(seg, v);
  p.g = tail_l ? d0 : (tail_r ? d1 : p.g);
  p.Lth = tail ? T(0) : p.Lth;         // L = log g is constant on the linear tails
  const T g = p.g, Lth = p.Lth, ibw = p.ibw;
  // cotangents (gy on the value of the forward map in the actual frame, gl on log g)
  T gy, gl, grad_in;
  if (!INV) {
    gy = gout; gl = glog;
    grad_in = gy * g + gl * sgn * Lth * ibw;
  } else {
    // inverse outputs (x, -L):  dx = (dy - f_p dp)/g ,  d(-L) = -(L_x dx + L_p dp)
    // => cotangent of y: A1 = (gout - glog L_x)/g ; of p: -A1 f_p - glog L_p
    const T Lx = sgn * Lth * ibw;
    const T A1 = (gout - glog * Lx) / g;
    grad_in = A1;
    gy = -A1; gl = -glog;
  }
  const T gyF = sgn * gy;   // cotangent on F's value in the unreflected frame
  T d0b, d1b, x0b, wb, y0b, hb;
  if (tail) {
    d0b = tail_l ? gyF * (v - xlo) + gl / d0 : T(0);
    d1b = tail_r ? gyF * (v - s.xe) + gl / d1 : T(0);
    x0b = wb = y0b = hb = T(0);
  } else {
    const RqCot<T> c = rq_cotangents(seg, p, gyF, gl);
    d0b = c.d0b; d1b = c.d1b; hb = c.hb; wb = c.wb;
    y0b = gyF;
    x0b = -c.thb * ibw;
  }
  // back through softmax / cumsum (the free x / y blocks of a[] hold the softmax numerators)
  const bool fixx = MT == 0 && A.fx != nullptr, fixy = MT == 0 && A.fy != nullptr;
  const ChanMap cm = chan_map(m, fixx, fixy);
  const T gc0 = d0b * sg0, gc1 = d1b * sg1;
  if (!fixx) {
    const T Sx = x0b * (s.x0 - xlo) + wb * s.bw;
    const T isa = T(1) / sa;
#pragma unroll
    for (int k = 0; k < nb; ++k) {
      const T lead_x = (k < s.j) ? x0b : ((k == s.j) ? wb : T(0));
      a[cm.ox + k] = a[cm.ox + k] * isa * (W * lead_x - Sx);
    }
  }
  if (!fixy) {
    const T Sy = y0b * (s.y0 - ylo) + hb * s.bh;
    const T isb = T(1) / sb;
#pragma unroll
    for (int k = 0; k < nb; ++k) {
      const T lead_y = (k < s.j) ? y0b : ((k == s.j) ? hb : T(0));
      a[cm.oy + k] = a[cm.oy + k] * isb * (H * lead_y - Sy);
    }
  }
#pragma unroll
  for (int k = 0; k < m; ++k) a[cm.od + k] = (k == s.j) ? gc0 : ((k == s.j + 1) ? gc1 : T(0));
  return grad_in;
}

}  // namespace nf

/* normflow_hip.h -- C ABI of libnormflow_hip.so (gfx950 / MI355X).
 *
 * The drop-in boundary for the coupling-layer hot path of jkomijani/normflow_.
 * The reference has no FFI of its own (it is pure Python on eager aten ops), so
 * each entry point replaces an *eager op chain* of the reference; the file:line
 * of that chain is cited per function (paths relative to the reference root).
 * INTEGRATION.md shows the ctypes binding a reference maintainer would add.
 *
 * Rules of the boundary
 *   - every pointer is a DEVICE pointer owned by the caller (a torch tensor's
 *     data_ptr(), a hipMalloc'd buffer ...); the library never allocates, frees
 *     or synchronises; scratch space is passed in (`workspace`), its size is
 *     given by nf_workspace_bytes();
 *   - every launch goes to the `stream` argument (a hipStream_t passed as void*);
 *   - every function returns 0 on success, a negative NF_E* code otherwise, and
 *     never throws; nf_last_error_string() describes the last failure of the
 *     calling thread;
 *   - tensors are dense and row-major.  B = batch, V = number of lattice sites,
 *     C = channels of raw net output per site.  `dtype` selects the arithmetic
 *     and storage type of all floating tensors of a call.
 *
 * Site activity ("checkerboard masking", src/mask/mask.py:17-61) is given by a
 * byte mask of V entries: 1 = the site is transformed by this layer ("active"),
 * 0 = it is frozen.  Two layouts of the per-site parameter tensor exist:
 *   NF_LAYOUT_FULL : params is (B, C, V); entries at frozen sites are ignored;
 *   NF_LAYOUT_PAIR : params is (B, C, V/2): the sites are taken in aligned pairs
 *                    (2h, 2h+1), exactly one site of every pair is active (true
 *                    for an even-odd mask whose fastest axis is even), and column
 *                    h holds the parameters of that pair's active site.  This is
 *                    the HBM-efficient layout: no parameter bytes are read for
 *                    frozen sites.
 */
#ifndef NORMFLOW_HIP_H
#define NORMFLOW_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NF_VERSION 301 /* 0.3.1 */

/* NF_F16 (nf_rqs_fwd / nf_rqs_inv with knots_len 4/8/16, nf_affine_fwd / nf_affine_inv): x, params and y are IEEE half, the arithmetic is fp32 and
 * log0 / logj are fp32 ("fp16 params / fp32 log-det accumulate", BASELINE config 5). */
/* NF_F16_FIELD (nf_affine_fwd / nf_affine_inv only): x and y are IEEE half, params stay fp32 (what a conv layer wrote),
 * fp32 arithmetic and log-det. */
enum nf_dtype { NF_F32 = 0, NF_F64 = 1, NF_F16 = 2, NF_F16_FIELD = 3 };
enum nf_layout { NF_LAYOUT_FULL = 0, NF_LAYOUT_PAIR = 1 };
enum nf_extrap { NF_EXTRAP_NONE = 0, NF_EXTRAP_LINEAR = 1, NF_EXTRAP_ANTI = 2 };
enum nf_status {
  NF_OK = 0,
  NF_EINVAL = -1,    /* bad argument (null pointer, bad size, unsupported option) */
  NF_EWORKSPACE = -2,/* workspace too small */
  NF_ELAUNCH = -3    /* hip launch error */
};

/* Options of one rational-quadratic spline family
 * (RQSplineCoupling_.__init__, src/nn/scalar/couplings_.py:159-176). */
typedef struct nf_rqs_opts {
  int32_t m;            /* knots per spline; C = 3m-2, or 2m-1 / m with fixed knots */
  int32_t extrap_left;  /* nf_extrap */
  int32_t extrap_right; /* nf_extrap */
  int32_t layout;       /* nf_layout of `params` (and of grad_params) */
  double xlo, xhi, ylo, yhi;
  const void *fixed_knots_x; /* optional device array of m values (dtype), or NULL */
  const void *fixed_knots_y; /* optional device array of m values (dtype), or NULL */
} nf_rqs_opts;

/* Strides (in elements) from one batch entry to the next; 0 selects the dense
 * default.  They exist so that one data channel of a multi-channel tensor
 * (MultiRQSplineCoupling_, couplings_.py:279-436) can be addressed in place. */
typedef struct nf_strides {
  int64_t x_batch;      /* default V            */
  int64_t y_batch;      /* default V            */
  int64_t params_batch; /* default C * V or C*V/2 */
} nf_strides;

int nf_version(void);
const char *nf_last_error_string(void);

/* Process-wide kernel-selection options.  They choose between kernels that compute the SAME layer (results within the
 * tolerances stated per kernel); none of them skips work.  The library never reads the environment in a product build
 * (timing ablations and clock stamps exist only in `make DIAG=1` builds, which define NF_DIAG).
 *   NF_OPT_SPLIT16 (default 1): tanh / logistic ConvAct stacks may run the split-fp16 kernels (nf_conv_h.hip: every fp32
 *                  product as three fp16 matrix-core products, fp32 accumulation); 0 = exact fp32 MFMA products everywhere
 *                  (nf_conv_weight_layout / nf_conv_split16_supported answer accordingly);
 *   NF_OPT_PIPE    (default 1): eligible fp32 layers run the persistent, staging-overlapped kernels (nf_conv_pipe.hip);
 *                  0 = one box per workgroup (nf_conv.hip).
 * nf_set_option returns the previous value (>= 0) or NF_EINVAL; set options before launching, not concurrently with calls.
 */
enum nf_option { NF_OPT_SPLIT16 = 0, NF_OPT_PIPE = 1, NF_OPT_COUNT_ = 2 };
int nf_set_option(int which, int value);
int nf_get_option(int which);

/* Bytes of scratch needed by any coupling / distconv call on a (B, V) problem. */
size_t nf_workspace_bytes(int64_t B, int64_t V);

/* ---- planning queries: how the element-wise kernels cut a (B, units) problem into workgroups.  Pure host code, no GPU
 * work; they call the planners the launchers call, so a test can assert which regime a shape lands in.
 *
 * nf_plan_tiling: every workgroup of `block` lanes (256; 64 or 128 for the LDS-column spline kernel, see
 * nf_rqs_plan_block) owns block * iters consecutive units of ONE sample, walks them in `iters` in {1, 2, 4, 8} strides of
 * `block` and writes one double partial per (sample, workgroup); *blocks_x = workgroups per sample =
 * ceil(units / (block * iters)).  iters doubles while (units / (2 block iters)) * B >= 8192.  `units` per entry point:
 *   V            nf_rqs_* / nf_affine_* in NF_LAYOUT_FULL, nf_distconv, nf_distconv_sites, nf_phi4_action,
 *                nf_normal_logprob
 *   V / 2        nf_rqs_* / nf_affine_* in NF_LAYOUT_PAIR (one unit = one site pair)
 *   ceil(V / 4)  nf_normal_sample in fp32 (one unit = one Philox call = four normals); ceil(V / 2) in fp64
 * (nf_pade plans by itself; its plan can be read from nf_pade_workspace_bytes: one 16-byte partial per (sample, channel
 * group, workgroup).)  Returns 0, or NF_EINVAL for a NULL output pointer, a negative size or a block other than 64, 128
 * or 256.
 * nf_rqs_plan_block: the workgroup size the spline kernels run this family with in `dtype` (256 for the register kernels
 * of knots_len 4, 8, 16 without fixed knots; the LDS-column kernel halves it until a column of C logits per lane fits
 * 64 KiB), or 0 -- with the reason in nf_last_error_string -- if the options are invalid or the spline does not fit. */
int nf_plan_tiling(int64_t units, int64_t B, int block, int *iters, int64_t *blocks_x);
int nf_rqs_plan_block(const nf_rqs_opts *opts, int dtype);

/* ---- K2/K3: rational-quadratic spline coupling -----------------------------
 * Replaces, fused in one pass: knot construction (couplings_.py:211-262:
 * split, softmax, cumsum, scale/shift, softplus(beta=ln2)), boundary
 * augmentation (src/lib/spline/spline.py:458-532), bin search (:154-172),
 * segment evaluation (:185-220) or inversion (:222-287), purify + log +
 * per-sample sum (couplings_.py:186-188, src/nn/_core.py:38-42).
 *
 *   x       (B, V)  input field; only active sites are read
 *   params  (B, C, V) or (B, C, V/2) raw net output (logits)
 *   mask    (V) bytes, 1 = active
 *   log0    (B) or NULL (treated as 0)
 *   y       (B, V)  out: transformed value at active sites, 0 at frozen sites
 *   logj    (B)     out: log0 + sum over active sites of log|dy/dx|
 * nf_rqs_inv is the inverse map (y -> x) and adds log|dx/dy|; it uses the
 * cancellation-free root 2 a0 / (-a1 + sqrt(a1^2 - 4 a0 a2)).
 */
int nf_rqs_fwd(const void *x, const void *params, const uint8_t *mask, const void *log0,
               void *y, void *logj, int64_t B, int64_t V, const nf_rqs_opts *opts,
               const nf_strides *strides, void *workspace, size_t workspace_bytes,
               int dtype, void *stream);
int nf_rqs_inv(const void *y, const void *params, const uint8_t *mask, const void *log0,
               void *x, void *logj, int64_t B, int64_t V, const nf_rqs_opts *opts,
               const nf_strides *strides, void *workspace, size_t workspace_bytes,
               int dtype, void *stream);

/* Vector-Jacobian products of the two maps above (what autograd derives from the
 * eager chain in the reference; needed by Fitter.step, src/_normflowcore.py:288).
 *   grad_out  (B, V)  cotangent of the value output
 *   grad_logj (B)     cotangent of the log-Jacobian output
 *   grad_in   (B, V)  out: cotangent of the value input (0 at frozen sites)
 *   grad_params       out: same shape/layout as params (0 at frozen sites)
 * nf_rqs_fwd_vjp takes the forward INPUT x; nf_rqs_inv_vjp takes the inverse's
 * OUTPUT x (= the point on the x axis), so neither recomputes a root.
 */
int nf_rqs_fwd_vjp(const void *x, const void *params, const uint8_t *mask,
                   const void *grad_out, const void *grad_logj, void *grad_in,
                   void *grad_params, int64_t B, int64_t V, const nf_rqs_opts *opts,
                   const nf_strides *strides, int dtype, void *stream);
int nf_rqs_inv_vjp(const void *x, const void *params, const uint8_t *mask,
                   const void *grad_out, const void *grad_logj, void *grad_in,
                   void *grad_params, int64_t B, int64_t V, const nf_rqs_opts *opts,
                   const nf_strides *strides, int dtype, void *stream);

/* nf_affine_sites: nf_affine_fwd (inverse = 0) / nf_affine_inv (1) that additionally writes the log-derivative of every
 * site (-|s| forward, +|s| inverse; 0 for a shift layer and at frozen sites) to site_out (B,V) of dtype: what
 * Module_.sum_density passes through when propagate_density is set (src/nn/_core.py:19,38-42).  NF_F32 / NF_F64. */
int nf_affine_sites(const void *v, const void *params, const uint8_t *mask, const void *log0, void *out,
                    void *logj, void *site_out, int64_t B, int64_t V, int n_ch, int layout, int inverse,
                    void *workspace, size_t workspace_bytes, int dtype, void *stream);

/* ---- K2s: the spline object of a coupling layer -------------------------------
 * What a user of the reference reaches through RQSplineCoupling_.make_spline / _hack
 * (src/nn/scalar/couplings_.py:202-262) and through propagate_density
 * (src/nn/_core.py:19,38-42): the derivative of every site instead of only its summed log.
 *
 * nf_rqs_fwd_sites / nf_rqs_inv_sites are nf_rqs_fwd / nf_rqs_inv (same arguments, same y and
 * logj) and additionally write site_out (B,V) of dtype: with NF_SITES_LOG the log-derivative
 * log|dy/dx| (fwd) or log|dx/dy| (inv) of every active site, with NF_SITES_DERIVATIVE the
 * derivative itself (`g` of spline.py:87-123 with grad=True; the inverse returns 1/g as the
 * reference's spline.backward does, spline.py:222-287); 0 at frozen sites.  NF_F32 / NF_F64.
 *
 * nf_rqs_knots writes the knot tensors make_spline builds from the logits, before the boundary
 * augmentation of spline.py:458-532: knots (B, 3m, V) of dtype = knots_x (m planes), knots_y (m),
 * knots_d (m); fixed knots_x / knots_y are copied through.  params in the full layout (B, C, V).
 * The arithmetic is the coupling kernels' own: these are the knots they evaluate. */
enum nf_sites_mode { NF_SITES_LOG = 1, NF_SITES_DERIVATIVE = 2 };
int nf_rqs_fwd_sites(const void *x, const void *params, const uint8_t *mask, const void *log0,
                     void *y, void *logj, void *site_out, int site_mode, int64_t B, int64_t V,
                     const nf_rqs_opts *opts, const nf_strides *strides, void *workspace,
                     size_t workspace_bytes, int dtype, void *stream);
int nf_rqs_inv_sites(const void *y, const void *params, const uint8_t *mask, const void *log0,
                     void *x, void *logj, void *site_out, int site_mode, int64_t B, int64_t V,
                     const nf_rqs_opts *opts, const nf_strides *strides, void *workspace,
                     size_t workspace_bytes, int dtype, void *stream);
int nf_rqs_knots(const void *params, void *knots, int64_t B, int64_t V, const nf_rqs_opts *opts,
                 int dtype, void *stream);

/* ---- K2e: a spline from explicit knot tensors ------------------------------------
 * The reference's generic spline object RQSpline(knots_x, knots_y, knots_d) = Pade22Spline
 * (src/lib/spline/spline.py:39-68; forward / backward :87-123; searchsorted + clamp :154-172;
 * segment function :185-220; inverse :222-287, with the stable root of App. A #2).
 * v, out, deriv: (B, V) of dtype (deriv may be NULL).  A knot tensor is (B, K, V) planes, or a
 * shared vector of K entries when its shared_* flag is set (the reference's 1-D knots).  Knots
 * are evaluated as given (already augmented for extrapolation; values outside reuse the end
 * segments).  inverse: out = x(v), deriv = dx/dy = 1/g.  NF_F32 / NF_F64, B <= 65535. */
int nf_spline_eval(const void *v, const void *knots_x, const void *knots_y, const void *knots_d,
                   void *out, void *deriv, int64_t B, int64_t V, int K, int shared_x, int shared_y,
                   int shared_d, int inverse, int dtype, void *stream);

/* ---- K5h as a differentiable node: the fused last layer + RQ-spline coupling in a TRAINING step -----------------
 * Reference: Fitter.step (src/_normflowcore.py:275-294) differentiates couplings_.py:178-200 through autograd, which
 * keeps the (B, 3m-2, *L) logits of every layer alive.  Here the logits never exist in memory, forward or backward:
 *  nf_conv_rqs_split16_train = nf_conv_rqs on the split-fp16 kernel for hidden activations of unknown range:
 *    `in` = (B, 8, V) fp32 planes (fastest axis of 32 sites) or, with in_split16, the (B, V, 16) pair tensor
 *    nf_planes_to_split16 made of them; absmax_bits (nf_absmax_bits of the planes, or NULL = unit range): the input is /
 *    gets scaled by the matching power of two, the logits are descaled.  wsplit: NF_WLAYOUT_SPLIT16.  y (B, V), logj (B).
 *  nf_conv_rqs_split16_vjp: recomputes the logits in the kernel and sends the cotangents (grad_y (B, V), grad_logj (B))
 *    back through the spline: grad_logits (B, cout, V/2) fp32 pair-compact -- the form nf_conv_wgrad_split16 /
 *    nf_conv_dgrad_split16 read (compact_parity) -- and grad_x (B, V), zero at frozen sites.  x_point: the point on
 *    the x axis (the forward pass's input, or the inverse pass's output).  inverse: VJP of the inverse map.
 * knots_len 2..16, cout = 3m-2; lattices as nf_conv_rqs_split16_supported. */
int nf_conv_rqs_split16_train(const void *in, int in_split16, const void *wsplit, const void *bias, int cout,
                              const void *x_active, const void *log0, void *y, void *logj, int64_t B,
                              const int32_t *lattice, int active_parity, const void *absmax_bits,
                              const nf_rqs_opts *opts, int inverse, void *workspace, size_t workspace_bytes,
                              void *stream);
int nf_conv_rqs_split16_vjp(const void *in, int in_split16, const void *wsplit, const void *bias, int cout,
                            const void *x_point, const void *grad_y, const void *grad_logj, void *grad_logits,
                            void *grad_x, int64_t B, const int32_t *lattice, int active_parity,
                            const void *absmax_bits, const nf_rqs_opts *opts, int inverse, void *stream);

/* ---- K5s: a whole coupling layer of a SMALL lattice in one kernel ---------
 * kind 0 = RQ-spline coupling (cout = 3m - 2, m = 2..16), ndim 3: replaces, for lattices (L0, L1, 16) that fit a CU's LDS
 * (16^3 = BASELINE config 3), the whole atom
 * src/nn/scalar/couplings_.py:178-200: net(x_frozen) = ConvAct 1 -> 8 -> 8 -> cout (src/nn/scalar/modules.py:120-145,
 * 3^3 circular kernels, tanh / logistic hidden activations), make_spline (:211-262), the spline map and log g
 * (src/lib/spline/spline.py:154-287), purify and sum_density -- the hidden activations and the logits never leave the CU.
 * x_frozen, x_active, y: (B, V) fp32 (x_frozen: zeros at the active sites; y: zeros at the frozen sites); log0 (B) or
 * NULL, logj (B).  w1 / w2 / w3: the layers' weights scaled by 2^10 and split into fp16 (hi, lo) MFMA fragments --
 *   w1 [hi|lo][64 lanes][8]: A operand, lane 16 g + co holds taps 8g .. 8g+7 (tap = 9 j0 + 3 j1 + j2, zero from 27 and
 *      for co >= 8) of the single input channel;
 *   w2 [kernel row 3 j0 + j1 (9)][hi|lo][64][8]: A operand, lane 16 g + 8 s + co holds the 8 input channels of tap g - s of
 *      the fastest axis for output site s of a pair (zero outside 0..2);
 *   w3 [column tile (3)][K slice (7)][hi|lo][64][8]: B operand, lane 16 g + n holds the 8 input channels of tap 4 slice + g
 *      for logit channel 16 tile + n (zero for tap 27 and channels >= cout);
 * b1, b2 (8), b3 (cout): fp32 biases or NULL.  Hidden widths below 8: zero-padded by the host.
 * active_parity: the active site of pair (2h, 2h+1) in row (z, y) is 2h + ((active_parity + z + y) & 1).  fp32 only.
 * The same kernel serves the other small-lattice atoms: kind 1 = AFFINE coupling (couplings_.py:123-139: the net ends in
 * (t, s), cout = 2; y = t + x e^{-|s|}, logj = log0 - sum |s|; opts may be NULL); ndim 2: lattice (L1, 16) -- BASELINE
 * config 2's 16 x 16 -- with the 3^2 kernels embedded as the middle plane (j0 = 1) of 3^3 weight tensors, zero elsewhere,
 * packed in the same fragments.  In 2-D the active site of pair (2h, 2h+1) in row y is 2h + ((active_parity + y) & 1). */
int nf_small_lattice_supported(const int32_t *lattice, int ndim, int kind, int cout, int m, int act1, int act2);
int nf_small_lattice_coupling(int kind, const void *x_frozen, const void *x_active, const void *w1, const void *b1,
                              const void *w2, const void *b2, const void *w3, const void *b3, const void *log0,
                              void *y, void *logj, int64_t B, const int32_t *lattice, int ndim, int active_parity,
                              int cout, int act1, int act2, const nf_rqs_opts *opts, int inverse, void *stream);

/* ---- K1: affine / shift coupling --------------------------------------------
 * Replaces couplings_.py:123-139 (affine: chunk, 2 purify, abs, exp, fma, sum)
 * and :110-116 (shift).  params is (B, 2, .) = (t, s) for affine, (B, 1, .) = t
 * for shift (n_ch selects).  fwd: y = t + x e^{-|s|}, logj = log0 - sum|s|;
 * inv: x = (y - t) e^{|s|}, logj = log0 + sum|s|.
 */
int nf_affine_fwd(const void *x, const void *params, const uint8_t *mask, const void *log0,
                  void *y, void *logj, int64_t B, int64_t V, int n_ch, int layout,
                  void *workspace, size_t workspace_bytes, int dtype, void *stream);
int nf_affine_inv(const void *y, const void *params, const uint8_t *mask, const void *log0,
                  void *x, void *logj, int64_t B, int64_t V, int n_ch, int layout,
                  void *workspace, size_t workspace_bytes, int dtype, void *stream);
/* `inverse` selects which map is differentiated; `v` is that map's input. */
int nf_affine_vjp(const void *v, const void *params, const uint8_t *mask,
                  const void *grad_out, const void *grad_logj, void *grad_in,
                  void *grad_params, int64_t B, int64_t V, int n_ch, int layout,
                  int inverse, int dtype, void *stream);

/* ---- K4: DistConvertor_ = Expit_ -> SplineNet_ (shared knots) -> Logit_ ------
 * Replaces src/nn/scalar/modules_.py:93-114, 277-302, 333-358 with ONE pass over
 * the field.  The spline is shared by all sites; its K knots, already augmented for
 * the boundary condition (src/lib/spline/spline.py:458-532; O(m) host-side work on
 * the learned logits), are staged in LDS by the kernels.
 *
 *   knots   3*K values of dtype: x[0..K) | y[0..K) | d[0..K), K <= 512
 *   stages  bit0 = expit before, bit1 = spline, bit2 = logit after
 *           (DistConvertor_ = 7, a bare SplineNet_ = 2)
 *   inverse runs the inverse chain (the reversed list of inverted stages,
 *           src/nn/_core.py:69-72)
 *   x, y    (B, V);  log0, logj (B)
 */
int nf_distconv(const void *x, const void *knots, int K, const void *log0, void *y, void *logj,
                int64_t B, int64_t V, int stages, int inverse, void *workspace,
                size_t workspace_bytes, int dtype, void *stream);
/* VJP: grad_in (B,V) and grad_knots (3K DOUBLES, summed over the whole field,
 * overwritten by the call).  `v` is the forward chain's input (inverse=0) or the
 * inverse chain's OUTPUT (inverse=1). */
int nf_distconv_vjp(const void *v, const void *knots, int K, const void *grad_out,
                    const void *grad_logj, void *grad_in, double *grad_knots, int64_t B,
                    int64_t V, int stages, int inverse, void *workspace,
                    size_t workspace_bytes, int dtype, void *stream);

/* ---- K4 per site: Module_.propagate_density on Expit_ / SplineNet_ / Logit_ and their
 * fused triple (src/nn/_core.py:19,38-42 with src/nn/scalar/modules_.py:93-114, 277-302),
 * and InvisibilityMaskWrapperModule_ around one of them (src/nn/_core.py:196-231: split,
 * net_ on the visible part, purify(channel=0), sum_density, cat) as ONE masked pass.
 * Stages, knots and directions as nf_distconv.
 *   mask    (V) uint8 activity bytes or NULL (all active).  Where 0: y = x, the site's
 *           log-density is 0 and the site is not evaluated.
 *   mode    NF_DC_SITES: site_out (B, V) = log0 + log|f'| per site; log0 (B, V) or NULL;
 *                        logj unused.
 *           NF_DC_SUM:   logj (B) = log0 + sum of log|f'| over the ACTIVE sites; log0 (B)
 *                        or NULL; site_out unused.  Scratch: nf_workspace_bytes(B, V).
 */
enum nf_distconv_mode { NF_DC_SUM = 0, NF_DC_SITES = 1 };
int nf_distconv_sites(const void *x, const void *knots, int K, const void *log0, const uint8_t *mask,
                      void *y, void *site_out, void *logj, int64_t B, int64_t V, int stages, int inverse,
                      int mode, void *workspace, size_t workspace_bytes, int dtype, void *stream);
/* VJP of nf_distconv_sites, arguments as nf_distconv_vjp: grad_logj is (B, V) in
 * NF_DC_SITES mode and (B) in NF_DC_SUM mode; inactive sites pass grad_out through and add
 * nothing to grad_knots (3K doubles, per-workgroup partials then one reduction). */
int nf_distconv_sites_vjp(const void *v, const void *knots, int K, const uint8_t *mask, const void *grad_out,
                          const void *grad_logj, void *grad_in, double *grad_knots, int64_t B, int64_t V,
                          int stages, int inverse, int mode, void *workspace, size_t workspace_bytes,
                          int dtype, void *stream);

/* ---- Pade11_ / Pade22_: learnable monotone maps of [0, 1] with per-channel parameters --
 * Replaces src/nn/scalar/modules_.py:117-222 (forward and backward of both modules: ~15
 * eager element-wise ops plus Module_.sum_density, src/nn/_core.py:38-42) with ONE pass:
 *   NF_PADE11  y = x / (x + d (1 - x))                                     (d = d0; d1 unused)
 *   NF_PADE22  y = x (x + d0 (1 - x)) / (1 + (d0 + d1 - 2) x (1 - x))
 * inverse = 1 applies the inverse map (Pade11: x / (x + (1 - x) / d); Pade22: the root
 * 2y / (-b + sqrt(b^2 - 4 a y)), b = (d0 + d1 - 2) y - d0, a = -1 - b, with no a == 0
 * branch) and adds log|dx/dy| (Pade22: -log f'(x) at the recovered x).  No clamping.
 * The same pass carries the site-local maps of the real line (modules_.py:72-90, 225-274):
 *   NF_TANH    y = tanh x, log|f'| = -2 (|x| + log1p(e^{-2|x|}) - ln 2): finite for every finite
 *              x, where the reference's log(cosh x) overflows.  No parameters: C = 1, d0 and d1
 *              may be NULL.  inverse = 1: atanh, log = -(log1p(x) + log1p(-x))
 *   NF_PADE32  y = x (a + x^2) / (1 + a x^2), a = d0 in (0, 3) per channel (the caller maps
 *              3 expit(w0)); d1 unused.  inverse = 1: the one real root of
 *              x^3 - a y x^2 + a x - y = 0 (scaled Cardano + two Newton steps; odd, 0 at 0,
 *              finite for every finite y), log = -log f'(x) at that root
 *
 *   x, y      the field as (outer, C, inner), dense; B samples of outer*C*inner / B elements
 *             each (a sample is whole rows of `inner`: B divides outer*C, and the rows per
 *             sample are a multiple of C, or 1 when the channel axis is the batch axis)
 *   d0, d1    C values of dtype each: the per-channel parameters, already softplus(beta=ln2)
 *             mapped (modules_.py:156-163, 210-220); channel of element (o, c, i) = c
 *   per_site  0: log0 / logj are (B): logj = log0 + the per-sample sum of log|f'|;
 *             1: log0 / logj have the shape of x: logj = log0 + log|f'| at every element
 *             (Module_.propagate_density, src/nn/_core.py:19,38-42)
 *   log0      NULL = 0
 * Scratch: nf_pade_workspace_bytes(B, outer, C, inner) bytes (none for per_site map calls).
 */
enum nf_pade_kind { NF_TANH = 1, NF_PADE11 = 11, NF_PADE22 = 22, NF_PADE32 = 32 };
size_t nf_pade_workspace_bytes(int64_t B, int64_t outer, int64_t C, int64_t inner);
int nf_pade(const void *x, const void *d0, const void *d1, const void *log0, void *y, void *logj, int64_t B,
            int64_t outer, int64_t C, int64_t inner, int kind, int inverse, int per_site, void *workspace,
            size_t workspace_bytes, int dtype, void *stream);
/* VJP of nf_pade: x is the forward map's INPUT (inverse = 0) or the inverse map's OUTPUT
 * (inverse = 1), so no root is recomputed.  grad_y has the shape of x; grad_logj is (B)
 * (per_site = 0) or has the shape of x (per_site = 1).  Writes grad_x (shape of x) and
 * grad_d: 2C doubles, the cotangents of d0 (first C; 0 for NF_TANH) and d1 (next C; 0 unless NF_PADE22) summed
 * over batch and sites per workgroup, then per channel in a fixed order (no atomics: the
 * same inputs give the same bits). */
int nf_pade_vjp(const void *x, const void *d0, const void *d1, const void *grad_y, const void *grad_logj,
                void *grad_x, double *grad_d, int64_t B, int64_t outer, int64_t C, int64_t inner, int kind,
                int inverse, int per_site, void *workspace, size_t workspace_bytes, int dtype, void *stream);

/* ---- the power-spectrum filter of FFTNet_ / PSDBlock_ in the separable real Hartley basis ----
 * Replaces src/nn/scalar/fftflow_.py:98-176 (rfftn, multiply, irfftn) and, with the zero mode replaced, the mean-field
 * split of src/nn/scalar/psd_.py:17-57 with ONE launch in which the sample never leaves LDS:
 *   y_b = T D_b T x_b,   T = H_{N_1} x ... x H_{N_d},   H_N[k, n] = (cos(2 pi k n / N) + sin(2 pi k n / N)) / sqrt(N),
 *   D_b(k) = w_half[k_1, .., min(k_d, N_d - k_d)], except D_b(0) -> the coefficient is SET to zero_new[b] when given.
 * For a weight that is even in every k_mu separately (w = sigma(khat^2)^(-1/2) is) this equals
 * irfftn(rfftn(x) w_half, s = lattice) for any axis lengths, odd ones included.
 *   x, y       (B, V) fields, dense, of dtype (NF_F32 / NF_F64); y may be x
 *   w_half     the weight on the rfftn grid, (N_1, .., N_d / 2 + 1), of dtype
 *   zero_new   (B) or NULL;  zero_old (B) or NULL: receives (T x_b)(0) = sum(x_b) / sqrt(V)
 *   lat, ndim  the ndim <= 4 axis lengths, each <= 64
 * nf_spectral_supported(lat, ndim, dtype, for_vjp): 1 when the sample (for_vjp: the sample and its cotangent) and the
 * Hartley matrices fit the 160 KiB of LDS -- every 1- to 4-D lattice up to 64 KiB per sample does --, else 0 with the
 * reason in nf_last_error_string; launches nothing.
 * nf_spectral_filter_vjp: T D T is symmetric, so gx_b = T D_b T g_b (mode 0 dropped when zero_replaced);
 * gzero[b] = (T g_b)(0) ((B) or NULL); gw_half[k] = sum_b sum_{k' folding onto k} (T g_b)(k') (T x_b)(k') (entry 0 is 0
 * when zero_replaced), summed per workgroup and then over the workgroups in a fixed order: no atomics, the same inputs
 * give the same bits.  NOTE: entry by entry gw_half is not the gradient autograd derives through rfftn (the Hartley modes
 * of a symmetry orbit (+-k_1, .., +-k_d) mix differently from the Fourier pairs); the sums over each orbit agree, so every
 * parameter behind a weight that depends on k through khat^2 gets the same gradient.
 * Scratch of the VJP: nf_spectral_workspace_bytes(lat, ndim, B, dtype) bytes. */
int nf_spectral_supported(const int32_t *lat, int ndim, int dtype, int for_vjp);
size_t nf_spectral_workspace_bytes(const int32_t *lat, int ndim, int64_t B, int dtype);
int nf_spectral_filter(const void *x, const void *w_half, const void *zero_new, void *y, void *zero_old,
                       const int32_t *lat, int ndim, int64_t B, int dtype, void *stream);
int nf_spectral_filter_vjp(const void *x, const void *g, const void *w_half, int zero_replaced, void *gx, void *gw_half,
                           void *gzero, void *workspace, size_t workspace_bytes, const int32_t *lat, int ndim, int64_t B,
                           int dtype, void *stream);

/* ---- K5: circular 'same' convolution + bias + activation on the f32 matrix cores ----
 * Replaces one Conv{1,2,3}d(padding='same', padding_mode='circular') / Conv4d layer of
 * ConvAct together with the activation that follows it (src/nn/scalar/modules.py:120-145,
 * src/nn/scalar/convNd.py:86-126).  Lattices of dimension d < 4 are passed with leading
 * axes of extent 1 and kernel extent 1.
 *
 *   in      (B, cin, V) f32, channel planes (the layout of a torch (B, C, *L) tensor)
 *   wfrag   weights in MFMA-fragment order.  nf_conv_packed_steps(cin, ntaps) == 0 (cin a multiple
 *           of 4, or cin >= 8): [tap][ceil(cin/4)][ceil(cout/16)][4][16],
 *           wfrag[t][q][n][g][j] = W[16n + j][4q + g][t];
 *           otherwise (cin in {1,2,3,5,6,7}) K-packed: [step][ceil(cout/16)][4][16] with
 *           wfrag[s][n][g][j] = W[16n + j][kk % cin][kk / cin], kk = 4s + g, for
 *           s < nf_conv_packed_steps(cin, ntaps); 0 where out of range; taps in row-major
 *           kernel order
 *   bias    (cout) or NULL
 *   out     (B, cout, V), or with compact != 0 (B, cout, V/2): only the site of every
 *           aligned pair (2h, 2h+1) whose coordinate sum has parity `active_parity`
 *           (NF_LAYOUT_PAIR input of the coupling kernels)
 *   act     0 none, 1 tanh, 2 relu, 3 leaky_relu(0.01), 4 softplus, 5 abs, 6 sigmoid
 */
/* nf_conv_two_site(cout, compact, L3, k3) != 0: the layer is computed with two-site column packing
 * (cout <= 8): pass wfrag packed from the (16, cin, k0, k1, k2, k3+1) tensor W2 with
 * W2[o][..][t3] = W[o][..][t3] (t3 < k3) and W2[8+o][..][t3] = W[o][..][t3-1] (t3 >= 1), else 0. */
int nf_conv_two_site(int cout, int compact, int l3, int k3);
int nf_conv_cin_pad(int cin);
int nf_conv_ntiles(int cout);
int nf_conv_packed_steps(int cin, int ntaps);
/* `compact`: 0 = (B, cout, V) planes; 1 = pair-compact (B, cout, V/2), active sites only; NF_OUT_SPLIT16 (2) = the full
 * lattice as the fp16 (hi, lo) PAIR TENSOR of 8-output-channel two-site layers -- what nf_conv_fwd_split16 reads and writes
 * and nf_conv_rqs(flags = NF_CONV_UNIT_INPUT | NF_CONV_SPLIT16_INPUT) reads; same bytes as the 8 fp32 planes, (B, V, 16) halfs:
 *   per lattice row (the L3 sites of the fastest axis; rows in row-major order of the other axes) L3*32 bytes =
 *     [hi | lo][even sites | odd sites][L3/2 slots][8 channels], hi = fp16(a), lo = fp16(a - hi);
 *   the even block holds site 2s in slot s, the odd block site 2s - 1 (mod L3) in slot s.
 * A row is thus a contiguous image that LDS-DMA copies as it stands (L3 = 32: exactly one 1 KiB wave-instruction), every
 * 16-byte entry is one k-group of an MFMA A fragment, and a tap-by-tap read of the image is free of LDS bank conflicts. */
enum { NF_OUT_SPLIT16 = 2 };
int nf_conv_fwd(const void *in, const void *wfrag, const void *bias, void *out, int64_t B,
                const int32_t *lattice, const int32_t *ksize, int cin, int cout, int act,
                int compact, int active_parity, int dtype, void *stream);
/* Weight layout nf_conv_fwd / nf_conv_rqs (fused != 0) expects for this layer; pure planning, no GPU work.
 *   NF_WLAYOUT_FRAGMENT (0): the fragment order above, [tap][cin_pad/4][ntiles][4][16];
 *   NF_WLAYOUT_ROWPACK  (1): [row][cin_pad/4][64][NV], row = the taps of all axes but the fastest (row-major),
 *       lane = 16*(channel within the quad) + (column within its tile), value index v = j3*ntiles + tile for
 *       tap j3 < K3 along the fastest axis (K3 = k3, or k3 + 1 with two-site packing), NV = K3*ntiles rounded
 *       up to a multiple of 4 (zero fill).  I.e. fragment order permuted so that everything a lane needs for one
 *       kernel row sits in NV/4 16-byte words.  Used by the persistent kernel (fp32, cin % 4 == 0, k3 == 3,
 *       <= 48 output columns).
 *   NF_WLAYOUT_SPLIT16  (2): fp16 pairs for the split-fp16 kernel, [column tile (3)][K slice (21)][hi|lo][64 lanes][8]:
 *       slice 7*j3 + i = tap j3 (fastest axis) of kernel rows 4i..4i+3 ((j0, j1, j2) row-major; row 27 = zeros);
 *       lane = 16*g + n holds, for column 16*tile + n, the 8 input channels of kernel row 4i + g;
 *       hi = fp16(1024 w), lo = fp16(1024 w - hi) (the factor 2^10 keeps the lo parts of typical weights out of
 *       fp16's subnormal range; the kernel scales the accumulators back).  Needs finite weights with
 *       max|w| < 3.0e4 / 1024 = 29.296875 (normflow__amd._hip.SPLIT16_WEIGHT_LIMIT: 29.29 runs here, 29.30 and NaN / inf
 *       weights run the fp32 kernels).  Weights of any smaller size are taken: where the lo parts fall below fp16's
 *       subnormal step the error of an output degrades to the floor 2^-25 sum|w| + 2^-35 sum|x| over its terms, never to
 *       NaN (tests/split16_range_cases.py states the bound, tests/test_split16_range.py holds every entry point to it).
 * `fused`: bit 0 = the layer is the fused last layer (nf_conv_rqs), bit 1 = NF_CONV_UNIT_INPUT will be passed, bit 2 =
 * NF_CONV_SPLIT16_INPUT will be passed (the split-fp16 kernel takes fastest axes other than 32 sites only from a pair tensor).
 * Returns the code, or -1 for invalid arguments. */
enum { NF_WLAYOUT_FRAGMENT = 0, NF_WLAYOUT_ROWPACK = 1, NF_WLAYOUT_SPLIT16 = 2 };
int nf_conv_weight_layout(const int32_t *lattice, const int32_t *ksize, int cin, int cout, int compact,
                          int fused, int dtype);
/* A hidden 8 -> 8 layer whose input AND output are the fp16 (hi, lo) pair tensor above (nf_conv_g.hip: two-site columns,
 * one v_mfma_f32_16x16x32_f16 slice per kernel row, three fp16 products per fp32 product; persistent workgroups marching
 * 2 x 2 columns of lattice rows through an LDS ring filled by LDS-DMA).  in16 and out16 must not overlap.
 *   in16, out16: (B, V, 16) halfs; wsplit: 72 fragments of [64 lanes][8] halfs, scaled by 2^10 and split as in
 *   NF_WLAYOUT_SPLIT16.  First 18 STACKED fragments [set (2)][j2 (3)][j3 (3)]: lane 16*g + n holds, for row n = 8*part + co
 *   (part 0: hi, 1: lo), the 8 input channels of kernel row (j0, j1, j2) with 3 j0 + j1 = 4*set + g, tap j3.  Then the
 *   two-site fragments [kernel row (27)][hi|lo]: lane 16*g + n holds, for column n = 8*shift + co, the 8 input channels of
 *   tap (g - shift) of that kernel row (zero outside 0..2).  normflow__amd._hip.pack_conv_weight_split16_stacked packs it.
 *   bias (8) fp32 or NULL; act must keep |out| <= 1 (tanh, logistic).
 *   nf_conv_split16_supported: 3^4 kernel, 8 -> 8 channels, a fastest axis of 32 + 16 n sites, even other extents. */
int nf_conv_split16_supported(const int32_t *lattice, const int32_t *ksize, int cin, int cout, int act);
/* The LAST layer of an AffineCoupling_'s net (8 -> 2 channels: t, s) fused with the coupling (src/nn/scalar/couplings_.py:123-139),
 * fed by a pair tensor: y = t + x e^{-|s|}, logj = log0 - sum|s| (inverse != 0: x = (y - t) e^{|s|}, + sum|s|) at the active
 * site of every pair, 0 at the frozen one; the (B, 2, V/2) parameter tensor never exists in memory.  Same kernel as
 * nf_conv_fwd_split16 with another epilogue.
 *   wsplit: the hidden-layer fragment format of nf_conv_fwd_split16 packed from the (8, 8, 3,3,3,3) tensor whose output
 *   channels 0, 1 are the layer's weights and 2..7 zero; bias (8) fp32 (entries 0, 1 used) or NULL; x_active, y (B, V) fp32 --
 *   or IEEE half with flags = NF_CONV_FIELD_F16; log0 (B) or NULL, logj (B): fp32; workspace as nf_workspace_bytes(B, V). */
int nf_conv_affine_split16(const void *in16, const void *wsplit, const void *bias, const void *x_active, const void *log0,
                           void *y, void *logj, int64_t B, const int32_t *lattice, int active_parity, int inverse,
                           int flags, void *workspace, size_t workspace_bytes, void *stream);
/* The FIRST ConvAct layer (1 -> 8 channels, 3^4 kernel, tanh / logistic) in front of the two entry points above (nf_conv_c.hip):
 * fp32 field in, fp16 pair tensor out, every fp32 product as three fp16 matrix-core products (x = x_hi + x_lo, |x| up to
 * fp16's largest finite number: 65519 still rounds to 65504 and is taken; a site of 65520 and beyond, inf or NaN makes every
 * output whose window holds it NaN -- never a finite wrong number -- and leaves the outputs further away than the window
 * plus the two zero-weight taps of the two-site columns bit for bit as they were.  Small |x| lose nothing that matters: the
 * lo part carries an absolute error of 2^-25 = 3e-8.  Saturated pre-activations give exactly +-1 (tanh), 0 or 1 (logistic)
 * with a zero lo part).
 *   in (B, V) fp32 (the frozen half of the field, one channel); out16 (B, V, 16) halfs; bias (8) fp32 or NULL;
 *   wsplit: [K slice (4)][hi|lo][64 lanes][8] halfs: K index = 4 r + t, r = kernel row (j0, j1, j2) row-major (27, padded to
 *   32 with zeros), t = tap of the site pair (sites 2p-1 .. 2p+2); lane 16*g + n (column n = 8*shift + co) holds rows
 *   8*slice + 2*g + h (h = 0, 1) as values 4*h + t = W[co][r][t - shift] (zero outside 0..2), scaled by 2^10 and split as
 *   in NF_WLAYOUT_SPLIT16.  nf_conv_first_split16_supported: 8 output channels, 3^4 kernel, a fastest axis of 32 + 16 n
 *   sites, even other extents.
 *   Frozen-parity flags, ORed into `act` (both entry points mask them off before they look at the activation): with
 *   NF_FIRST_FROZEN_EVEN / NF_FIRST_FROZEN_ODD the caller states that `in` is non-zero only at the sites whose coordinate sum
 *   x0 + x1 + x2 + x3 is even / odd (the frozen half of a checkerboard coupling).  On lattices with L3 % 32 == 0, L0 % 4 == 0
 *   and L1 % 4 == 0 the parity-compact instance then runs: it LOADS those sites only (whatever stands at the others is never
 *   read) and multiplies K = 27 rows x 2 live taps.  Every other supported lattice runs the dense kernel on `in` as it is.
 *   A flagged call states the size of its blob with NF_FIRST_FRAGS(16): the 8 dense fragments above, then
 *   [sigma (2)][K slice (2)][hi|lo][64 lanes][8]: sigma = (output row parity x0 + x1 + x2) ^ (frozen parity), K index =
 *   2 r + t', lane 16*g + n holds rows 16*slice + 4*g + h (h = 0..3) as values 2*h + t' = W[co][r][t - shift] at the live
 *   taps t = 1 - e + 2 t', e = sigma ^ (j0 + j1 + j2 + 1) & 1 (zero outside 0..2 and for r >= 27); scaled and split as the
 *   dense ones.  A flagged call without it is refused (NF_EINVAL).  Without a flag nothing changes. */
#define NF_FIRST_FROZEN_EVEN 0x100
#define NF_FIRST_FROZEN_ODD 0x200
#define NF_FIRST_FRAGS_MAX 0xff
#define NF_FIRST_FRAGS(n) ((int)(n) << 16)
int nf_conv_first_split16_supported(const int32_t *lattice, const int32_t *ksize, int cout, int act);
int nf_conv_first_split16(const void *in, const void *wsplit, const void *bias, void *out16, int64_t B,
                          const int32_t *lattice, int act, void *stream);
int nf_conv_fwd_split16(const void *in16, const void *wsplit, const void *bias, void *out16, int64_t B,
                        const int32_t *lattice, int act, void *stream);
/* What nf_conv_fwd (fused = 0; compact = 0, 1 or 2 = NF_OUT_SPLIT16) or nf_conv_rqs (fused bit 0 set; bits 1 and 2 as for
 * nf_conv_weight_layout, knots_len = (cout + 2) / 3) will do with this layer for a batch of B under the current options:
 * the planner the two entry points execute, pure host code (no device needed, no pointer but the extents looked at).
 *   path               the code nf_conv_last_path reports after the launch: 0 one box per workgroup, 1 persistent pipelined
 *                      kernel, 2 single-input-channel kernel, 3 split-fp16 fused kernel
 *   weight_layout      NF_WLAYOUT_* that kernel reads (what nf_conv_weight_layout returns)
 *   mt                 16-site tiles per wave: a box holds 4 mt 16 output units (0 for path 3, whose box is fixed)
 *   two_site, packed   two-site column packing (cout <= 8), K-packed reduction (cin % 4 != 0, cin < 8)
 *   box, nbox          sites of a box and boxes per axis; a workgroup (or work item of a persistent kernel) is one box of one sample
 *   plane_stride       elements between the channel planes of the staged box + halo in LDS (0 for path 3)
 *   channels_per_pass  input channels staged per pass of the reduction loop
 *   launches           kernel launches (path 0: one per 48 output columns)
 *   lds_bytes          dynamic LDS of a launch
 *   partials           log-det partials per sample (fused layers: the workspace must hold B x partials doubles), else 0
 * Grid sizes are not part of the plan: the persistent kernels size theirs by the device's CU count and occupancy.
 * Returns what the entry point would: NF_EINVAL with its message for a layer or batch it refuses.  nf_conv_weight_layout is
 * this plan's weight_layout at B = 1, except that a pair-tensor layer (bit 2) which the split-fp16 kernel does not take is
 * answered with the layout of the fp32 kernel it would need, not refused.  An added entry point leaves NF_VERSION as it is. */
typedef struct nf_conv_layer_plan {
  int32_t path;
  int32_t weight_layout;
  int32_t mt;
  int32_t two_site;
  int32_t packed;
  int32_t box[4];
  int32_t nbox[4];
  int32_t plane_stride;
  int32_t channels_per_pass;
  int32_t launches;
  int64_t lds_bytes;
  int64_t partials;
} nf_conv_layer_plan;
int nf_conv_plan(const int32_t *lattice, const int32_t *ksize, int cin, int cout, int compact, int fused, int dtype,
                 int64_t B, nf_conv_layer_plan *out);
/* Which kernel the calling thread's last nf_conv_fwd / nf_conv_rqs launched: 0 = one box per workgroup
 * (nf_conv.hip), 1 = persistent workgroups with staging overlapped with the MFMAs (nf_conv_pipe.hip;
 * fp32, cin % 4 == 0, kernel extent 3 on the fastest axis), 2 = the single-input-channel kernel of the first
 * ConvAct layer (nf_conv_pipe.hip, conv_c1_kernel), 3 = the split-fp16 fused kernel (nf_conv_h.hip).  For tests and benches. */
int nf_conv_last_path(void);

/* ---- K5+K2 fused: last conv layer of the parameter net + RQ-spline coupling ---------------
 * The (B, 3m-2, V/2) logit tensor is produced in the MFMA accumulators, staged in LDS and
 * consumed by the spline map in the same workgroup; it never goes to HBM (SURVEY 8(f) item 1:
 * src/nn/scalar/modules.py:120-145 feeding src/nn/scalar/couplings_.py:178-200).
 * Inference only (no VJP); needs a plain even-odd activity pattern (`active_parity` = parity of
 * the coordinate sum of the active sites), an even fastest axis, knots_len in {4, 8, 16}.
 *   in (B, cin, V) hidden activations; wfrag/bias as nf_conv_fwd with cout = 3m-2;
 *   x_active, y (B, V); log0, logj (B); inverse != 0 applies the inverse map.
 *   flags: NF_CONV_UNIT_INPUT = the caller guarantees |in| <= 1 (hidden activations that are tanh / sigmoid
 *   outputs): eligible layers (8 -> 46 channels, 3^4 kernel, a fastest axis of 32 sites -- or, fed by a pair tensor, 32 + 16 n --, even
 *   other extents) then run the split-fp16 kernel
 *   (nf_conv_h.hip): every fp32 product as three fp16 matrix-core products with fp32 accumulation, ~1.7x the
 *   rounding error of an fp32 chain, well inside the 1e-5 budget; the weights must then be packed in
 *   NF_WLAYOUT_SPLIT16 (nf_conv_weight_layout with `fused` = 1 | 2 says which layout a layer wants).
 */
/*   NF_CONV_SPLIT16_INPUT (with NF_CONV_UNIT_INPUT): `in` is not (B, 8, V) fp32 but what the previous layer wrote
 *   with nf_conv_fwd(compact = NF_OUT_SPLIT16): (B, V, 16) IEEE halfs = per site hi[8] | lo[8]. */
/*   NF_CONV_FIELD_F16: x_active and y are IEEE half (fp16 field storage; the arithmetic stays fp32 and log0 / logj stay fp32:
 *   BASELINE config 5, "fp16 params / fp32 log-det accumulate" -- in the fused path the "params" never exist in memory). */
enum { NF_CONV_UNIT_INPUT = 1, NF_CONV_SPLIT16_INPUT = 2, NF_CONV_FIELD_F16 = 4 };
int nf_conv_rqs_supported(int cout, int m);
/* Planning query for the split-fp16 chain: its fused last layer takes ANY knots_len 2 <= m <= 16 (cout = 3m - 2 <= 46
 * logit channels: the reference leaves knots_len free, src/nn/scalar/couplings_.py:211-262) on 4-D lattices with even
 * extents and a fastest axis of 32 + 16 n sites, fed by the pair tensor (NF_CONV_UNIT_INPUT | NF_CONV_SPLIT16_INPUT).
 * Hidden widths below 8 run the same kernels on weights zero-padded to 8 channels (the host packs them). */
int nf_conv_rqs_split16_supported(const int32_t *lattice, int cout, int m);
int nf_conv_rqs(const void *in, const void *wfrag, const void *bias, const void *x_active,
                const void *log0, void *y, void *logj, int64_t B, const int32_t *lattice,
                const int32_t *ksize, int cin, int cout, int active_parity,
                const nf_rqs_opts *opts, int inverse, int flags, void *workspace, size_t workspace_bytes,
                int dtype, void *stream);

/* ---- end points of the flow ------------------------------------------------
 * nf_phi4_action: S[b] = sum_x (w2 phi^2 + w4 phi^4) - w0 sum_mu sum_x phi(x) phi(x - mu), periodic
 * (ScalarPhi4Action.action, src/action/scalar_action.py:38-46; w0, w2, w4 from get_coef, :24-36):
 * ONE pass instead of the reference's d+1.  cfgs (B, V), lattice[4] (leading extents 1 for d < 4),
 * action (B).  nf_phi4_action_vjp: grad_cfgs = grad_action[b] * dS/dphi.
 * nf_normal_logprob: logp[b] = sum_x [-(x-loc)^2/(2 s^2) - log s - log sqrt(2 pi)], loc/scale (V)
 * or NULL (0 / 1) (Prior.log_prob with torch.distributions.Normal, src/prior/prior.py:30-36).
 */
int nf_phi4_action(const void *cfgs, void *action, int64_t B, const int32_t *lattice, double w0, double w2,
                   double w4, void *workspace, size_t workspace_bytes, int dtype, void *stream);
int nf_phi4_action_vjp(const void *cfgs, const void *grad_action, void *grad_cfgs, int64_t B,
                       const int32_t *lattice, double w0, double w2, double w4, int dtype, void *stream);
/* nf_phi4_action_density: the per-site action (ScalarPhi4Action.action_density,
 * src/action/scalar_action.py:48-62; the reference's 1 + 2d passes), ONE stencil pass:
 *   density[b, x] = wm phi^2 + w4 phi^4
 *                   + (w0 / 4) sum_mu [(phi(x) - phi(x + mu))^2 + (phi(x) - phi(x - mu))^2]
 * with wm = w2 - d w0 (= m^2 a^d / 2), periodic; an axis of extent 1 adds nothing.  Its sites
 * sum to the action.  cfgs, density (B, V).  nf_phi4_action_density_vjp: grad_cfgs from the
 * per-site cotangent grad_density (B, V), one pass. */
int nf_phi4_action_density(const void *cfgs, void *density, int64_t B, const int32_t *lattice, double w0,
                           double wm, double w4, int dtype, void *stream);
int nf_phi4_action_density_vjp(const void *cfgs, const void *grad_density, void *grad_cfgs, int64_t B,
                               const int32_t *lattice, double w0, double wm, double w4, int dtype, void *stream);
int nf_normal_logprob(const void *x, const void *loc, const void *scale, void *logp, int64_t B, int64_t V,
                      void *workspace, size_t workspace_bytes, int dtype, void *stream);
int nf_normal_logprob_vjp(const void *x, const void *loc, const void *scale, const void *grad_logp,
                          void *grad_x, int64_t B, int64_t V, int dtype, void *stream);
/* Folded (XOR) into the high key word of nf_normal_sample's Philox generator: separates its streams from torch's own
 * Philox kernels, which key on the bare seed. */
#define NF_PHILOX_KEY_DOMAIN 0x6e66686bu   /* 'nfhk' */

/* nf_normal_sample: Prior.sample_ for a NormalPrior (src/prior/prior.py:26-29 with :30-36 and :92-101) in ONE launch:
 * x[b, i] = loc[i] + scale[i] z[b, i] with z standard normal, and logr[b] = sum_i [-z^2/2 - log scale[i] - log sqrt(2 pi)]
 * accumulated from the z still in registers (the reference draws, then re-reads the field for log_prob, then sums).
 * Generator: Philox4x32-10 (Salmon et al., SC'11; the Random123 / cuRAND / torch generator), counter-based and stateless:
 *   group q = i / 4 (float32: four normals per call) or i / 2 (float64: two), g = b * ceil(V / per) + q,
 *   counter = (lo32 g, hi32 g, lo32 offset, hi32 offset), key = (lo32 seed, hi32 seed), outputs r0..r3;
 *   float32: (z0, z1) = rho (cos, sin)(2 pi u2) with u1 = (r0 + 1) 2^-32, u2 = r1 2^-32, rho = sqrt(-2 ln u1); (z2, z3) from (r2, r3);
 *   float64: u1 = ((r0 << 21 ^ r1 >> 11) + 1) 2^-53, u2 = (r2 << 21 ^ r3 >> 11) 2^-53.
 * The caller owns the stream position: advance `offset` by 1 per call (the host mirror takes seed and offset from torch's
 * CUDA generator, so torch.manual_seed governs this kernel too).  loc / scale: (V) or NULL (0 / 1). */
int nf_normal_sample(void *x, void *logr, const void *loc, const void *scale, int64_t B, int64_t V, uint64_t seed,
                     uint64_t offset, void *workspace, size_t workspace_bytes, int dtype, void *stream);
/* nf_normal_sample_rows: rows first_row .. first_row + B - 1 of the stream above, written to x (B, V) and logr (B): row b of
 * the launch draws the groups g = (first_row + b) * ceil(V / per) + q.  A batch beyond the grid's 65535 rows is drawn in
 * slabs at ONE offset, and is the same numbers however it is cut; nf_normal_sample is first_row = 0. */
int nf_normal_sample_rows(void *x, void *logr, const void *loc, const void *scale, int64_t B, int64_t V, int64_t first_row,
                          uint64_t seed, uint64_t offset, void *workspace, size_t workspace_bytes, int dtype, void *stream);

/* ---- blocked Metropolis on the device (BlockedMCMCSampler, src/mcmc/mcmc.py:132-220; block updater
 * src/prior/prior.py:106-112, 161-178) for C independent chains.  x is the chains' prior-side field (C, V); block k is the
 * sites [k block_len, (k+1) block_len) of every chain.  Neither entry allocates, copies or synchronises: both can be
 * captured into a HIP graph.  fp32 and fp64.
 *
 * nf_block_propose: backup[c, j] = x[c, k block_len + j], then x[c, k block_len + j] = loc[s] + scale[s] z[c, j] with
 * s = k block_len + j: the block's OWN sites' loc / scale ((V) or NULL: 0 / 1).  Sites outside the block are not touched.
 * z is exactly what nf_normal_sample draws for a (B = C, V = block_len) field with the same seed and offset (its layout
 * above: group q = j / 4 (fp32) or j / 2 (fp64), g = c ceil(block_len / per) + q, counter = (lo32 g, hi32 g, lo32 offset,
 * hi32 offset), key = (lo32 seed, hi32 seed ^ NF_PHILOX_KEY_DOMAIN)), i.e. the block is
 * oracle/nf_oracle.py::normal_prior_sample(seed, offset, C, block_len, loc_blk, scale_blk).
 *
 * nf_block_accept: per chain c one uniform from counter = (lo32 c, hi32 c, lo32 offset, hi32 offset) and key =
 * (lo32 seed, hi32 seed ^ NF_PHILOX_ACCEPT_DOMAIN) -- a key domain of its own, so the uniforms never share a stream with
 * the normals -- u = ((r0 << 21 ^ r1 >> 11) + 1) 2^-53 in (0, 1]; in double:
 *   accept = force_accept || log u < logqp_ref[c] - (logq[c] - logp[c]).
 * Accepted: logqp_ref[c] = logq[c] - logp[c].  Rejected: the block of x[c] is copied back from backup[c], bitwise.
 * accept_out[c] = accept (uint8).  logq / logp (C) are of the field dtype, logqp_ref (C) is double for either.
 * The caller owns the stream positions, as for nf_normal_sample: a fresh offset per launch. */
#define NF_PHILOX_ACCEPT_DOMAIN 0x6e666163u   /* 'nfac' */
int nf_block_propose(void *x, void *backup, const void *loc, const void *scale, int64_t C, int64_t V, int64_t block_len,
                     int64_t block_ind, uint64_t seed, uint64_t offset, int dtype, void *stream);
int nf_block_accept(void *x, const void *backup, const void *logq, const void *logp, double *logqp_ref,
                    uint8_t *accept_out, int64_t C, int64_t V, int64_t block_len, int64_t block_ind, int force_accept,
                    uint64_t seed, uint64_t offset, int dtype, void *stream);

/* ---- independence Metropolis on the device (MCMCSampler with n_chains = C; the reference does the accept/reject on the
 * host: MCMCSampler._accept_reject_step, src/mcmc/mcmc.py:56-87, with Metropolis.calc_accept_status and
 * calc_accept_indices, :304-328) for C independent chains over S steps.  The batch of B = S C proposals is laid out as the
 * blocked sampler's: row r = s C + c is step s of chain c.  Neither entry allocates, copies or synchronises: both can be
 * captured into a HIP graph.
 *
 * nf_metropolis_chains: every decision of the C chains over the S steps in ONE launch.  Per row r one uniform from
 * counter = (lo32 r, hi32 r, lo32 offset, hi32 offset) and key = (lo32 seed, hi32 seed ^ NF_PHILOX_CHAIN_DOMAIN) -- a key
 * domain of its own -- u = ((r0 << 21 ^ r1 >> 11) + 1) 2^-53 in (0, 1]; chain c walks s = 0 .. S-1 and decides in double:
 *   accept[r] = (fresh && s == 0) || log u < logqp_ref[c] - (double(logq[r]) - double(logp[r])).
 * Accepted: logqp_ref[c] = double(logq[r]) - double(logp[r]), ref_logq[c] = logq[r], ref_logp[c] = logp[r].
 * keep[r] = the row that holds the configuration chain c has after step s: the last accepted row of the chain up to r,
 * or row c while the chain still holds the state it came in with (then accept[c] == 0, and the configuration is the
 * caller's stored sample of chain c, which nf_metropolis_select puts into row c); keep[r] <= r, keep[r] % C == c.
 * logq_sel[r] / logp_sel[r] = the log q / log p of that configuration (bitwise logq[keep[r]], or the incoming
 * ref_logq[c]), so the host needs no gather.  In: logq, logp (S C) of dtype fp32 or fp64.  In and out: logqp_ref (C)
 * double, ref_logq, ref_logp (C) of dtype: the chains' stored state, on return the state after the last step.  With
 * fresh != 0 the chains have no stored state: the three are not read and every chain accepts its step 0.  Out: accept
 * (S C) uint8, keep (S C) int64, logq_sel, logp_sel (S C) of dtype; they may not overlap the inputs.
 * One launch consumes one offset; the caller owns the stream position, as for nf_normal_sample.
 *
 * nf_metropolis_select: makes y (S C, V), the proposals, the chains' states IN PLACE from accept and keep.  A row with
 * accept[r] != 0 is left as it is.  A rejected row r is overwritten, bitwise, with row keep[r] if accept[keep[r]] != 0,
 * else with ref_sample[r % C] (C, V): the chain still holds its stored sample.  Only rejected rows move.  Rows are
 * copied as bytes: elem_size (1, 2, 4 or 8) is the size of an element of y and ref_sample, any field dtype works.
 * ref_sample may be NULL when no chain can need it (fresh chains: every step-0 row is accepted). */
#define NF_PHILOX_CHAIN_DOMAIN 0x6e666368u   /* 'nfch' */
int nf_metropolis_chains(const void *logq, const void *logp, double *logqp_ref, void *ref_logq, void *ref_logp,
                         uint8_t *accept, int64_t *keep, void *logq_sel, void *logp_sel, int64_t S, int64_t C, int fresh,
                         uint64_t seed, uint64_t offset, int dtype, void *stream);
int nf_metropolis_select(void *y, const void *ref_sample, const uint8_t *accept, const int64_t *keep, int64_t S, int64_t C,
                         int64_t V, int elem_size, void *stream);

/* ---- hybrid Monte Carlo for the phi^4 action, the chain resident in a CU (MI355X-side extension; the action is
 * src/action/scalar_action.py:24-46).  For C independent chains on lattice[4] (leading extents 1 for d < 4), per trajectory:
 *   F(phi)(x) = 2 w2 phi(x) + 4 w4 phi(x)^3 - w0 sum_mu [phi(x + mu) + phi(x - mu)]                      (periodic)
 *   pi ~ N(0, 1)^V;  H0 = sum pi^2 / 2 + S(phi)
 *   pi -= (dt / 2) F(phi);  k = 1 .. n_md: phi += dt pi, pi -= (dt, or dt / 2 when k = n_md) F(phi)
 *   H1 = sum pi^2 / 2 + S(phi);  dH = H1 - H0;  accept = force_accept || log u < -dH,  u in (0, 1]
 * with S of nf_phi4_action.  The field arithmetic is in dtype; the energies are summed and compared in double for either
 * dtype, in a fixed order: no atomics, a launch is bitwise reproducible and n_traj trajectories in one launch equal n_traj
 * launches of one.  No neighbour is read along an axis of extent 1 (a caller that wants ScalarPhi4Action's treatment of a
 * user axis of extent 1 folds -w0 phi^2 per such axis into w2, as for nf_phi4_action); on an axis of extent 2 the one
 * neighbour counts twice; extents need not be even.  A rejected chain keeps its phi bit for bit.
 * One workgroup per chain runs all n_traj trajectories with phi and pi in registers and one image of phi in LDS; the
 * launch neither allocates nor synchronises and can be captured into a HIP graph.
 *   phi        (C, V) of dtype, in and out: the chains' states
 *   action_out (C) double: S of the final states
 *   pi_in      (C, V) or NULL: replaces the drawn momenta (n_traj must be 1);  pi_out (C, V) or NULL: the momenta at the end
 *              of the last trajectory (of the proposal, accepted or not)
 *   dh_out     (n_traj, C) double;  accept_out (n_traj, C) uint8
 *   record     (n_traj / record_every, C, V) of dtype or NULL: the chains' states after every record_every-th trajectory
 * Random numbers: trajectory t draws its momenta as nf_normal_sample draws a unit (B = C, V) field at (seed, offset + 2 t)
 * (group layout and key hi32 seed ^ NF_PHILOX_KEY_DOMAIN above) and its uniform as nf_block_accept does at
 * (seed, offset + 2 t + 1): counter (lo32 c, hi32 c, lo32, hi32 of that offset), key hi32 seed ^ NF_PHILOX_ACCEPT_DOMAIN.
 * A launch consumes the 2 n_traj offsets from `offset` on.
 * nf_phi4_hmc_supported (pure host code, the launcher's own planner): 1 for NF_F32 / NF_F64 when a chain's image fits
 * 64 KiB of LDS, V sizeof(dtype) <= 65536 (16^2, 64^2, 16^3, 8^4 in both, 24^3 and 128^2 in fp32), else 0 with the reason
 * in nf_last_error_string.  The kernel runs ceil(V / ns) lanes (whole waves) per chain, ns = 1, 2, 4, 8 or 16 sites per lane.
 * NF_EINVAL: a NULL phi / action_out / dh_out / accept_out / lattice, C outside 1 .. 65535, n_md, n_traj or record_every
 * < 1, pi_in with n_traj > 1, an unsupported lattice or dtype, or
 *   n_md n_traj max(V, 256) ceil(C / 1024) > NF_HMC_MAX_WORK
 * (below 256 sites the two barriers of an MD step, not the sites, set its time; chains beyond the resident ones wait for
 * a free CU, so the time of a launch grows with every further 1024 chains).  Measured on an MI355X at n_md = 10
 * (tools/hmc_bench.py): 16^2 x 512 chains 0.7 us per MD step, 16^3 x 1024 chains 9 us per MD step; a launch at the cap
 * (with up to 1024 chains 2^18 MD steps at 16^2, 2^14 at 16^3; with 65535 chains a 64th of that) then takes about 0.2 s.
 * Longer runs are split into several launches by the caller.
 *
 * nf_phi4_hmc_measure: nf_phi4_hmc, argument for argument, with the observables of the recorded states taken inside the
 * launch:
 *   measure_out (n_traj / record_every, C, n_out) double: row (r, c) is the row that nf_lattice_measure (below) gives for
 *               the state of chain c after trajectory (r + 1) record_every - 1, BIT FOR BIT -- the 7 scalars and the
 *               slice sums of the four extents of lattice[4], n_out = 7 + their sum as nf_lattice_measure_plan reports it
 *   record      may be NULL (the use of this entry point: no configuration is stored) or given; with both, each output
 *               is what it is alone.  phi, action_out, dh_out, accept_out and pi_out are nf_phi4_hmc's bits.
 * After the decision of a recorded trajectory the workgroup writes the chain's state (the restored one on a reject) into
 * its LDS image and the routine of nf_lattice_measure takes every sum from that image, on the first `lanes` lanes of the
 * workgroup with `lanes` of nf_lattice_measure_plan for the lattice (64 up to 256 sites, 256 up to 4096, 512 beyond);
 * the other waves wait at its barriers.  The same Philox positions as nf_phi4_hmc; it can be captured into a HIP graph.
 * NF_EINVAL: what nf_phi4_hmc refuses, a NULL measure_out, or
 *   (n_md n_traj + NF_HMC_MEASURE_MD_STEPS (n_traj / record_every)) max(V, 256) ceil(C / 1024) > NF_HMC_MAX_WORK:
 * a measured trajectory counts as NF_HMC_MEASURE_MD_STEPS further MD steps.  From the code: an MD step is one pass over
 * the image (2 d + 1 reads and one write per site on all lanes) and 2 barriers.  A measurement is one pass in double with
 * d + 1 reads per site on the team (a quarter to all of the lanes), 7 wave sums of 6 dependent shuffle levels each, then
 * per axis one more read of the whole image by at most 16 stripes per slice, serial within a stripe (extent x 16 lanes
 * at work; 16^3: 256 of 1024 lanes), with 1 + 2 d barriers inside and 3 around the refill of the image: 12 barriers
 * against an MD step's 2 and several times its dependent latency.  Measured on an MI355X (tools/hmc_bench.py --measure,
 * whole sampler calls): about 7 MD steps at 16^3 x 1024 chains and on the order of 10 at 16^2 x 512; 16 covers both.
 *
 * nf_phi4_hmc_plan (pure host code, the launcher's own planner): sites_per_lane and lanes of the workgroup of a chain,
 * the dynamic LDS of a launch of nf_phi4_hmc (lds_bytes) and of nf_phi4_hmc_measure (lds_bytes_measure: 5 KiB of
 * measure slots more); NF_EINVAL where nf_phi4_hmc_supported answers 0. */
#define NF_HMC_MAX_WORK 67108864 /* 2^26 */
#define NF_HMC_MEASURE_MD_STEPS 16
typedef struct nf_hmc_plan {
  int32_t sites_per_lane;
  int32_t lanes;
  int64_t lds_bytes;
  int64_t lds_bytes_measure;
} nf_hmc_plan;
int nf_phi4_hmc_supported(const int32_t *lattice, int dtype);
int nf_phi4_hmc_plan(const int32_t *lattice, int dtype, nf_hmc_plan *out);
int nf_phi4_hmc(void *phi, double *action_out, const void *pi_in, void *pi_out, double *dh_out, uint8_t *accept_out,
                void *record, int record_every, int64_t C, const int32_t *lattice, double w0, double w2, double w4,
                int n_md, double dt, int n_traj, int force_accept, uint64_t seed, uint64_t offset, int dtype,
                void *stream);
int nf_phi4_hmc_measure(void *phi, double *action_out, const void *pi_in, void *pi_out, double *dh_out,
                        uint8_t *accept_out, void *record, double *measure_out, int record_every, int64_t C,
                        const int32_t *lattice, double w0, double w2, double w4, int n_md, double dt, int n_traj,
                        int force_accept, uint64_t seed, uint64_t offset, int dtype, void *stream);

/* ---- the same hybrid Monte Carlo with the chains in HBM and many workgroups per chain (nf_hmc_tiled.hip): for lattices
 * beyond nf_phi4_hmc's 64 KiB image.  The definition, the arguments, the energies in double, the accept rule and the two
 * Philox positions per trajectory are nf_phi4_hmc's, word for word; from the same (seed, offset) both walk the same chain
 * up to rounding.  Field arithmetic is in dtype; the energies are summed in a fixed order (lane partial, wave shuffle
 * tree, waves in order, tiles in order): no atomics, the same inputs give the same bits, n_traj trajectories in one call
 * equal n_traj calls of one at offsets offset + 2 t, and a chain's result does not depend on C or on the chains it shares
 * a call with (the plan depends on the lattice and the dtype alone).  No neighbour is read along an axis of extent 1, on
 * an axis of extent 2 the one neighbour counts twice, extents need not be even.  A rejected chain's phi is never written.
 * A trajectory is n_md + 2 launches in a line on `stream`: begin (the momenta, the energies of the start, the first half
 * kick), n_md fused steps (phi' = phi + dt pi and pi' = pi - eps F(phi') in one pass from one pair of workspace buffers
 * into the other; the last also writes the energies of the end) and commit (the decision, dh_out / accept_out /
 * action_out, the copy of the proposal into the accepted chains, the record row).  The call neither allocates nor
 * synchronises and can be captured into a HIP graph.
 * nf_hmc_tiled_plan, per axis of lattice[4]: a workgroup of `lanes` lanes owns a tile of tile[] sites (the last tile of an
 * axis may be narrower), ntiles[] tiles per axis, `tiles` per chain.  With three or four axes of extent > 1 the slowest
 * of them, march_axis, is walked plane by plane through a ring of ring_depth planes of phi' in LDS (tile[march_axis] is
 * the length of a workgroup's segment); otherwise march_axis = -1 and ring_depth = 0.  An axis that one tile covers has
 * no halo: its neighbours wrap inside the tile.  vec = sites per 16-byte access along the fastest axis (1 when its extent
 * is no multiple of 16 / sizeof(dtype), or when a field handed in is not 16-byte aligned); lds_bytes <= lds_budget.
 * nf_phi4_hmc_tiled_supported (pure host code): 1 for NF_F32 / NF_F64 on any lattice of extents >= 1 with V < 2^31 sites
 * per chain, else 0 with the reason in nf_last_error_string.  nf_phi4_hmc_tiled_workspace (pure host code): the bytes of
 * `workspace` for C chains (two phi and two pi buffers of (C, V) and the (C, tiles, 4) partials), 0 for an unsupported
 * case; the caller owns the workspace (8-byte aligned; 16 for the wide accesses) and it need not be initialised.
 * NF_EINVAL: what nf_phi4_hmc refuses (without its work cap), a short or NULL workspace, tiles x C above 2^24 - 1
 * workgroups, or (n_md + 2) n_traj > NF_HMC_TILED_MAX_LAUNCHES. */
#define NF_HMC_TILED_MAX_LAUNCHES 65536
typedef struct nf_hmc_tiled_plan {
  int32_t tile[4];
  int32_t ntiles[4];
  int32_t tiles;
  int32_t march_axis;
  int32_t ring_depth;
  int32_t lanes;
  int32_t vec;
  int32_t reserved;
  int64_t lds_bytes;
  int64_t lds_budget;
} nf_hmc_tiled_plan;
int nf_phi4_hmc_tiled_supported(const int32_t *lattice, int dtype);
int nf_phi4_hmc_tiled_plan(const int32_t *lattice, int dtype, nf_hmc_tiled_plan *out);
size_t nf_phi4_hmc_tiled_workspace(int64_t C, const int32_t *lattice, int dtype);
int nf_phi4_hmc_tiled(void *phi, double *action_out, const void *pi_in, void *pi_out, double *dh_out, uint8_t *accept_out,
                      void *record, int record_every, int64_t C, const int32_t *lattice, double w0, double w2, double w4,
                      int n_md, double dt, int n_traj, int force_accept, uint64_t seed, uint64_t offset, void *workspace,
                      size_t workspace_bytes, int dtype, void *stream);

/* ---- coupling ladders: per-chain phi^4 couplings and replica exchange (nf_hmc.hip, nf_hmc_tiled.hip, nf_ladder.hip;
 * MI355X-side extension).  C = K R chains; chain c belongs to replica set c / K and holds rung rung[c] in 0 .. K - 1;
 * within a set the rungs are a permutation of 0 .. K - 1 (the identity state is rung[c] = c % K).
 *   coef  (K, 3) double on the device: (w0, w2, w4) of rung k, a user axis of extent 1 already folded into w2
 *   rung  (C) int32 on the device
 * nf_phi4_hmc_ladder: nf_phi4_hmc_measure argument for argument, with (coef, K, rung) in place of (w0, w2, w4), and
 * measure_out may be NULL (then the kernel compiled without the measure code runs, under nf_phi4_hmc's work cap; with
 * measure_out, nf_phi4_hmc_measure's).  The same kernel template with one more compile-time flag: the workgroup of chain c
 * reads rung[c], clamps it into 0 .. K - 1 (a corrupt entry reads inside the table), loads that row of coef once into
 * scalar registers before the trajectory loop and from there on runs nf_phi4_hmc's code: a chain on rung k gets, bit for
 * bit, what nf_phi4_hmc gives it with rung k's coefficients at the same (seed, offset).
 * The time series are written RUNG-ORDERED: dh_out, accept_out, record and measure_out of chain c go to column
 * (c / K) K + rung[c] of their step; the chain's own state stays at c: phi, pi_in, pi_out, action_out.  The Philox draws
 * stay indexed by the chain c, at nf_phi4_hmc's positions.  rung is not written.
 * nf_phi4_hmc_tiled_ladder: nf_phi4_hmc_tiled with the same replacement and the same rung-ordered dh_out, accept_out and
 * record; the same launches, workspace and plan (begin and step take the coefficients of their workgroup's chain, commit
 * writes at the rung-ordered column).
 * NF_EINVAL: what the entry point without the ladder refuses, a NULL coef or rung, K < 1, or C % K != 0.
 *
 * nf_phi4_ladder_exchange: one exchange sweep.  rows (C, row_stride) double, indexed by CHAIN: nf_lattice_measure's row of
 * the chain's current state (only its first 7 entries are read: Q = row[1], P = row[2], Lam = row[3] + .. + row[6]).  One
 * workgroup per replica set builds the map rung -> chain in LDS; for every k with k % 2 == parity and k + 1 < K, with a
 * the chain on rung k and b the chain on rung k + 1, in double
 *   Delta = (w2_k - w2_{k+1}) (Q_a - Q_b) + (w4_k - w4_{k+1}) (P_a - P_b) - (w0_k - w0_{k+1}) (Lam_a - Lam_b)
 * and the swap is accepted iff log u < Delta, u in (0, 1] the accept uniform's 53 bits from counter (lo32 i, hi32 i, lo32
 * offset, hi32 offset), i = set K + k, under the key (lo32 seed, hi32 seed ^ NF_PHILOX_EXCHANGE_DOMAIN).  One call
 * consumes one offset.  On accept rung[a] and rung[b] are swapped (no configuration moves), action[a] and action[b]
 * (action (C) double or NULL) become w2 Q + w4 P - w0 Lam under the new rungs, and swapped[set, k] = 1; swapped
 * (C / K, K - 1) uint8 gets 0 for every pair not tried or refused.  K = 1 makes no pair: nothing is written.  A rung
 * outside 0 .. K - 1 is left out of the map and its pairs are not tried.  No atomics, plain vector stores, no allocation,
 * no host synchronisation: the call can be captured into a HIP graph.
 * NF_EINVAL: NULL rows / coef / rung (or swapped with K > 1), K outside 1 .. 1024, C < 1 or C % K != 0, row_stride < 7,
 * parity outside {0, 1}. */
#define NF_PHILOX_EXCHANGE_DOMAIN 0x6e666578u   /* 'nfex' */
int nf_phi4_hmc_ladder(void *phi, double *action_out, const void *pi_in, void *pi_out, double *dh_out,
                       uint8_t *accept_out, void *record, double *measure_out, int record_every, int64_t C,
                       const int32_t *lattice, const double *coef, int K, const int32_t *rung, int n_md, double dt,
                       int n_traj, int force_accept, uint64_t seed, uint64_t offset, int dtype, void *stream);
int nf_phi4_hmc_tiled_ladder(void *phi, double *action_out, const void *pi_in, void *pi_out, double *dh_out,
                             uint8_t *accept_out, void *record, int record_every, int64_t C, const int32_t *lattice,
                             const double *coef, int K, const int32_t *rung, int n_md, double dt, int n_traj,
                             int force_accept, uint64_t seed, uint64_t offset, void *workspace, size_t workspace_bytes,
                             int dtype, void *stream);
int nf_phi4_ladder_exchange(const double *rows, int64_t row_stride, const double *coef, int K, int32_t *rung,
                            double *action, uint8_t *swapped, int64_t C, int parity, uint64_t seed, uint64_t offset,
                            void *stream);

/* ---- integration schemes of the five HMC launchers above (nf_hmc.hip, nf_hmc_tiled.hip; MI355X-side extension).  A
 * scheme is s stages (1 <= s <= NF_HMC_MAX_STAGES) of drift weights a_1 .. a_s and kick weights b_1 .. b_s; a trajectory is
 *   pi -= (b_s / 2) dt F(phi)
 *   k = 1 .. n_md, j = 1 .. s:  phi += a_j dt pi;  pi -= b_j dt F(phi)     (b_s / 2 instead of b_s when k = n_md and j = s)
 * that is n_md s force evaluations (and one more at the start).  A scheme is valid when every weight is finite, sum a =
 * sum b = 1 within 1e-12, and the sequence is symmetric within 1e-12: a_j = a_{s+1-j}, and b_j = b_{s-j} for j < s (the
 * trajectory then reads the same backwards: it is reversible, and of even order).
 * nf_hmc_scheme_check (pure host code): NF_OK, or NF_EINVAL with the broken condition in nf_last_error_string.
 * nf_hmc_scheme_named (pure host code): the library's own schemes, stated here and nowhere else:
 *   NF_HMC_LEAPFROG  s = 1: a = (1), b = (1)
 *   NF_HMC_OMELYAN2  s = 2: the second-order minimum-norm scheme of Omelyan, Mryglod and Folk (Comput. Phys. Commun. 151
 *                    (2003) 272, "2MN"), lambda = 0.1931833275037836: a = (1/2, 1/2), b = (1 - 2 lambda, 2 lambda)
 *   NF_HMC_OMF4      s = 5: their fourth-order scheme with five force evaluations per step ("OMF4" in openQCD), r1 = 0.08398315262876693, r2 = 0.2539785108410595, r3 = 0.6822365335719091,
 *                    r4 = -0.03230286765269967: a = (r2, r4, 1 - 2 (r2 + r4), r4, r2),
 *                    b = (r3, 1/2 - r1 - r3, 1/2 - r1 - r3, r3, 2 r1)
 * The _scheme form of a launcher takes its arguments and `scheme` (NULL: leapfrog), checks the scheme before anything
 * else, and runs the same kernels: the update lengths they are handed are the doubles a_j dt, b_j dt and 0.5 b_s dt formed
 * on the host and cast to dtype by the kernel, so the fused and the tiled kernels still agree bit for bit in fp64, and
 * leapfrog through a _scheme entry is the launcher without it bit for bit (which calls the same code with NULL).  Random
 * numbers: two Philox positions per trajectory whatever s.  The fused kernel keeps the lengths in its by-value
 * arguments (scalar registers and scalar loads); the tiled call issues n_md s step launches, the buffers alternating with
 * the launch, the energies of the end written by the last one; neither needs more LDS, registers per site or workspace.
 * The work caps count force evaluations: n_md s stands where n_md stands above,
 *   (n_md s n_traj + NF_HMC_MEASURE_MD_STEPS measured) max(V, 256) ceil(C / 1024) <= NF_HMC_MAX_WORK
 *   (n_md s + 2) n_traj <= NF_HMC_TILED_MAX_LAUNCHES. */
#define NF_HMC_MAX_STAGES 8
#define NF_HMC_LEAPFROG 0
#define NF_HMC_OMELYAN2 1
#define NF_HMC_OMF4 2
typedef struct nf_hmc_scheme {
  int32_t stages;
  double a[NF_HMC_MAX_STAGES];
  double b[NF_HMC_MAX_STAGES];
} nf_hmc_scheme;
int nf_hmc_scheme_check(const nf_hmc_scheme *scheme);
int nf_hmc_scheme_named(int which, nf_hmc_scheme *out);
int nf_phi4_hmc_scheme(void *phi, double *action_out, const void *pi_in, void *pi_out, double *dh_out, uint8_t *accept_out,
                       void *record, int record_every, int64_t C, const int32_t *lattice, double w0, double w2, double w4,
                       int n_md, double dt, int n_traj, int force_accept, uint64_t seed, uint64_t offset, int dtype,
                       void *stream, const nf_hmc_scheme *scheme);
int nf_phi4_hmc_measure_scheme(void *phi, double *action_out, const void *pi_in, void *pi_out, double *dh_out,
                               uint8_t *accept_out, void *record, double *measure_out, int record_every, int64_t C,
                               const int32_t *lattice, double w0, double w2, double w4, int n_md, double dt, int n_traj,
                               int force_accept, uint64_t seed, uint64_t offset, int dtype, void *stream,
                               const nf_hmc_scheme *scheme);
int nf_phi4_hmc_ladder_scheme(void *phi, double *action_out, const void *pi_in, void *pi_out, double *dh_out,
                              uint8_t *accept_out, void *record, double *measure_out, int record_every, int64_t C,
                              const int32_t *lattice, const double *coef, int K, const int32_t *rung, int n_md, double dt,
                              int n_traj, int force_accept, uint64_t seed, uint64_t offset, int dtype, void *stream,
                              const nf_hmc_scheme *scheme);
int nf_phi4_hmc_tiled_scheme(void *phi, double *action_out, const void *pi_in, void *pi_out, double *dh_out,
                             uint8_t *accept_out, void *record, int record_every, int64_t C, const int32_t *lattice,
                             double w0, double w2, double w4, int n_md, double dt, int n_traj, int force_accept,
                             uint64_t seed, uint64_t offset, void *workspace, size_t workspace_bytes, int dtype,
                             void *stream, const nf_hmc_scheme *scheme);
int nf_phi4_hmc_tiled_ladder_scheme(void *phi, double *action_out, const void *pi_in, void *pi_out, double *dh_out,
                                    uint8_t *accept_out, void *record, int record_every, int64_t C,
                                    const int32_t *lattice, const double *coef, int K, const int32_t *rung, int n_md,
                                    double dt, int n_traj, int force_accept, uint64_t seed, uint64_t offset,
                                    void *workspace, size_t workspace_bytes, int dtype, void *stream,
                                    const nf_hmc_scheme *scheme);

/* ---- Fourier-accelerated hybrid Monte Carlo (nf_hmc_fa.hip; MI355X-side extension; Batrouni et al., Phys. Rev. D 32
 * (1985) 2736).  nf_phi4_hmc's definition word for word -- the action, the force, the schemes, the Philox positions, the
 * accept rule, the outputs -- with the kinetic term pi^T A pi / 2 in place of pi^2 / 2:
 *   The per-axis table.  shat_mu(k) = 4 sin^2(pi k / L_mu) for k = 0 .. L_mu - 1, made by the host in double through
 *     sinpi: ONE table of sum_mu L_mu doubles (nf_phi4_hmc_fa_table) that every path shares.  a(k) = 1 / (w0 sum_mu
 *     shat_mu(k_mu) + M^2), M^2 = fa_mass_sq, the sum over the axes left to right, formed in double and cast to dtype;
 *     a^(-1/2)(k) = sqrt(w0 sum_mu shat_mu(k_mu) + M^2) likewise.  Nothing is added for an axis of extent 1.
 *   The operator.  A = T diag(a) T with T = H_{L_0} x .. x H_{L_3} the orthonormal separable Hartley transform,
 *     H_N[k, n] = (cos(2 pi k n / N) + sin(2 pi k n / N)) / sqrt(N) (nf_spectral_core.h; a is even in every k_mu, so
 *     T diag(a) T x = irfftn(rfftn(x) a)).  A^(-1/2) is the same with a^(-1/2).
 *   One trajectory.  eta is drawn as nf_phi4_hmc draws its momenta, at (seed, offset + 2 t).
 *     1. pi = A^(-1/2) eta                                       (pi_in, when given, replaces this step: it is pi, not eta)
 *     2. H0 = sum pi (A pi) / 2 + S(phi)
 *     3. pi -= (b_s / 2) dt F(phi)
 *     4. k = 1 .. n_md, j = 1 .. s:  phi += a_j dt (A pi);  pi -= b_j dt F(phi)      (b_s / 2 at the very end)
 *     5. H1 = sum pi (A pi) / 2 + S(phi)
 *     6. accept = force_accept || log u < -(H1 - H0), u the uniform at (seed, offset + 2 t + 1)
 *   The kinetic energy is taken from pi and A pi at both ends, never from eta: dH is a function of (phi, pi) through one
 *   operator, and a reversed trajectory reproduces it.  The energies are summed in double in a fixed order, no atomics.
 *   pi_out is pi (of the proposal, accepted or not).  A rejected chain keeps its phi bit for bit.  Two Philox positions
 *   per trajectory, as before.  Cost: n_md s + 3 filters per trajectory (refresh, H0, one per drift, H1); a filter is two
 *   transforms and one multiply.
 * nf_phi4_hmc_fa: nf_phi4_hmc_scheme's arguments (scheme NULL: leapfrog) and fa_mass_sq.  One workgroup per chain runs all
 * n_traj trajectories in ONE launch with nf_phi4_hmc's lane map; pi in registers, phi in LDS (the image that the force
 * reads is the state), one transform buffer of V elements and the Hartley matrices (built once per launch; equal extents
 * share one): dynamic LDS = 2 V sizeof(dtype) + matrices.  The table travels in the kernel's argument segment.  No
 * allocation, no host synchronisation, capturable into a HIP graph, bitwise reproducible; n_traj trajectories in one
 * launch equal n_traj launches of one; record / record_every as in nf_phi4_hmc.  There is no measuring form: record the
 * rows and measure them with nf_lattice_measure.
 * nf_phi4_hmc_fa_supported (pure host code, the launcher's planner): 1 iff dtype is NF_F32 / NF_F64, every extent is at
 * most 64, V sizeof(dtype) <= 65536 and 2 V sizeof(dtype) + matrices <= 163840 (16^2, 64^2, 16^3, 8^4 in both, 24^3 in
 * fp32; not 128^2) -- and V >= 8 (the reduction slots lie in the transform buffer) -- else 0 with the reason in
 * nf_last_error_string.
 * nf_phi4_hmc_fa_plan (pure host code): lanes and sites per lane, where phi and pi live (phi_in_lds, pi_in_lds: 1 = LDS,
 * 0 = registers), lds_bytes, matrix_bytes and filters = n_md stages + 3; NF_EINVAL where _supported answers 0.
 * nf_phi4_hmc_fa_table (pure host code): out[sum_mu lattice[mu]] = shat of the four extents one behind the other.
 * NF_EINVAL, with the reason in the message: what nf_phi4_hmc_scheme refuses, fa_mass_sq <= 0 or not finite, w0 < 0, an
 * unsupported lattice, or
 *   (n_md s + NF_HMC_FA_MD_STEPS (n_md s + 3)) n_traj max(V, 256) ceil(C / 1024) > NF_HMC_MAX_WORK:
 * a filter counts as NF_HMC_FA_MD_STEPS MD steps.  MEASURED on an MI355X (tools/hmc_fa_bench.py, the bare launch, leapfrog,
 * n_md = 10, 20 trajectories, medians of 7 alternating timings): one accelerated force evaluation in MD steps of nf_phi4_hmc
 * is 6.20 at 16^2 x 512 fp32, 6.30 in fp64, 6.25 at 16^3 x 1024 fp32, 6.57 in fp64; the largest, rounded up to a power of
 * two, is 8.  (Counting LDS passes in the code had given the same: an MD step is 2 d + 2 accesses per site and 2 barriers,
 * a filter 3 + 2 d (2 + ceil(L / 16)) accesses per site and 2 d + 2 barriers.) */
#define NF_HMC_FA_MD_STEPS 8
typedef struct nf_hmc_fa_plan {
  int32_t sites_per_lane;
  int32_t lanes;
  int32_t phi_in_lds;
  int32_t pi_in_lds;
  int64_t lds_bytes;
  int64_t matrix_bytes;
  int64_t filters;
} nf_hmc_fa_plan;
int nf_phi4_hmc_fa_supported(const int32_t *lattice, int dtype);
int nf_phi4_hmc_fa_plan(const int32_t *lattice, int dtype, int n_md, int stages, nf_hmc_fa_plan *out);
int nf_phi4_hmc_fa_table(const int32_t *lattice, double *out);
int nf_phi4_hmc_fa(void *phi, double *action_out, const void *pi_in, void *pi_out, double *dh_out, uint8_t *accept_out,
                   void *record, int record_every, int64_t C, const int32_t *lattice, double w0, double w2, double w4,
                   int n_md, double dt, int n_traj, int force_accept, uint64_t seed, uint64_t offset, int dtype,
                   void *stream, const nf_hmc_scheme *scheme, double fa_mass_sq);

/* ---- the same with the chains in HBM and many workgroups per chain (nf_hmc_fa_tiled.hip): the accelerated trajectory
 * above, word for word -- the table, a(k) and a^(-1/2)(k) formed in double and cast, eta at (seed, offset + 2 t) as
 * nf_normal_sample draws it and u at + 1 as nf_block_accept, H from pi and A pi at both ends, pi_in / pi_out are pi, the
 * accept rule, a rejected chain not written at all -- for the lattices beyond nf_phi4_hmc_fa's LDS (32^3, 16^4, 32^4, 48^4,
 * 64^3).  The energies follow nf_phi4_hmc_tiled: per-workgroup partials in double, added in a fixed order, no atomics.
 *   The filter x <- T diag(d) T x runs over HBM.  The axes of lattice[4] are cut into g >= 1 groups of adjacent axes.  One
 *     pass of a group loads panels into LDS -- the full extents of the group's axes times a run of the remaining sites,
 *     contiguous along the sites behind the group (or, where the run takes all of those, a run of the index in front of
 *     it: the panel is then one contiguous stretch) --, transforms them along the group's axes with the axis pass of
 *     nf_spectral_core.h and writes them back.  A filter is 2 g - 1 passes: the groups from the fastest to the slowest,
 *     diag(d) inside the slowest group's pass between its forward and its backward transform, the other groups back.  The
 *     single axes are transformed in the order 3, 2, 1, 0 forward and 0, 1, 2, 3 back whatever the cut, and a line's
 *     arithmetic depends on the line and its matrix alone: phi and pi out of a trajectory do not depend on the cut, bit for
 *     bit (the energies' partials are the step kernel's, so dH does not either).
 *   Drift and kick: phi' = phi + a_j dt v and pi' = pi - b_j dt F(phi') with v = A pi read from its own buffer -- the step of
 *     nf_phi4_hmc_tiled (the same kernel template, tile plan, ring of four planes, halo rule and wide accesses) with the
 *     velocity as a separate operand.
 *   A trajectory is a fixed line of launches on `stream`: draw; the refresh filter (both skipped with pi_in); the H0 filter;
 *     begin (the partials of sum pi (A pi) / 2 and S(phi), the first kick); per stage a filter and a step; the H1 filter;
 *     the partials of the end; commit (decision, copy of the accepted chains, record row, pi_out) -- `launches` =
 *     (n_md s + 3) (2 g - 1) + n_md s + 4 per trajectory, `filters` = n_md s + 3.  No allocation, no host synchronisation,
 *     capturable into a HIP graph, bitwise reproducible; the plan does not depend on C, so a chain's result does not depend
 *     on the chains it shares a call with; n_traj trajectories in one call equal n_traj calls of one; record /
 *     record_every as in nf_phi4_hmc_tiled.  There is no measuring form and no ladder form.
 * cut: -1 (the planner's choice) or a mask; bit mu (0 .. 2) set = a group boundary between axis mu and mu + 1 of
 * lattice[4].  A mask that puts a boundary next to an axis of extent 1 is refused, and so is one with a group whose one
 * line of sites and Hartley matrices exceed the 163840 B of LDS.  The planner sizes a panel for about 32 KiB, a run of 64
 * bytes at least and at most 80 KiB of LDS per pass where the group allows (else up to 163840 B), and chooses for -1: the
 * cuts whose every run reaches 64 bytes inside 80 KiB first, then the fewest groups, then the longest shortest contiguous
 * stretch, then the smallest mask.  Cut 0 (one group, the whole chain in one panel) is legal where it fits.
 * nf_phi4_hmc_fa_tiled_supported (pure host code): 1 iff dtype is NF_F32 / NF_F64, every extent is in 1 .. 64 (128^2 and
 * 130^2 stay refused: the message names the axis), V < 2^31 and some cut fits -- every lattice nf_phi4_hmc_fa takes
 * included -- else 0 with the reason in nf_last_error_string.
 * nf_phi4_hmc_fa_tiled_plan (pure host code), for n_md steps of a scheme of `stages` stages: the cut used, `groups` = g,
 * `passes` = 2 g - 1 per filter; per group i (the slowest first; entries from g on are 0) its axes first[i] .. last[i],
 * run[i] remaining sites per panel (run_inner[i] of them along the sites behind the group), panels[i] per chain,
 * panel_sites[i], lanes[i] of a workgroup, lds_bytes[i] (<= 163840) of which matrix_bytes[i] hold the matrices;
 * `filters`, `launches` (per trajectory, as above) and `step`, the step kernel's tile plan (nf_phi4_hmc_tiled_plan's).
 * nf_phi4_hmc_fa_tiled_workspace (pure host code): round256(C tiles 4 sizeof(double)) + 5 round256(C V sizeof(dtype)) bytes
 * -- the partials and five fields (two phi, two pi, v), round256 rounding up to a multiple of 256 and tiles = step.tiles
 * --, 0 for an unsupported case; it does not depend on the cut.  The caller owns the workspace; alignment as for
 * nf_phi4_hmc_tiled (8 bytes; 16 for the wide accesses); it need not be initialised.
 * nf_phi4_hmc_fa_tiled: nf_phi4_hmc_tiled_scheme's arguments (scheme NULL: leapfrog), fa_mass_sq and cut.
 * NF_EINVAL, with the reason in the message: what nf_phi4_hmc_fa and nf_phi4_hmc_tiled refuse for the arguments they share
 * (without nf_phi4_hmc_fa's work cap and lattice limits), a bad cut, or launches x n_traj > NF_HMC_TILED_MAX_LAUNCHES. */
typedef struct nf_hmc_fa_tiled_plan {
  int32_t cut;
  int32_t groups;
  int32_t passes;
  int32_t reserved;
  int32_t first[4];
  int32_t last[4];
  int32_t run[4];
  int32_t run_inner[4];
  int32_t panels[4];
  int32_t lanes[4];
  int64_t panel_sites[4];
  int64_t lds_bytes[4];
  int64_t matrix_bytes[4];
  int64_t filters;
  int64_t launches;
  nf_hmc_tiled_plan step;
} nf_hmc_fa_tiled_plan;
int nf_phi4_hmc_fa_tiled_supported(const int32_t *lattice, int dtype);
int nf_phi4_hmc_fa_tiled_plan(const int32_t *lattice, int dtype, int cut, int n_md, int stages, nf_hmc_fa_tiled_plan *out);
size_t nf_phi4_hmc_fa_tiled_workspace(int64_t C, const int32_t *lattice, int dtype);
int nf_phi4_hmc_fa_tiled(void *phi, double *action_out, const void *pi_in, void *pi_out, double *dh_out,
                         uint8_t *accept_out, void *record, int record_every, int64_t C, const int32_t *lattice, double w0,
                         double w2, double w4, int n_md, double dt, int n_traj, int force_accept, uint64_t seed,
                         uint64_t offset, void *workspace, size_t workspace_bytes, int dtype, void *stream,
                         const nf_hmc_scheme *scheme, double fa_mass_sq, int cut);

/* ---- cluster updates of phi^4 chains (nf_cluster.hip; MI355X-side extension): one Swendsen-Wang sweep of the embedded
 * Ising signs (Brower-Tamayo: phi = s |phi|).  A sweep is never rejected, leaves sum phi^2 and sum phi^4 alone and
 * flips every cluster half of the time.  The sweep, stated once:
 * There are C chains on lattice[4], with leading extents 1 for d < 4.  x is the row-major site index in 0 .. V - 1.
 * y = x + mu is the periodic forward neighbour along axis mu.
 * 1. Links.  Every pair (x, mu) with lattice[mu] > 1 is a link.
 *    - An axis of extent 1 has none.  Its self-term -w0 phi^2 is even in phi.
 *    - On an axis of extent 2 the pairs (x, mu) and (y, mu) are two links between the same two sites.  This matches the
 *      action, which counts that neighbour twice.
 * 2. Bonds.  Compute t = (w0 phi(x)) phi(y), in double on values cast to double, left to right.
 *    - The link is active iff t > 0 && u < -expm1(-2.0 * t).
 *    - A NaN or a zero makes no bond.  Either sign of w0 is legal.
 *    - The uniform is u = (r[mu] + 0.5) 2^-32, from word mu of ONE Philox4x32-10 call per site.
 *    - The counter is (lo32 i, hi32 i, lo32 offset, hi32 offset), with i = c V + x.
 *    - The key is (lo32 seed, hi32 seed ^ NF_PHILOX_CLUSTER_DOMAIN), where NF_PHILOX_CLUSTER_DOMAIN = 0x6e66636cu ('nfcl').
 * 3. Clusters.  These are the connected components of the active links.  label(x) is the smallest site index of x's
 *    component.
 * 4. Flips.  The cluster with label rho of chain c flips iff r[0] >> 31 of the Philox call with i = c V + rho at position
 *    offset + 1, under the same key.
 *    - A flipped site becomes -phi, a sign-bit flip.
 *    - Every other site keeps its bits.
 * 5. One sweep consumes 2 offsets.
 * The labels are a unique fixed point, so a sweep is a pure function of (phi, w0, seed, offset): the kernel's schedule
 * cannot show in its result.
 *
 * nf_phi4_cluster: the sweep of C chains phi (C, V), in place, one workgroup per chain with the labels (int32) and one
 * byte of bond bits per site in LDS (lds_bytes of the plan, about 5 V), for the lattices nf_phi4_hmc_supported takes
 * (V sizeof <= 64 KiB; NF_F32 and NF_F64).  phi is read once for the bonds; only the flipped sites are written back, with
 * plain vector stores.  Labelling is min-label propagation over the active links (integer minimum on LDS) with pointer
 * jumping, round after round until a round changes nothing, AT MOST V ROUNDS (a label travels at least one link per
 * round); every barrier is in uniform control flow and the exit test is a workgroup-wide flag every lane reads.
 *   stats       (C, 4) int32: clusters, sites flipped, size of the largest cluster, rounds used.  A chain that hits the
 *               bound is left untouched with (0, 0, 0, -1): it cannot happen, the bound keeps a bug from being a hang.
 *   labels_out  (C, V) int32 or NULL
 * C is 1 .. 65535.  No allocation, no host synchronisation: the call can be captured into a HIP graph.
 * NF_EINVAL: NULL phi / stats / lattice, an unsupported lattice or dtype, C out of range.
 * nf_phi4_cluster_plan / nf_phi4_cluster_supported: pure host; the lane map is nf_phi4_hmc's.
 *
 * nf_phi4_cluster_ladder / nf_phi4_cluster_tiled_ladder: the two sweeps on a coupling ladder, argument for argument with
 * (coef (K, 3) double, K, rung (C) int32, clamped into 0 .. K - 1) of nf_phi4_hmc_ladder in place of w0: a chain on rung
 * k gets nf_phi4_cluster's bits at w0_k = coef[3 k].  phi and labels_out stay at c; stats is written at the RUNG-ORDERED
 * row (c / K) K + rung[c], like dh_out of the ladder HMC kernels (rows collide unless rung is a permutation of
 * 0 .. K - 1 within every set of K chains).  Planners, workspace, launches and Philox indices are the plain ones.
 * NF_EINVAL: whatever the plain entry point refuses, a NULL coef or rung, K < 1, C not a multiple of K.
 *
 * nf_phi4_cluster_draws: the draws of the sweep at (seed, offset), element-wise, for any lattice with V < 2^31 and C in
 * 1 .. 65535: u_out (C, V, 4) double = the uniforms of step 2 (all four words, whatever the extents), flip_out (C, V)
 * uint8 = the bit of step 4 for every site index taken as a label.  A sweep composed from other pieces walks the kernel's
 * stream with these. */
#define NF_PHILOX_CLUSTER_DOMAIN 0x6e66636cu   /* 'nfcl' */
typedef struct nf_cluster_plan {
  int32_t sites_per_lane, lanes;
  int64_t lds_bytes;
} nf_cluster_plan;
int nf_phi4_cluster_supported(const int32_t *lattice, int dtype);
int nf_phi4_cluster_plan(const int32_t *lattice, int dtype, nf_cluster_plan *out);
int nf_phi4_cluster(void *phi, int32_t *stats, int32_t *labels_out, int64_t C, const int32_t *lattice, double w0,
                    uint64_t seed, uint64_t offset, int dtype, void *stream);
int nf_phi4_cluster_ladder(void *phi, int32_t *stats, int32_t *labels_out, int64_t C, const int32_t *lattice,
                           const double *coef, int K, const int32_t *rung, uint64_t seed, uint64_t offset, int dtype,
                           void *stream);
int nf_phi4_cluster_draws(double *u_out, uint8_t *flip_out, int64_t C, const int32_t *lattice, uint64_t seed,
                          uint64_t offset, void *stream);

/* ---- the same sweep with the chains in HBM and many workgroups per chain (nf_cluster_tiled.hip): for lattices beyond
 * nf_phi4_cluster's class (32^3, 16^4, 32^4, 48^4, ...).  The rule, the draws and the label convention are those above,
 * word for word, and the labels are a unique fixed point: fields, labels and stats[:, 0 .. 2] are nf_phi4_cluster's bit for
 * bit where both apply, whatever the tiles.  Any lattice of extents >= 1 with V < 2^31 sites per chain, NF_F32 and NF_F64,
 * C in 1 .. 65535.
 * A chain is cut into tiles, runs of tile_sites consecutive site indices (the last may be short; a tile may be cut in the
 * middle of a row).  tile_sites = 0 is the default (16384); any value from 1 to 32704 (what the 160 KiB of LDS hold at 5
 * bytes per site) is legal, and a value above V means V.  Four launches in a line on `stream`, after one memset of the
 * workspace's flags: (1) bonds, and the labels of the links inside a tile in LDS, by nf_phi4_cluster's rounds, at most
 * tile_sites of them; (2) the links that cross tiles, by a lock-free union on the label array in HBM (chase to the roots,
 * atomic minimum of the larger root's label; at most V - 1 atomics per link and V steps per chase; no lane waits for
 * another workgroup); (3) every site's root and the clusters' sizes (integer atomics); (4) flips and stats.  The call
 * neither allocates nor synchronises and can be captured into a HIP graph.
 *   stats       (C, 4) int32: clusters, sites flipped, size of the largest cluster, and the number of tiles of a chain
 *               (>= 1; not a round count: the rounds of phase 1 depend on the lanes' schedule, and all four columns are
 *               a pure function of the inputs).  A chain that hits one of the bounds is left untouched with
 *               (0, 0, 0, -1): it cannot happen, the bounds keep a bug from being a hang.
 *   labels_out  (C, V) int32 or NULL
 *   workspace   nf_phi4_cluster_tiled_workspace bytes, 16-byte aligned, owned by the caller, need not be initialised:
 *               per chain 4 V of labels, 4 V of sizes and V of bond bytes, plus 8 bytes of flags: 9 C V + 8 C.  After the
 *               call the int32 pair of chain c at byte 8 C V + 8 c holds (a bound was hit, the most rounds phase 1 took
 *               on a tile of the chain).
 * nf_phi4_cluster_tiled_plan (pure host): tiles per chain, the tile_sites in force, the lanes of a tile's workgroup and
 * its LDS bytes (256 + 4 tile_sites + tile_sites, the two arrays rounded up to 16).  nf_phi4_cluster_tiled_supported (pure
 * host): 1 or 0 with the reason in nf_last_error_string.  nf_phi4_cluster_tiled_workspace (pure host): the bytes, 0 for
 * a case the planner refuses or C outside 1 .. 65535.
 * NF_EINVAL: NULL phi / stats / lattice, an extent < 1, 2^31 sites or more, another dtype, C out of range, tile_sites
 * outside 0 .. 32704 or so small that tiles x lanes reaches 2^32, a NULL, short or misaligned workspace. */
typedef struct nf_cluster_tiled_plan {
  int64_t tiles;
  int32_t tile_sites, lanes;
  int64_t lds_bytes;
} nf_cluster_tiled_plan;
int nf_phi4_cluster_tiled_supported(const int32_t *lattice, int dtype, int64_t tile_sites);
int nf_phi4_cluster_tiled_plan(const int32_t *lattice, int dtype, int64_t tile_sites, nf_cluster_tiled_plan *out);
size_t nf_phi4_cluster_tiled_workspace(int64_t C, const int32_t *lattice, int64_t tile_sites);
int nf_phi4_cluster_tiled(void *phi, int32_t *stats, int32_t *labels_out, int64_t C, const int32_t *lattice, double w0,
                          uint64_t seed, uint64_t offset, int dtype, int64_t tile_sites, void *workspace,
                          size_t workspace_bytes, void *stream);
int nf_phi4_cluster_tiled_ladder(void *phi, int32_t *stats, int32_t *labels_out, int64_t C, const int32_t *lattice,
                                 const double *coef, int K, const int32_t *rung, uint64_t seed, uint64_t offset, int dtype,
                                 int64_t tile_sites, void *workspace, size_t workspace_bytes, void *stream);

/* ---- cluster-improved estimators from the labels of a sweep (nf_cluster_moments.hip; MI355X-side extension).  Every
 * cluster's sign is an independent coin, so the average of an even observable over all 2^Nc sign assignments follows
 * from per-cluster sums.  The rule, stated once:
 * Inputs.  A chain phi (V) of dtype NF_F32 / NF_F64; its labels (V) int32, ANY keys in 0 .. V - 1: sites with equal keys
 * are one cluster (the sweeps give the smallest site index); lattice[4] with leading extents 1 for d < 4; x is the
 * row-major site index and x_mu its coordinate along axis mu.
 * Fixed point.  q(w) = llrint(w 2^32), round half to even, of a double w.  Integer sums make a per-cluster sum
 * independent of the order of its terms: integer atomics only, no floating-point atomic anywhere.  A site is IN RANGE iff
 * |phi(x)| < 2^min(16, 30 - ceil(log2 V)); NaN and +-inf are not.  No int64 sum can overflow under it.
 * Per-cluster sums, all int64:
 *   A_C      = sum_{x in C} q(phi(x))
 *   R_{C,mu} = sum_{x in C} q(phi(x) tw[off_mu + x_mu][0]),  I_{C,mu} likewise with [1], for every axis mu
 * phi is cast to double and multiplied ONCE: that product is the only rounding before q.  tw is the caller's table of
 * (lattice[0] + lattice[1] + lattice[2] + lattice[3], 2) doubles, off_mu = sum_{nu < mu} lattice[nu]; entry t of axis mu
 * is meant to be (cos, sin)(2 pi t / L_mu), but the kernel uses whatever numbers it is given.
 * Outputs.
 *   out         (C, 6) double: sum_C a^2, sum_C a^4 and, per axis mu = 0 .. 3, sum_C r^2 + sum_C i^2, where
 *               a = (double)A_C 2^-32 and r, i likewise from R and I.  Each of the sums over the V slots (a^2, a^4, and r^2
 *               and i^2 of every axis, separately) is taken in a fixed order: lane l of the workgroup takes the slots
 *               l, l + lanes, ... with explicit fma (acc = fma(a, a, acc); acc4 = fma(a a, a a, acc4)), then a shuffle
 *               tree per wave, then the waves in order; out[2 + mu] = (sum r^2) + (sum i^2).  A row's bits depend on the
 *               chain, its labels, the lattice and the dtype alone.  An axis of extent 1 repeats column 0.
 *   status      (C) int32: 0 for a good chain; 1 if any site is out of range or any label lies outside 0 .. V - 1.  Such a
 *               chain has its out row all NaN and its moments row all 0; no slot outside the chain's own is touched, and
 *               the label check comes before any indexed access: a bad label is a refused input, never an
 *               out-of-bounds access.
 *   moments_out (C, V) int64 or NULL: A_C at slot = label, 0 elsewhere.
 * With M_C = A_C 2^-32 and the signs averaged: <(sum phi)^2> = sum M_C^2; <(sum phi)^4> = 3 (sum M_C^2)^2 - 2 sum M_C^4;
 * <|sum_x phi e^{i p x_mu}|^2> = sum_C |M~_C(p)|^2.  All three are sign-invariant (q(-w) = -q(w)): a flipped cluster gives
 * the same bits, so they may be taken from the field before or after the flip.
 *
 * nf_cluster_moments: one workgroup per chain with nf_phi4_cluster's lane map, for the lattices nf_phi4_cluster_supported
 * takes (V sizeof <= 64 KiB).  phi and the labels are read once into registers; the int64 slots live in LDS (8 V bytes per
 * quantity) and are filled by 64-bit integer LDS adds.  The 1 + 2 d quantities (d = axes of extent > 1) go in `passes`
 * passes of `per_pass` quantities that reuse the slot arrays: as many per pass as the 160 KiB of LDS hold behind 2 KiB of
 * reduction slots.  Same-address contention (one cluster holding most of the lattice) is met in the lane: consecutive
 * sites of a lane with one label are added in a register and issue ONE atomic.  Integer sums: bit-exact either way.
 * C is 1 .. 65535.  No allocation, no host synchronisation: the call can be captured into a HIP graph.
 * NF_EINVAL: NULL phi / labels / out / status / lattice / tw, an unsupported lattice or dtype, C out of range.
 * nf_cluster_moments_plan / nf_cluster_moments_supported: pure host. */
typedef struct nf_moments_plan {
  int32_t sites_per_lane, lanes;
  int32_t quantities, passes, per_pass;
  int64_t lds_bytes;
} nf_moments_plan;
int nf_cluster_moments_supported(const int32_t *lattice, int dtype);
int nf_cluster_moments_plan(const int32_t *lattice, int dtype, nf_moments_plan *out);
int nf_cluster_moments(const void *phi, const int32_t *labels, double *out, int32_t *status, int64_t *moments_out,
                       int64_t C, const int32_t *lattice, const double *tw, int dtype, void *stream);

/* ---- the same estimators with the chains, the labels and the int64 slots in HBM (nf_cluster_moments_tiled.hip): for
 * lattices beyond nf_cluster_moments' class (32^3, 16^4, 32^4, 48^4, ...).  The "cluster-improved estimators" rule above
 * holds word for word: the fixed point q, the range test, the sums A, R, I per cluster in int64, the caller's twiddle
 * table, status, the NaN row and the zero moments row of a refused chain, moments_out.  The clusters' integer sums are
 * exact whatever the grouping, so moments_out and status are nf_cluster_moments' and the composed path's bit for bit.
 * The ONE new part is the order of the sums of squares over the V slots, because one workgroup no longer sees them all:
 *   - a chain's slots are cut into BLOCKS, runs of block_sites consecutive slot indices (the last may be short);
 *   - within a block, lane l of 256 takes the slots first + l, first + l + 256, ... with the explicit fma forms above,
 *     then the shuffle tree per wave, then the 4 waves in order: the block's partial;
 *   - a last kernel adds the blocks' partials with one wave per (chain, column): lane l takes the blocks l, l + 64, ... in
 *     order, then the shuffle tree (nf_lattice_measure_tiled's rule for its bricks);
 *   - out[2 + mu] = (sum r^2) + (sum i^2); an axis of extent 1 repeats column 0.
 * A row's bits depend on the chain, its labels, the lattice, the dtype and block_sites alone: not on C, not on the row's
 * place in the batch, not on per_pass, not on the schedule.
 * Any lattice of extents >= 1 with V < 2^31, NF_F32 / NF_F64, C in 1 .. 65535.  block_sites = 0 is the default (4096, 16
 * sites per lane); any value from 1 upwards is legal and a value above V means V; blocks x 256 must stay below 2^32.  The
 * 1 + 2 d quantities go in passes of per_pass quantities that reuse the slot arrays; per_pass = 0 means all in one pass.
 * Launches, in a line on `stream` after one memset of the flags: CHECK (range and label test of every site, before
 * anything is indexed by a label; a failing block sets the chain's flag, and every later kernel leaves a refused chain's
 * slots alone); per pass a memset of the pass's slot arrays, SCATTER (every site's q to the slot of its label by 64-bit
 * integer atomic adds without a return value) and SQUARES (the blocks' partials; quantity 0 also writes the moments_out
 * row, zeros for a refused chain); FINISH (the partials in block order, the row or NaNs, status): 2 + 2 passes kernels.
 * No floating-point atomic, no allocation, no host synchronisation: the call can be captured into a HIP graph.
 * Same-address contention is met on chip (nf_cluster_table.h): a lane adds up its consecutive sites that share a label,
 * then claims the label's entry of a direct-mapped table in LDS, H = 512 entries of an int32 key (-1: free) and one int64
 * sum per quantity of the pass, entry h = label & (H - 1), by a compare-and-swap of the key; a lane that finds the entry
 * its label's adds there (LDS integer adds), a lane that finds another label's sends its run straight to HBM; after a
 * barrier every claimed entry sends ONE global add per non-zero sum.  Labels k, k + H, k + 2 H share an entry.  Hit, miss
 * and flush order cannot change a bit.
 *   workspace   nf_cluster_moments_tiled_workspace bytes, 16-byte aligned, owned by the caller, need not be initialised:
 *               4 C bytes of flags rounded up to 16, per_pass C V 8 bytes of slots, C blocks 10 doubles of partials.
 * nf_cluster_moments_tiled_plan (pure host): blocks per chain, the block_sites in force, quantities, per_pass (in force),
 * passes, table entries (H), kernel launches, and the LDS bytes of the scatter kernel.  _supported (pure host): 1 or 0
 * with the reason in nf_last_error_string.  _workspace (pure host): the bytes, 0 for a case the planner refuses or C
 * outside 1 .. 65535.
 * NF_EINVAL: whatever nf_cluster_moments refuses other than the lattice's class, 2^31 sites or more, block_sites < 0 or so
 * small that blocks x 256 reaches 2^32, per_pass outside 0 .. quantities, a NULL, short or misaligned workspace. */
typedef struct nf_moments_tiled_plan {
  int64_t blocks;
  int32_t block_sites, quantities, per_pass, passes, table_entries, launches;
  int64_t lds_bytes;
} nf_moments_tiled_plan;
int nf_cluster_moments_tiled_supported(const int32_t *lattice, int dtype, int64_t block_sites);
int nf_cluster_moments_tiled_plan(const int32_t *lattice, int dtype, int64_t block_sites, int per_pass,
                                  nf_moments_tiled_plan *out);
size_t nf_cluster_moments_tiled_workspace(int64_t C, const int32_t *lattice, int64_t block_sites, int per_pass);
int nf_cluster_moments_tiled(const void *phi, const int32_t *labels, double *out, int32_t *status, int64_t *moments_out,
                             int64_t C, const int32_t *lattice, const double *tw, int dtype, int64_t block_sites,
                             int per_pass, void *workspace, size_t workspace_bytes, void *stream);

/* ---- cluster spectrum (nf_cluster_spectrum.hip; MI355X-side extension): the "cluster-improved estimators" above at every
 * on-axis momentum, the input of the improved propagator and time-slice correlator.  It extends that rule and changes
 * nothing of it: the fixed point q, the range test, the refusal (status 1, a NaN row), the int64 sums, the caller's table
 * tw and the order of a sum of squares over the V slots (lane l takes the slots l, l + lanes, ... with explicit fma, then
 * the wave shuffle tree, then the waves in order) hold word for word.  What is new:
 * Momenta.  kmax >= 0 is the caller's.  K_mu = 0 for an axis of extent 1; otherwise K_mu = floor(L_mu / 2) if kmax = 0
 * ("all"), else min(kmax, floor(L_mu / 2)).
 * Per-cluster sums, all int64, for every axis mu in order and every k = 1 .. K_mu:
 *   R_{C,mu,k} = sum_{x in C} q(phi(x) tw[off_mu + (k x_mu mod L_mu)][0]),  I_{C,mu,k} likewise with [1],
 * and A_C as above.  The table is the one of nf_cluster_moments: no new table, every path gets the same twiddles bit for
 * bit, and k = 1 is that rule's quantity.  At the Nyquist momentum (2 k = L_mu) I is LEFT OUT: the table's sine there is
 * at most 1.3e-16 in magnitude, q of it times any in-range phi is 0, and the column has the same bits as with it.
 * The quantities, in order: A, then per axis in order and per k ascending R, I (R alone at Nyquist):
 *   Q = 1 + sum_mu (2 K_mu - [2 K_mu = L_mu]).
 * Outputs.
 *   out     (C, 2 + sum_mu K_mu) double: sum_C a^2, sum_C a^4, then per axis in order and per k ascending
 *           (sum_C r^2) + (sum_C i^2), at Nyquist sum_C r^2 alone; NO column for an axis of extent 1.  Every sum of
 *           squares is taken in the order above, so columns 0 and 1 and every k = 1 column are nf_cluster_moments' bits.
 *           A row's bits depend on the chain, its labels, the lattice, the dtype and kmax alone.
 *   status  (C) int32, as above; a refused chain's out row is all NaN.
 * With the signs averaged, P_mu(k) = sum_C |sum_{x in C} phi(x) e^{2 pi i k x_mu / L_mu}|^2 is the column of (mu, k),
 * P_mu(0) = column 0 and P_mu(L - k) = P_mu(k); sum_s <S_mu(s) S_mu(s + t)> = (1 / L_mu) sum_k P_mu(k) cos(2 pi k t / L_mu).
 *
 * nf_cluster_spectrum: the lattices and the structure of nf_cluster_moments (one workgroup per chain, nf_phi4_cluster's
 * lane map, phi and labels read once into registers, the checks before any indexed access, int64 slot arrays in dynamic
 * LDS filled by 64-bit integer LDS adds, a lane's run of same-label sites as ONE atomic, passes that reuse the arrays).
 * A quantity's axis, k and component follow inside the kernel from wave-uniform integer arithmetic on its index and four
 * per-axis prefix counts: nothing in registers is indexed dynamically.  The reduction region is 4 KiB whatever Q: a
 * pass's wave sums are added in wave order at the end of the pass and its columns written then; a sum r^2 whose sum i^2
 * falls into the next pass is carried.  per_pass = min(Q, 16, (160 KiB - 4 KiB) / 8 V), passes = ceil(Q / per_pass),
 * lds_bytes = 4096 + per_pass 8 V.  C is 1 .. 65535.  No allocation, no host synchronisation: graph-capturable.
 * NF_EINVAL: whatever nf_cluster_moments refuses, and kmax < 0.
 * nf_cluster_spectrum_plan / _supported: pure host; plan.kmax[mu] = K_mu of the padded axes, columns = 2 + sum K_mu. */
typedef struct nf_spectrum_plan {
  int32_t sites_per_lane, lanes, kmax[4], columns, quantities, passes, per_pass;
  int64_t lds_bytes;
} nf_spectrum_plan;
int nf_cluster_spectrum_supported(const int32_t *lattice, int dtype, int kmax);
int nf_cluster_spectrum_plan(const int32_t *lattice, int dtype, int kmax, nf_spectrum_plan *out);
int nf_cluster_spectrum(const void *phi, const int32_t *labels, double *out, int32_t *status, int64_t C,
                        const int32_t *lattice, int kmax, const double *tw, int dtype, void *stream);

/* ---- cluster modes (nf_cluster_modes.hip; MI355X-side extension): the "cluster-improved estimators" above at a LIST of
 * momentum vectors, on or off the axes: the input of the improved propagator at general momenta and of the time-slice
 * correlator at non-zero spatial momentum.  It extends that rule and changes nothing of it: the fixed point
 * q(w) = llrint(w 2^32), the range test, the refusal (status 1, a NaN row, the label check before any indexed access), the
 * int64 per-cluster sums by integer atomics only, phi cast to double and multiplied ONCE, and the order of a sum of
 * squares over the V slots (lane l takes the slots l, l + lanes, ... with explicit fma, then the wave shuffle tree, then
 * the waves in order) hold word for word.  What is new:
 * Momenta.  A list of P >= 1 integer vectors n = (n_0 .. n_3), padded like the lattice, P <= 512.  The component of an
 * axis of extent 1 must be 0.  Each component is reduced to 0 .. L_mu - 1, so negative components are legal.
 * One table.  N = the lcm of the extents > 1; N = 1 (every extent is 1) is refused, and so is N > 65536.  twN is the
 * caller's (N, 2) doubles; entry j is meant to be (cos, sin)(2 pi j / N), made on the host as math.cos(2.0 * math.pi * j /
 * N): the formula of the table `tw` above for an axis of extent N.  The kernel uses whatever numbers it is given.
 * Phase of a site.  j(x) = (sum_mu m_mu x_mu) mod N with m_mu = (n_mu mod L_mu) (N / L_mu), made on the host.  On the
 * kernel's lattices m_mu < 2^16 and x_mu < 2^14, so the sum is below 2^32: unsigned 32-bit arithmetic cannot overflow.
 * Per-cluster sums, all int64:
 *   R_{C,n} = sum_{x in C} q(phi(x) twN[j(x)][0]),  I_{C,n} likewise with [1],  and A_C as above.
 * Self-conjugate momenta.  A momentum with 2 n_mu = 0 (mod L_mu) on every axis -- the zero momentum and the Nyquist
 * corners -- has its I LEFT OUT, as at the on-axis Nyquist point: the sine there is 0 or about 1e-16, q of it times any
 * in-range phi is 0, and the column has the same bits as with it.
 * The quantities, in order: A, then per momentum in list order R, I (R alone for a self-conjugate momentum):
 *   Q = 1 + sum_n (2 - [n self-conjugate]).
 * Outputs.
 *   out     (C, 2 + P) double: sum_C a^2, sum_C a^4, then per momentum (sum_C r^2) + (sum_C i^2), formed after both sums
 *           are complete (sum_C r^2 alone for a self-conjugate momentum).
 *   status  (C) int32, as above; a refused chain's out row is all NaN.
 * A row's bits depend on the chain, its labels, the lattice, the dtype and -- column by column -- the momentum of the
 * column alone: not on C, not on the row's place in the batch, not on the other entries of the list or their order, not
 * on the pass layout.  Consequences:
 *   1. columns 0 and 1 are nf_cluster_moments' bits;
 *   2. the zero momentum's column is column 0's bits: the table's entry 0 is exactly (1, 0);
 *   3. for a momentum on axis mu alone, n = k e_mu, with N / L_mu a power of two, the column is nf_cluster_spectrum's
 *      column (mu, k) bit for bit: entry j (N / L_mu) of the N-table then equals entry j of the L_mu-table (every lattice
 *      of equal extents is such a case; (16, 16), (1, 2, 16), (24, 24, 24), (64, 128), (24, 48) were checked).  For other
 *      ratios the entries may differ in the last bit ((5, 7, 3): 3 entries of the axis of 7; (48, 32): 11 of the axis of
 *      32) and the columns agree within the rounding bound of the sums only;
 *   4. the values are invariant under cluster flips bit for bit (q(-w) = -q(w)).
 * With the signs averaged the column of n is sum_C |sum_{x in C} phi(x) e^{i p x}|^2, p_mu = 2 pi n_mu / L_mu; with ONE
 * cluster (all labels equal) it is the plain |phi~(p)|^2 in the same fixed point.
 *
 * The quantity table.  desc is (Q, 8) int32, one row per quantity (nf_cluster_modes_core.h): m_0 .. m_3, the component
 * (0 = R, 1 = I), the column, 1 for an R without an I, and the momentum's place in the list; row 0, the quantity A, is
 * zero but for its last field, the row length 2 + P.  nf_cluster_modes_describe (pure host) makes it from the list, with
 * Q and N; nf_cluster_modes_check (pure host) holds a HOST copy to the rule: NF_OK iff it is what _describe gives for some
 * list of momenta.  The launcher itself takes desc and twN as DEVICE pointers owned by the caller and cannot read them
 * without a synchronising copy, which a graph-capturable call may not make; so it checks Q, N and the lattice on the
 * host, and the kernel holds every row to the part of the rule that guards memory (m_mu in 0 .. N - 1, the component in
 * {0, 1}, the column in 2 .. 1 + P, an I right after its R) before it uses a field: with a table that fails, every chain
 * gets status 1, out is left alone (the row length is the table's own word) and nothing is indexed.
 *
 * nf_cluster_modes: the lattices and the structure of nf_cluster_spectrum (one workgroup per chain, nf_phi4_cluster's
 * lane map, phi and labels read once into registers, the checks before any indexed access, int64 slot arrays in dynamic
 * LDS filled by 64-bit integer LDS adds, a lane's run of same-label sites as ONE atomic, passes that reuse the arrays, a
 * 4 KiB reduction region, the carry of a sum r^2 whose sum i^2 falls into the next pass).  A quantity's row of desc is
 * read with wave-uniform loads; a site's coordinates are taken once.  per_pass = min(Q, 16, (160 KiB - 4 KiB) / 8 V),
 * passes = ceil(Q / per_pass), lds_bytes = 4096 + per_pass 8 V.  C is 1 .. 65535.  No allocation, no host
 * synchronisation: graph-capturable.
 * NF_EINVAL, all before any launch: whatever nf_cluster_moments refuses; NULL desc or twN; Q outside 2 .. 1025; N = 1,
 * N > 65536 or N not the lattice's lcm.  _describe, _plan and _supported also refuse NULL modes, P outside 1 .. 512 and a
 * non-zero component on an axis of extent 1; _check refuses every row that is not the rule's, with the row's number.
 * nf_cluster_modes_plan / _supported: pure host, from the host list. */
typedef struct nf_modes_plan {
  int32_t sites_per_lane, lanes, N, columns, quantities, per_pass, passes;
  int64_t lds_bytes;
} nf_modes_plan;
int nf_cluster_modes_supported(const int32_t *lattice, int dtype, const int32_t *modes, int P);
int nf_cluster_modes_plan(const int32_t *lattice, int dtype, const int32_t *modes, int P, nf_modes_plan *out);
int nf_cluster_modes_describe(const int32_t *lattice, const int32_t *modes, int P, int32_t *desc, int32_t *Q, int32_t *N);
int nf_cluster_modes_check(const int32_t *lattice, const int32_t *desc, int Q, int N);
int nf_cluster_modes(const void *phi, const int32_t *labels, double *out, int32_t *status, int64_t C,
                     const int32_t *lattice, const int32_t *desc, int Q, const double *twN, int N, int dtype, void *stream);

/* ---- the cluster spectrum with the chains, the labels and the int64 slots in HBM (nf_cluster_spectrum_tiled.hip): for
 * lattices beyond nf_cluster_spectrum's class (32^3, 16^4, 32^4, 48^4, ...).  The "cluster spectrum" rule above holds word
 * for word: the momenta K_mu from kmax; the quantities and their order (A, then per axis in order and per k ascending R,
 * I; R alone at Nyquist); Q = 1 + sum_mu (2 K_mu - [2 K_mu = L_mu]); the fixed point q, the range test, the caller's
 * twiddle table with index off_mu + (k x_mu mod L_mu); the refusal (status 1, a NaN row); the columns (C, 2 + sum_mu K_mu),
 * with no column for an axis of extent 1.
 * The ONE new part is the order of each sum of squares over the V slots, and it is nf_cluster_moments_tiled's:
 *   - a chain's slots are cut into BLOCKS, runs of block_sites consecutive slot indices (the last may be short);
 *   - within a block, lane l of 256 takes the slots first + l, first + l + 256, ... with the explicit fma forms above,
 *     then the shuffle tree per wave, then the 4 waves in order: the block's partial;
 *   - a last kernel adds the blocks' partials with one wave per (chain, sum): lane l takes the blocks l, l + 64, ... in
 *     order, then the shuffle tree;
 *   - a column is (sum r^2) + (sum i^2), formed after both sums are complete; at Nyquist sum r^2 alone.
 * Consequences:
 *   - a row's bits depend on the chain, its labels, the lattice, the dtype and block_sites alone: not on C, not on the
 *     row's place in the batch, not on per_pass, not on the workspace's former content, not on the schedule;
 *   - a column's bits do not depend on kmax: the columns at kmax = m are the corresponding columns at kmax = 0;
 *   - columns 0 and 1 and every k = 1 column are nf_cluster_moments_tiled's bits at the same block_sites, and status is
 *     its status;
 *   - where one block holds the chain and nf_cluster_spectrum runs 256 lanes (a (16, 16) lattice is such a case), the row
 *     is nf_cluster_spectrum's bit for bit.
 * Any lattice of extents >= 1 with V < 2^31, NF_F32 / NF_F64, C in 1 .. 65535.  block_sites as in
 * nf_cluster_moments_tiled: 0 is the default (4096), a value above V means V, blocks x 256 must stay below 2^32.  The Q
 * quantities go in passes of per_pass CONSECUTIVE quantities that reuse the slot arrays; per_pass = 0 means min(Q, 16) and
 * the legal values are 0 .. min(Q, 16): 16 is nf_cluster_spectrum's cap per pass and keeps a lane's run sums in registers.
 * Q <= 1024: a lattice and kmax with more quantities is refused (give a smaller kmax > 0); the cap bounds the launches and
 * the partials.
 * Launches, in a line on `stream` after one memset of the flags: CHECK (range and label test of every site, before
 * anything is indexed by a label; a failing block sets the chain's flag, and every later kernel leaves a refused chain's
 * slots alone); per pass a memset of the pass's slot arrays, SCATTER (a site is read once per pass and all quantities of
 * the pass are taken from it; x_mu is taken once per axis of the pass; a lane adds up its consecutive sites that share a
 * label and sends the run through the claim-add-flush table of nf_cluster_moments_tiled, H = 512 entries with one int64
 * sum per quantity of the pass in dynamic LDS, 512 (4 + 8 per_pass) bytes; one global 64-bit integer add without a return
 * value per claimed (label, quantity)) and SQUARES (the blocks' partials); FINISH (the partials in block order, the row or
 * NaNs, status): 2 + 2 passes kernels and 1 + passes memsets.  No floating-point atomic, no allocation, no host
 * synchronisation: the call can be captured into a HIP graph.
 *   workspace   nf_cluster_spectrum_tiled_workspace bytes, 16-byte aligned, owned by the caller, need not be initialised:
 *               4 C bytes of flags rounded up to 16, per_pass C V 8 bytes of slots, C (Q + 1) blocks doubles of partials
 *               (a^2, a^4 and one sum per further quantity).
 * nf_cluster_spectrum_tiled_plan (pure host): blocks per chain, the block_sites in force, kmax[mu] = K_mu of the padded
 * axes, columns, quantities, per_pass (in force), passes, table entries (H), kernel launches, and the LDS bytes of the
 * scatter kernel.  _supported (pure host, per_pass = 0): 1 or 0 with the reason in nf_last_error_string.  _workspace (pure
 * host): the bytes, 0 for a case the planner refuses or C outside 1 .. 65535.
 * NF_EINVAL, all checked before anything is launched: whatever nf_cluster_moments_tiled refuses, kmax < 0, per_pass
 * outside 0 .. min(Q, 16), Q > 1024. */
typedef struct nf_spectrum_tiled_plan {
  int64_t blocks;
  int32_t block_sites, kmax[4], columns, quantities, per_pass, passes, table_entries, launches;
  int64_t lds_bytes;
} nf_spectrum_tiled_plan;
int nf_cluster_spectrum_tiled_supported(const int32_t *lattice, int dtype, int kmax, int64_t block_sites);
int nf_cluster_spectrum_tiled_plan(const int32_t *lattice, int dtype, int kmax, int64_t block_sites, int per_pass,
                                   nf_spectrum_tiled_plan *out);
size_t nf_cluster_spectrum_tiled_workspace(int64_t C, const int32_t *lattice, int kmax, int64_t block_sites, int per_pass);
int nf_cluster_spectrum_tiled(const void *phi, const int32_t *labels, double *out, int32_t *status, int64_t C,
                              const int32_t *lattice, int kmax, const double *tw, int dtype, int64_t block_sites,
                              int per_pass, void *workspace, size_t workspace_bytes, void *stream);

/* ---- cluster modes with the chains, the labels and the int64 slots in HBM (nf_cluster_modes_tiled.hip): for lattices
 * beyond nf_cluster_modes' class (32^3, 16^4, 32^4, 48^4, ...).  It changes nothing of "cluster modes" above, and these
 * hold word for word: the momentum list (P <= 512, components reduced mod L_mu, 0 on axes of extent 1); the one table twN
 * of N = lcm(L_mu) entries, N <= 65536; m_mu = (n_mu mod L_mu) N / L_mu and j(x) = (sum_mu m_mu x_mu) mod N; the fixed
 * point q and the range test; the int64 sums A, R and I by integer atomics only; R alone for a self-conjugate momentum;
 * the quantity table desc (Q, 8) of nf_cluster_modes_core.h with nf_cluster_modes_describe and nf_cluster_modes_check; the
 * refusal (status 1 and a NaN row); out (C, 2 + P).  What is new, and only this:
 * Lattices.  Any lattice of extents >= 1 with V < 2^31 whose N is 2 .. 65536, NF_F32 / NF_F64, C in 1 .. 65535.
 * Phase arithmetic.  An extent may now reach 65536, so sum_mu m_mu x_mu can exceed 2^32 and "unsigned 32-bit arithmetic
 * cannot overflow" no longer holds.  The phase is formed exactly (nf_cluster_modes_tiled_core.h): each product m_mu x_mu,
 * below 2^32, is reduced mod N before the axes are added, and the sum of the four residues, below 4 N, is reduced once
 * more.  64-bit arithmetic gives the same integer.  (The reductions use no division: with M = floor(2^32 / N) from the
 * host, floor(t M / 2^32) is floor(t / N) or one less for every t < 2^32, and one conditional subtraction ends it.)
 * Order of the sums of squares.  It is nf_cluster_moments_tiled's:
 *   - a chain's slots are cut into BLOCKS, runs of block_sites consecutive slot indices (the last may be short);
 *     block_sites = 0 is the default (4096), a value above V means V, blocks x 256 must stay below 2^32;
 *   - within a block, lane l of 256 takes the slots first + l, first + l + 256, ... with the explicit fma forms above,
 *     then the shuffle tree per wave, then the 4 waves in order: the block's partial;
 *   - a last kernel adds the blocks' partials with one wave per (chain, sum): lane l takes the blocks l, l + 64, ... in
 *     order, then the shuffle tree;
 *   - a column is (sum r^2) + (sum i^2), formed after both sums are complete; sum r^2 alone for a self-conjugate momentum.
 * Passes.  The Q quantities go in passes of per_pass CONSECUTIVE quantities that reuse the slot arrays; per_pass = 0 means
 * min(Q, 16) and the legal values are 0 .. min(Q, 16).  A pass boundary may fall between the R and the I of one momentum.
 * No carry is needed: every quantity's sum is kept in the partials until FINISH.
 * Consequences:
 *   1. a column's bits depend on the chain, its labels, the lattice, the dtype, block_sites and the column's own momentum
 *      alone: not on the rest of the list or its order, not on per_pass, not on C, not on the row's place in the batch, not
 *      on the workspace's former content, not on the schedule;
 *   2. columns 0 and 1 are nf_cluster_moments_tiled's bits at the same block_sites, and status is its status;
 *   3. the zero momentum's column is column 0's bits;
 *   4. for n = k e_mu with N / L_mu a power of two, the column is nf_cluster_spectrum_tiled's column (mu, k) bit for bit
 *      at the same block_sites;
 *   5. where one block holds the chain and nf_cluster_modes runs 256 lanes (a (16, 16) lattice is such a case), the row is
 *      nf_cluster_modes' bit for bit;
 *   6. the values are invariant under cluster flips, bit for bit.
 * Launches, in a line on `stream` after one memset of the flags: CHECK (the range and label test of every site, before
 * anything is indexed by a label; it also holds every row of desc to cm_row_ok: with a failing table every chain gets
 * status 1, out is left alone and nothing is indexed by a field of the table); per pass a memset of the pass's slot
 * arrays, SCATTER (the pass's rows of desc by wave-uniform loads in front of the site loop; a site is read once per pass,
 * its coordinates are taken once, the phase once per momentum of the pass -- the R and the I of one momentum share it, a
 * pass that begins with an I forms it anew; a lane adds up its consecutive sites that share a label and sends the run
 * through the claim-add-flush table of nf_cluster_moments_tiled, H = 512 entries with one int64 sum per quantity of the
 * pass in dynamic LDS, 512 (4 + 8 per_pass) bytes) and SQUARES (the blocks' partials); FINISH (the partials in block
 * order, the row or NaNs, status): 2 + 2 passes kernels and 1 + passes memsets.  No floating-point atomic, no allocation,
 * no host synchronisation: the call can be captured into a HIP graph.
 *   workspace   nf_cluster_modes_tiled_workspace bytes, 16-byte aligned, owned by the caller, need not be initialised:
 *               4 C bytes of flags rounded up to 16, per_pass C V 8 bytes of slots, C (Q + 1) blocks doubles of partials
 *               (a^2, a^4 and one sum per further quantity).
 * desc and twN are DEVICE pointers, as in nf_cluster_modes.  nf_cluster_modes_tiled_plan (pure host, from the host list):
 * blocks per chain, the block_sites in force, N, columns (2 + P), quantities, per_pass (in force), passes, table entries
 * (H), kernel launches, and the LDS bytes of the scatter kernel.  _supported (pure host, per_pass = 0): 1 or 0 with the
 * reason in nf_last_error_string.  _workspace (pure host, from Q): the bytes, 0 for a case the planner refuses or C outside
 * 1 .. 65535.
 * NF_EINVAL, all checked on the host before anything is launched, every message with the value that was refused: a NULL
 * pointer, the dtype, an extent < 1, 2^31 sites or more, N = 1, N > 65536 or N not the lattice's lcm, Q outside 2 .. 1025,
 * C outside 1 .. 65535, block_sites < 0 or so small that blocks x 256 reaches 2^32, per_pass outside 0 .. min(Q, 16), a
 * NULL, short or misaligned workspace; _plan and _supported also refuse what nf_cluster_modes_describe refuses. */
typedef struct nf_modes_tiled_plan {
  int64_t blocks;
  int32_t block_sites, N, columns, quantities, per_pass, passes, table_entries, launches;
  int64_t lds_bytes;
} nf_modes_tiled_plan;
int nf_cluster_modes_tiled_supported(const int32_t *lattice, int dtype, const int32_t *modes, int P, int64_t block_sites);
int nf_cluster_modes_tiled_plan(const int32_t *lattice, int dtype, const int32_t *modes, int P, int64_t block_sites,
                                int per_pass, nf_modes_tiled_plan *out);
size_t nf_cluster_modes_tiled_workspace(int64_t C, const int32_t *lattice, int Q, int64_t block_sites, int per_pass);
int nf_cluster_modes_tiled(const void *phi, const int32_t *labels, double *out, int32_t *status, int64_t C,
                           const int32_t *lattice, const int32_t *desc, int Q, const double *twN, int N, int dtype,
                           int64_t block_sites, int per_pass, void *workspace, size_t workspace_bytes, void *stream);

/* ---- what the samplers' rows measure (nf_measure.hip; MI355X-side extension): every sufficient statistic of N
 * configurations in one pass.  cfgs (N, V) of dtype NF_F32 / NF_F64 on lattice[4] (leading extents 1 for d < 4);
 * out (N, n_out) DOUBLE, n_out = 7 + lattice[0] + lattice[1] + lattice[2] + lattice[3], per row
 *   out[0], out[1], out[2]   sum phi, sum phi^2, sum phi^4
 *   out[3 + mu]              sum_x phi(x) phi(x - mu), periodic; 0 for an axis of extent 1 (no neighbour is read, the
 *                            convention of nf_phi4_action); on an axis of extent 2 the plain formula (the one neighbour
 *                            once per site)
 *   out[7 + off_mu + t]      S_mu(t) = sum over the sites with x_mu = t of phi(x), off_mu = sum_{nu < mu} lattice[nu]; an
 *                            axis of extent 1 has the one entry sum phi
 * so that S = w2 out[1] + w4 out[2] - w0 sum_mu out[3 + mu] is nf_phi4_action's action.  Every site value is converted
 * to double before any arithmetic, for either dtype.  The sums have a fixed order (lane partial in site order, wave
 * shuffle tree, waves in order; per slice fixed stripes in stripe order; segments in segment order) and there are no
 * atomics: the same input gives the same bits, and a row's result depends on its values, the lattice and the dtype alone
 * -- not on N, on its position in the batch, on the other rows or on the alignment of cfgs.  A row is read from HBM
 * once (16-byte loads when the fastest extent is a multiple of 16 / sizeof(dtype) and cfgs is 16-byte aligned, one site
 * at a time otherwise) into an LDS image that every sum is read from.  The call neither allocates nor synchronises and
 * can be captured into a HIP graph.
 * nf_measure_plan (a function of lattice and dtype alone): regime NF_MEASURE_PACKED (V <= 256 sites: rows_per_group = 4
 * rows per workgroup, one wave each), NF_MEASURE_RESIDENT (V sizeof(dtype) <= 64 KiB: one workgroup per row) or
 * NF_MEASURE_SEGMENTED (beyond: the slowest axis of extent > 1 is cut into `segments` runs of seg_len planes, the last
 * may be shorter, every run a whole number of 16-byte units (seg_len x plane sites is a multiple of vec); a workgroup stages its run at once, stage_planes = seg_len, reads the one plane before it from HBM for
 * the backward link and writes its partials to the workspace, and a second kernel adds them in segment order).  lanes =
 * the lanes that share one image; vec = sites per 16-byte access (1: site by site); lds_bytes <= lds_budget.
 * nf_lattice_measure_supported (pure host code): 1 for NF_F32 / NF_F64, extents >= 1, V and n_out < 2^31 and a plane of the slowest
 * axis of extent > 1 that fits the LDS of a CU next to the reduction slots (32^4 in fp32 does, 32^4 in fp64 and 48^4 do
 * not), else 0 with the reason in nf_last_error_string.  nf_lattice_measure_workspace (pure host code): the bytes of
 * `workspace` for N rows, 0 when segments == 1 or the case is unsupported; the caller owns it (8-byte aligned, need not
 * be initialised).
 * NF_EINVAL: NULL cfgs / out / lattice, an unsupported lattice or dtype, N < 0, a short or NULL workspace where one is
 * needed, or more than 2^24 - 1 workgroups (ceil(N / rows_per_group) segments, or ceil(N n_out / 256)).  N = 0: NF_OK. */
#define NF_MEASURE_RESIDENT 0
#define NF_MEASURE_PACKED 1
#define NF_MEASURE_SEGMENTED 2
typedef struct nf_measure_plan {
  int32_t regime;
  int32_t rows_per_group;
  int32_t segments;
  int32_t seg_len;
  int32_t stage_planes;
  int32_t lanes;
  int32_t vec;
  int32_t n_out;
  int64_t lds_bytes;
  int64_t lds_budget;
} nf_measure_plan;
int nf_lattice_measure_supported(const int32_t *lattice, int dtype);
int nf_lattice_measure_plan(const int32_t *lattice, int dtype, nf_measure_plan *out);
size_t nf_lattice_measure_workspace(int64_t N, const int32_t *lattice, int dtype);
int nf_lattice_measure(const void *cfgs, double *out, int64_t N, const int32_t *lattice, void *workspace,
                       size_t workspace_bytes, int dtype, void *stream);

/* ---- the same statistics for rows that nf_lattice_measure refuses (nf_measure_tiled.hip): bricks.  cfgs, out (N, n_out),
 * the definitions of every entry, the conversion to double and the extent-1 / extent-2 rules are nf_lattice_measure's,
 * word for word.  The row is cut along its first two axes of extent > 1, axis0 and axis1 (axis1 = -1: the lattice has one
 * such axis and is cut along it alone), into bricks of e0 planes of axis0 x e1 sub-planes of axis1 x all of the axes
 * behind, one workgroup each, n0 x n1 = `bricks` per row, brick b = b0 n1 + b1 covering the planes b0 e0 .. and the
 * sub-planes b1 e1 .. (the last of an axis may be shorter).
 * nf_measure_tiled_plan (a function of lattice, dtype and brick_bytes alone, not of N): brick_bytes is the target size of
 * a brick, 0 = the default (32 KiB).  axis1 is filled first, e1 = min(L_axis1, brick_bytes / bytes of a sub-plane), and
 * axis0 is cut into pieces of more than one plane (e0 > 1) only when e1 = L_axis1; the pieces of an axis are as even as
 * they get, and along the fastest axis they are whole 16-byte units (vec sites).  A sub-plane beyond brick_bytes is still
 * taken, as one brick, while it fits the LDS of a CU next to the reduction slots; beyond that the lattice is refused
 * ("does not fit": there is no cut along a third axis).  lanes = 512 for bricks above 4096 sites, else 256; n_part = 7 + e0
 * + e1 + the uncut extents, the partial sums a brick writes; lds_bytes <= lds_budget.
 * A brick is one run of consecutive sites: it is staged into LDS once (16-byte loads when vec > 1 and cfgs is 16-byte
 * aligned, site by site otherwise: the same image) and every sum is read from the image as in nf_lattice_measure; the
 * plane before the brick and the sub-plane before it are read from HBM for the backward links.  Sum order: inside a
 * brick nf_lattice_measure's (lane partial in site order, wave shuffle tree, waves in order; per slice fixed stripes in
 * stripe order); then a second kernel adds the bricks' partials (workspace: (N, bricks, n_part) doubles), one wave of 64
 * lanes per (row, output): lane l adds the bricks l, l + 64, ... of the output's list in order, then the shuffle tree.
 * The list of a slice of axis0 is the n1 bricks that hold it in b1 order, of a slice of axis1 the n0 bricks in b0 order,
 * of everything else all bricks in brick order.  No atomics: a row's bits depend on its values, the lattice, the dtype
 * and brick_bytes alone -- not on N, its position, the other rows or the alignment of cfgs.  Two launches; the call
 * neither allocates nor synchronises and can be captured into a HIP graph.
 * nf_lattice_measure_tiled_supported / _workspace (pure host code): as for nf_lattice_measure; the workspace is needed
 * for every N >= 1 (8-byte aligned, need not be initialised).
 * NF_EINVAL: NULL cfgs / out / lattice, extents < 1, V or n_out of 2^31 or more, a dtype other than NF_F32 / NF_F64, a
 * brick_bytes below one element or above lds_budget, a brick that does not fit, N < 0, a short, NULL or misaligned
 * workspace, or more than 2^24 - 1 workgroups (N bricks, or ceil(N n_out / 4)).  N = 0: NF_OK. */
typedef struct nf_measure_tiled_plan {
  int32_t axis0;
  int32_t axis1;
  int32_t e0;
  int32_t e1;
  int32_t n0;
  int32_t n1;
  int32_t bricks;
  int32_t lanes;
  int32_t vec;
  int32_t n_out;
  int32_t n_part;
  int32_t reserved;
  int64_t lds_bytes;
  int64_t lds_budget;
} nf_measure_tiled_plan;
int nf_lattice_measure_tiled_supported(const int32_t *lattice, size_t brick_bytes, int dtype);
int nf_lattice_measure_tiled_plan(const int32_t *lattice, size_t brick_bytes, int dtype, nf_measure_tiled_plan *out);
size_t nf_lattice_measure_tiled_workspace(int64_t N, const int32_t *lattice, size_t brick_bytes, int dtype);
int nf_lattice_measure_tiled(const void *cfgs, double *out, int64_t N, const int32_t *lattice, size_t brick_bytes,
                             void *workspace, size_t workspace_bytes, int dtype, void *stream);

/* ---- VJP of the conv layer (K5)---------------------------------------------------------------
 * grad_input is nf_conv_fwd itself applied to the pre-activation cotangent with the weights
 * flipped along every kernel axis and in/out channels swapped.  The two entry points below are
 * the rest of what autograd derives for ConvAct in Fitter.step (src/_normflowcore.py:288):
 *   nf_act_vjp     grad_pre = grad_out * act'(.), the derivative written through the activation's
 *                  OUTPUT y (tanh: 1-y^2, relu/leaky: sign test, softplus: 1-e^-y, sigmoid: y(1-y));
 *   nf_conv_wgrad  gw[o][t*cin + i] += sum_{b,n} gz[b,o,n] * in[b,i,(n + t - k//2) mod L] and
 *                  gw[o][ntaps*cin] += sum_{b,n} gz[b,o,n] (the bias gradient), accumulated with
 *                  float atomics into a ZEROED (16*ceil(cout/16), nf_conv_wgrad_cols(cin, ntaps))
 *                  buffer; cout <= 48 per call; gz is the full-lattice (B, cout, V) cotangent.
 */
int nf_act_vjp(const void *grad_out, const void *y, void *grad_pre, int64_t n, int act, int dtype,
               void *stream);
int nf_conv_wgrad_cols(int cin, int ntaps);
int nf_conv_wgrad(const void *in, const void *gz, void *gw, int64_t B, const int32_t *lattice,
                  const int32_t *ksize, int cin, int cout, int dtype, void *stream);

/* The same weight gradient on the fp16 matrix cores (every fp32 product as three fp16 products, fp32 accumulation;
 * gz scaled by the power of two of *absmax_bits, see nf_absmax_bits) for the lattice networks' shapes: 4-D lattice with 32 + 16 n sites on
 * the fastest axis, 3^4 kernels, cin 1 or 8, cout <= 48, fp32.  Same gw layout and accumulate-into-gw semantics as
 * nf_conv_wgrad; deterministic (per-workgroup partial matrices in the workspace, summed in a fixed order).
 * compact_parity < 0: gz is the full-lattice (B, cout, V) tensor; 0 / 1: gz is pair-compact (B, cout, V/2), the cotangent of
 * an active-site-only layer (coordinate sum == compact_parity mod 2), read as it is -- no expanded copy (same for
 * nf_planes_to_split16).
 * nf_conv_wgrad_split16_supported says whether a shape qualifies; callers fall back to nf_conv_wgrad otherwise. */
/* Input gradients of the lattice networks' conv layers on the split-fp16 chain (training).  The gradient w.r.t. the input of
 * a layer with 8 input channels is a convolution of the output cotangent gz (B, C, V) with the flipped, transposed weights:
 * nf_planes_to_split16 writes gz, scaled into fp16's range by the power of two that belongs to *absmax_bits (nf_absmax_bits;
 * NULL: unscaled, for activations), as ceil(C / 8) pair tensors (G, B, V, 16 halfs; layout of NF_OUT_SPLIT16);
 * nf_conv_dgrad_split16 runs the hidden-layer kernel on one of them with weights packed like a forward 8 -> 8 layer's
 * (flipped / transposed by the caller, zero rows past C), bias NULL, act 0, and writes -- or, with accumulate, adds --
 * the descaled fp32 planes gx (B, 8, V).  The same entry runs a FORWARD 8 -> 8 layer whose output training keeps as planes:
 * activations as an unscaled pair tensor (absmax_bits NULL), bias, act = tanh.  Lattices as nf_conv_split16_supported. */
int nf_planes_to_split16(const void *gz, void *out16, const void *absmax_bits, int64_t B, int C,
                         const int32_t *lattice, int compact_parity, void *stream);
int nf_conv_dgrad_split16(const void *in16, const void *wsplit, const void *bias, void *gx, int64_t B,
                          const int32_t *lattice, const void *absmax_bits, int accumulate, int act, void *stream);

/* The last conv layer 8 -> 46 of a spline coupling's net at the active sites on the split-fp16 kernel (the matrix-core part of
 * nf_conv_rqs), with the logits written out pair-compact (B, 46, V/2) fp32 instead of consumed: the forward pass of a
 * training step, which differentiates the spline separately.  in: fp32 channel planes (B, 8, V) (fastest axis of 32 sites)
 * or, with in_split16, the (B, V, 16) pair tensor; absmax_bits (nf_absmax_bits of the input, or NULL for inputs already in
 * fp16's range): the input gets / is scaled by the matching power of two and the logits are descaled; wsplit in
 * NF_WLAYOUT_SPLIT16; bias (46) fp32 or NULL. */
int nf_conv_last_logits_split16(const void *in, int in_split16, const void *wsplit, const void *bias, void *logits,
                                int64_t B, const int32_t *lattice, int active_parity, const void *absmax_bits,
                                void *stream);
/* ... the same for any cout <= 46 (logits (B, cout, V/2); weights still packed to 48 columns), ADDED to the logits already in
 * `logits` when accumulate != 0 (bias NULL then): the second group of 8 input channels of a 16 -> cout layer -- hidden width 16 on the split-fp16 kernels (reference: modules.py:68-154 leaves the hidden
 * widths free); normflow__amd/_hip.py, conv_wide_logits_split16 composes the stack 1 -> 16 -> 16 -> 3m-2 from
 * nf_conv_first_split16 x 2, nf_conv_dgrad_split16 x 4 (+ nf_planes_to_split16 x 2) and this entry x 2. */
int nf_conv_last_logits_split16_acc(const void *in, int in_split16, const void *wsplit, const void *bias, void *logits,
                                    int64_t B, const int32_t *lattice, int active_parity, const void *absmax_bits,
                                    int accumulate, int cout, void *stream);

/* nf_expand_pairs: a pair-compact tensor (rows, V/2) -- the layout the active-site-only conv output and its cotangent use --
 * to the full lattice (rows, V), zeros at the sites of the other parity; rows = B * channels; lattice[3] even. */
int nf_expand_pairs(const void *compact, void *full, int64_t rows, const int32_t *lattice, int parity, int dtype,
                    void *stream);
/* nf_gather_pad: out[i] = index[i] in [0, nsrc) ? src[index[i]] : 0 for i < n, elements of 2, 4 or 8 bytes moved as bits.
 * The host side re-arranges a layer's weights into a kernel's fragment layout with it (normflow__amd/_hip.py, _pack_by_gather:
 * the index map of a layer shape is built once): one launch where the torch expression of the same packing is a dozen. */
int nf_gather_pad(const void *src, const int32_t *index, void *out, int64_t n, int64_t nsrc, int elem_bytes, void *stream);
/* nf_conv_wgrad_sites: the same gradient (same gw layout and accumulate-into-gw contract as nf_conv_wgrad) for layers with
 * FEW columns -- taps x cin + 1 <= 224, i.e. every 1-, 2- and 3-D 3-tap layer of up to 8 input channels: the layers of the
 * small lattices flows are usually trained on (reference: src/_normflowcore.py:275-294 differentiating
 * src/nn/scalar/modules.py:120-145).  Every wave holds all column tiles and the waves split the sites of a box; no atomics --
 * per-workgroup partial matrices in `workspace` (nf_conv_wgrad_sites_workspace bytes) are added to gw in a fixed order, so the
 * gradient is bitwise reproducible.  compact_parity 0 / 1: gz is the pair-compact (B, cout, V/2) cotangent of an active-site-only
 * layer (values at the sites whose coordinate sum == parity mod 2; needs an even fastest axis) and only those sites are
 * walked; -1: gz is (B, cout, V).  fp32 and fp64 (fp64 with cout > 32 only up to 96 columns). */
int nf_conv_wgrad_sites_supported(const int32_t *lattice, const int32_t *ksize, int cin, int cout, int dtype);
size_t nf_conv_wgrad_sites_workspace(const int32_t *ksize, int cin, int cout, int dtype);
int nf_conv_wgrad_sites(const void *in, const void *gz, void *gw, int64_t B, const int32_t *lattice, const int32_t *ksize,
                        int cin, int cout, int compact_parity, void *workspace, size_t workspace_bytes, int dtype,
                        void *stream);
int nf_conv_wgrad_split16_supported(const int32_t *lattice, const int32_t *ksize, int cin, int cout);
size_t nf_conv_wgrad_split16_workspace(int64_t B, const int32_t *lattice, int cin);
int nf_conv_wgrad_split16(const void *in, const void *gz, void *gw, int64_t B, const int32_t *lattice,
                          const int32_t *ksize, int cin, int cout, const void *absmax_bits, int compact_parity,
                          void *workspace, size_t workspace_bytes, void *stream);
/* max |x| of an fp32 tensor of n elements, as the bits of a float in 4 bytes of device memory: what the training kernels
 * (nf_conv_wgrad_split16, nf_planes_to_split16 / nf_conv_dgrad_split16) scale a cotangent by; one pass serves both.
 * Equal to max|x| bit for bit (+0 for an empty or all-zero tensor; a NaN entry is skipped, an inf entry gives inf).
 * The kernels that read it multiply their operand by 2^(13 - e), max|x| = f 2^e with f in [0.5, 1), and the result by the
 * inverse, both carried as exponents (never as one float: 2^(13 - e) overflows below 2^-115).  For an operand whose
 * largest entry is a NORMAL fp32 number, multiplying the operand by 2^k multiplies every output by exactly 2^k wherever
 * the scaled output is a normal number or zero (tests/test_split16_range.py: k from -120, a largest entry of about
 * 2^-118, to 100); the operand's own subnormal entries count with the bits fp32 keeps of them.  Below that nothing is
 * promised but finite results: nf_conv_last_logits_split16 and the fused last layer return zeros for a maximum below
 * 2^-127 (their descale 2^(-23 + e) is one float and underflows there).  An all-zero operand gives exact zeros; a
 * non-finite maximum leaves the operand unscaled (the inf meets the products and gives non-finite outputs, a NaN entry
 * likewise in its window).  A bias is carried in the scaled accumulators as
 * bias 2^(23 - e): with a bias, |bias| / max|x| must stay below 2^100. */
int nf_absmax_bits(const void *x, int64_t n, void *bits, void *stream);
/* The power of two 2^c that brings the larger of max|a| and max|b| (fp32 tensors of na, nb elements) to [1, 2), and 2^-c:
 * work (16 bytes of device memory) = [bits of max|a|][bits of max|b|][2^c][2^-c], the last two as floats.  A zero or
 * subnormal maximum gives c = 126, an inf one c = 0; NaN entries do not count.  The fused last layer's backward pass
 * multiplies its two cotangents by 2^c and its gradients by 2^-c, so that the fp32 logit cotangent it materialises
 * keeps its bits for cotangents of any size. */
int nf_cotangent_pow2(const void *a, int64_t na, const void *b, int64_t nb, void *work, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NORMFLOW_HIP_H */

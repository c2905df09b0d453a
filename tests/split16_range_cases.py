"""Operand-range cases of the split-fp16 kernels (test infrastructure for tests/test_split16_range_host.py and
tests/test_split16_range.py).

The split-fp16 kernels (include/normflow_hip.h: NF_WLAYOUT_SPLIT16, nf_conv_first_split16, nf_conv_fwd_split16,
nf_conv_dgrad_split16, nf_conv_last_logits_split16, nf_conv_wgrad_split16, nf_small_lattice_coupling) replace every fp32
product x w by three fp16 matrix-core products with fp32 accumulation:

    x = x_hi + x_lo,  x_hi = fp16(x), x_lo = fp16(x - x_hi)           (an operand read as it is, or first multiplied by
    1024 w = w_hi + w_lo, split the same way                            the power of two of nf_absmax_bits)
    out = 2^-10 sum_k (x_hi w_hi + x_lo w_hi + x_hi w_lo)             (x_lo w_lo is dropped)

This module holds
  * the SCALES: pairs of powers of two (kx, kw) applied to a base field and base weights -- every operand size the header
    says the kernels take, from lo parts that are all normal fp16 numbers down to lo parts that are all below fp16's
    subnormal step, and the weights at the guard (`_hip.SPLIT16_WEIGHT_LIMIT`);
  * `emulate`: a numpy emulation of that arithmetic, written from the header (np.float16 splits, the three products,
    sequential fp32 accumulation over one output's K terms).  It never runs a kernel.  It sets the constant of the bound
    and -- through its four MUTATIONS, each a way a kernel could be subtly wrong -- shows which cases would notice;
  * the per-output conditioned BOUND, the pattern of tests/cond_bound.py: for output i with terms k

        B_i = C_SPLIT * ( 2^-22 S_i + 2^-25 sum_k |w_k| + 2^-35 sum_k |x_k| ),    S_i = sum_k |w_k| |x_k|

    (the two operand representations 2 x 2^-23 |x w| + the dropped lo lo product 2^-22 |x w| + accumulation, as one term;
    fp16's subnormal half-step 2^-25 on x_lo; the half-step 2^-25 on the lo part of 1024 w, i.e. 2^-35 on w).  Outputs that
    pass through tanh / logistic (1-Lipschitz) and the pair split get  B_i + 1e-5 max|ref| : the tolerance
    test_split_fp16_hidden_layer_and_chain holds these kernels to at unit scale.

Base operands.  The field of a first layer is randn, hidden activations are tanh(randn), weights 0.2 randn -- what every other
split-fp16 test draws -- with two restrictions that keep EVERY scale pair of the table inside the range the header states:
the field is clamped to +-1.95 (so that the pair (2^15, 2^-15) stays below fp16's 65504) and the weights to +-0.45 (so that the
pair (2^-14, 2^6) stays below the weight limit 29.296875).  Hidden activations carry planted exact +-1, exact 0 and 2^-20.
"""
import numpy as np
import torch

from oracle import nf_oracle as O

F16, F32, F64 = np.float16, np.float32, np.float64
W_EXP = 10                                   # the weights are packed as fp16 pairs of 2^10 w (_hip.SPLIT16_WEIGHT_SCALE)
X_CLAMP, W_CLAMP, W_STD = 1.95, 0.45, 0.2
ACT_EXTRA = 1e-5                             # x max|ref|: test_split_fp16_hidden_layer_and_chain's tolerance at unit scale

# name -> (log2 kx, log2 kw or None, max|w| to place or None)
SCALES = {
    "unit":            (0, 0, None),
    "w 2^-3":          (0, -3, None),
    "w 2^-10":         (0, -10, None),
    "w 2^-14":         (0, -14, None),
    "w 2^-20":         (0, -20, None),
    "wmax 28.0":       (0, None, 28.0),
    "wmax 29.29":      (0, None, 29.29),       # just inside _weights_fit_fp16 (29.296875)
    "x 2^-3":          (-3, 0, None),
    "x 2^-6":          (-6, 0, None),
    "x 2^-14":         (-14, 0, None),
    "x 2^-24":         (-24, 0, None),
    # compensated: pre-activations stay of order one while one operand sits at an end of its range
    "x 2^15 w 2^-15":  (15, -15, None),
    "x 2^12 w 2^-12":  (12, -12, None),
    "x 2^-14 w 2^6":   (-14, 6, None),
}

MUTATIONS = ("drop x_lo*w_hi", "drop x_hi*w_lo", "flush lo < 2^-14", "no 2^-10 descale")

# The entry points of tests/test_split16_range.py as the emulation sees them: K terms per output, which base the split
# operand x comes from, whether x is first multiplied by the power of two of its own maximum (nf_absmax_bits: then kx cannot
# matter, which the covariance tests hold exactly), which power of two the other operand carries (W_EXP for packed weights;
# "absmax" for the weight gradient, whose second operand is the scaled cotangent), and whether an activation follows.
#   weight_grad: x = the layer's input (read as it is), "w" = the cotangent gz: K = B * sites terms per weight entry.
ENTRY_POINTS = {
    "conv_first_split16":         dict(K=81,  x="field",  x_absmax=False, w_exp=W_EXP,    act=True),
    "conv_layer_split16":         dict(K=648, x="hidden", x_absmax=False, w_exp=W_EXP,    act=True),
    "conv_hidden_planes_split16": dict(K=648, x="hidden", x_absmax=True,  w_exp=W_EXP,    act=False),
    "conv_last_logits_split16":   dict(K=648, x="hidden", x_absmax=True,  w_exp=W_EXP,    act=False),
    "conv_input_grad_split16":    dict(K=648, x="cotangent", x_absmax=True, w_exp=W_EXP,  act=False),
    "conv_weight_grad":           dict(K=768, x="hidden", x_absmax=False, w_exp="absmax", act=False),
    "small_lattice_coupling":     dict(K=27,  x="field",  x_absmax=False, w_exp=W_EXP,    act=True),
}

# The constant of the bound: the smallest power of two that is at least 4 x the emulation's worst err / (B_i / C_SPLIT) over
# every entry point and scale pair of this file (the matrix cores accumulate in another order than the sequential emulation
# and are expected below it).  test_split16_range_host.py::test_constant_of_the_bound recomputes the worst value and this rule.
EMULATION_WORST = 0.944      # measured on the CPU: conv_layer_split16 at "wmax 29.29" (648 sequential fp32 additions x 3); 0.51 at unit scale
C_SPLIT = 4.0                # 4 x 0.944 = 3.78 -> 4


# K5s is held to its first layer's bound CARRIED through two more layers that pass their input on and the affine map
# (tests/test_split16_range.py, _small_bound): besides B_i + ACT_EXTRA max|h1| of the first layer that is, at most, a second
# ACT_EXTRA (|h2| <= 1), the bound of two one-term layers on |h| <= 1, and the epilogue's 2 x 2^-22.  The host test judges a
# mutation "powered" for K5s against the sum, so that it is powered against the bound the GPU test asserts.
K5S_CARRIED = ACT_EXTRA + 2 * C_SPLIT * (2.0 ** -22 + 2.0 ** -25 + 2.0 ** -35) + 2.0 ** -21

# ------------------------------------------------------------------------------------------------ base operands and scales
def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def base_field(shape, seed):
    """randn clamped to +-X_CLAMP, fp32 values as float64, shape `shape`."""
    t = torch.randn(shape, generator=_gen(seed), dtype=torch.float32, device="cpu").clamp_(-X_CLAMP, X_CLAMP)
    return t.double()


def base_hidden(shape, seed):
    """tanh(randn) with planted exact +1, -1, 0 and 2^-20 (every 37th entry, in turn), fp32 values as float64."""
    t = torch.tanh(torch.randn(shape, generator=_gen(seed), dtype=torch.float32, device="cpu"))
    flat = t.reshape(-1)
    for j, v in enumerate((1.0, -1.0, 0.0, 2.0 ** -20)):
        flat[j * 9 + 3::37 * 4] = v
    return t.double()


def base_cotangent(shape, seed):
    return torch.randn(shape, generator=_gen(seed), dtype=torch.float32, device="cpu").double()


def base_weights(shape, seed):
    """0.2 randn clamped to +-W_CLAMP, fp32 values as float64."""
    t = (W_STD * torch.randn(shape, generator=_gen(seed), dtype=torch.float32, device="cpu")).clamp_(-W_CLAMP, W_CLAMP)
    return t.double()


def scale_x(x, name):
    """The base x at the scale pair `name`: an exact power of two (float64 in, fp32-representable float64 out)."""
    return x * 2.0 ** SCALES[name][0]


def scale_w(w, name):
    """The base weights at the scale pair `name`: a power of two, or max|w| placed at the pair's value (its fp32 rounding)."""
    _, kw, wmax = SCALES[name]
    if wmax is None:
        return w * 2.0 ** kw
    top = float(np.float32(wmax))
    out = (w * (top / float(w.abs().max()))).float().double()
    out = out.clamp(-top, top)
    i = int(w.abs().reshape(-1).argmax())
    out.reshape(-1)[i] = top if w.reshape(-1)[i] > 0 else -top
    return out


# ------------------------------------------------------------------------------------------------ the bound
def bound_terms(S, sum_w, sum_x):
    """B_i / C_SPLIT from S_i = sum |w||x|, sum |w| and sum |x| over the terms of output i (arrays or tensors)."""
    return 2.0 ** -22 * S + 2.0 ** -25 * sum_w + 2.0 ** -35 * sum_x


def conv_bound(x, w):
    """B_i of every output of the circular convolution of x (B, cin, *L) with w (cout, cin, *k), float64 tensors:
    (B, cout, *L).  S_i is the convolution of |x| with |w|; sum|w| belongs to the output channel, sum|x| to the window."""
    ax, aw = x.abs(), w.abs()
    S = O.circular_conv_fast(ax, aw)
    sum_w = aw.reshape(aw.shape[0], -1).sum(1).reshape((1, -1) + (1,) * (x.dim() - 2))
    sum_x = O.circular_conv_fast(ax, torch.ones_like(aw[:1]))
    return C_SPLIT * bound_terms(S, sum_w, sum_x)


# ------------------------------------------------------------------------------------------------ the emulation
def _absmax_exp(a):
    """The exponent the kernels scale an operand by (nf_absmax_bits + pow2_exp_for): 13 - e, max|a| = f 2^e, f in [0.5, 1)."""
    mx = float(np.abs(a).max())
    if not (mx > 0.0) or not np.isfinite(mx):
        return 0
    return 13 - int(np.frexp(np.float32(mx))[1])


def _split(a32, flush):
    """fp32 rows -> (hi, lo) halfs as fp32; rows with `flush` set lose the lo parts below fp16's smallest normal number."""
    hi = a32.astype(F16)
    lo = (a32 - hi.astype(F32)).astype(F16).astype(F32)
    lo = np.where(flush[:, None] & (np.abs(lo) < F32(2.0 ** -14)), F32(0), lo)
    return hi.astype(F32), lo


def _emulate_rows(x, w, ex, ew, mut):
    """Rows of K terms, each with its own operand exponents (ex, ew: int arrays) and mutation (index into MUTATIONS, -1 =
    none): a dropped product is added as an exact zero."""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        xs = np.ldexp(x.astype(F32), ex[:, None]).astype(F32)
        ws = np.ldexp(w.astype(F32), ew[:, None]).astype(F32)
        flush = mut == 2
        xh, xl = _split(xs, flush)
        wh, wl = _split(ws, flush)
        keep_lh, keep_hl = (mut != 0).astype(F32), (mut != 1).astype(F32)
        acc = np.zeros(x.shape[0], F32)
        for k in range(x.shape[1]):                       # products of two halfs are exact in fp32; every add rounds
            acc = (acc + xh[:, k] * wh[:, k]).astype(F32)
            acc = (acc + keep_lh * (xl[:, k] * wh[:, k])).astype(F32)
            acc = (acc + keep_hl * (xh[:, k] * wl[:, k])).astype(F32)
        back = np.where(mut == 3, -ex, -ex - ew)          # (the weight gradient: its cotangent's power of two)
        return np.ldexp(acc, back).astype(F32)


def emulate(x, w, *, x_absmax=False, w_exp=W_EXP, mutation=None):
    """The documented arithmetic for N outputs of K terms: x, w (N, K) arrays of fp32-representable numbers -> (N,) fp32.
    x_absmax: x is first multiplied by the power of two of max|x| (over the whole array, as nf_absmax_bits sees a tensor);
    w_exp: the power of two the second operand carries (10, or "absmax" for its own maximum).  `mutation`: None or one of
    MUTATIONS -- the same arithmetic with one thing wrong."""
    x, w = np.asarray(x, F64), np.asarray(w, F64)
    n = x.shape[0]
    ex = _absmax_exp(x) if x_absmax else 0
    ew = _absmax_exp(w) if w_exp == "absmax" else int(w_exp)
    mut = -1 if mutation is None else MUTATIONS.index(mutation)
    return _emulate_rows(x, w, np.full(n, ex), np.full(n, ew), np.full(n, mut))


def emulation_case(entry, scale, n_out=48, seed=0):
    """(x, w) (n_out, K) float64 arrays of the entry point's operands at the scale pair, drawn like the GPU tests' tensors."""
    spec = ENTRY_POINTS[entry]
    K = spec["K"]
    seed = seed + 1000 * sorted(ENTRY_POINTS).index(entry)
    base = {"field": base_field, "hidden": base_hidden, "cotangent": base_cotangent}[spec["x"]]
    x = scale_x(base((n_out, K), seed + 1), scale)
    wbase = base_cotangent if spec["w_exp"] == "absmax" else base_weights
    w = scale_w(wbase((n_out, K), seed + 2), scale)
    return x.numpy(), w.numpy()


_ENTRY_RUNS = {}


def _entry_runs(entry):
    """Every scale pair x (correct + every mutation) of one entry point in ONE pass of the emulation (rows stacked)."""
    if entry not in _ENTRY_RUNS:
        spec = ENTRY_POINTS[entry]
        xs, ws, exs, ews, muts, keys = [], [], [], [], [], []
        for scale in SCALES:
            x, w = emulation_case(entry, scale)
            ex = _absmax_exp(x) if spec["x_absmax"] else 0
            ew = _absmax_exp(w) if spec["w_exp"] == "absmax" else int(spec["w_exp"])
            for m in range(-1, len(MUTATIONS)):
                xs.append(x), ws.append(w)
                exs.append(np.full(len(x), ex)), ews.append(np.full(len(x), ew)), muts.append(np.full(len(x), m))
                keys.append((scale, None if m < 0 else MUTATIONS[m]))
        got = _emulate_rows(np.concatenate(xs), np.concatenate(ws), np.concatenate(exs), np.concatenate(ews), np.concatenate(muts))
        n = len(xs[0])
        _ENTRY_RUNS[entry] = {k: (xs[i], ws[i], got[i * n:(i + 1) * n].astype(F64)) for i, k in enumerate(keys)}
    return _ENTRY_RUNS[entry]


def emulation_report(entry, scale, mutation=None, act="tanh"):
    """Worst err / (B_i / C_SPLIT) of the (mutated) emulation against float64 over the outputs of one case -- of the
    pre-activation -- and, for an entry point with an activation, worst err / (B_i + ACT_EXTRA max|ref|) of the activated
    output with B_i at the module's C_SPLIT.  Returns (ratio_linear_at_c1, ratio_as_asserted)."""
    spec = ENTRY_POINTS[entry]
    x, w, got = _entry_runs(entry)[(scale, mutation)]
    ref = (x * w).sum(1)
    b1 = bound_terms((np.abs(x) * np.abs(w)).sum(1), np.abs(w).sum(1), np.abs(x).sum(1))
    with np.errstate(over="ignore", invalid="ignore"):
        lin = float(np.max(np.abs(got - ref) / b1))
        if not spec["act"]:
            return lin, lin / C_SPLIT
        f = np.tanh if act == "tanh" else (lambda v: 1.0 / (1.0 + np.exp(-v)))
        ra = f(ref)
        extra = ACT_EXTRA * np.abs(ra).max() + (K5S_CARRIED if entry == "small_lattice_coupling" else 0.0)
        asserted = float(np.max(np.abs(f(got) - ra) / (C_SPLIT * b1 + extra)))
    return lin, asserted

"""Shared by tests/test_batch_slabs.py (device) and tests/test_batch_slabs_host.py (host): the batch sizes that cross
`_hip.MAX_B`, the rows every case looks at, row-dependent log0 and cotangents, the float64 references of the batch-slab
cases that tests/tile_cases.py does not already have, and COVERED -- which test of tests/test_batch_slabs.py runs which
`_slabs` loop of normflow__amd/_hip.py.  The host test parses _hip.py and fails when a function with a `_slabs(` call is
missing from COVERED, so a new loop cannot arrive without a crossing-batch test."""
import functools

import torch

from normflow__amd import _hip
from oracle import nf_oracle as O
import tile_cases as TC
from tile_cases import _on_cpu, _gen, _randn

MAX_B = _hip.MAX_B
B2 = MAX_B + 5              # two slabs, a ragged tail of 5 rows
B3 = 2 * MAX_B + 3          # three slabs, beyond the C entry points' 65535 rows: two slabs of rqs_knots (step 65535)
LAT6 = (6,)                 # V = 6 sites, alternating activity
TAIL_WEIGHT = 1000.0        # the cotangents of the rows >= MAX_B in a batch-reduced gradient (see tail_weights)

# function of normflow__amd/_hip.py with a `_slabs(` loop -> the tests of tests/test_batch_slabs.py that cross its limit
COVERED = {
    "_rqs_call": ("test_rqs_maps", "test_rqs_fp16_storage"),
    "_rqs_vjp_call": ("test_rqs_vjps",),
    "multi_rqs_sites": ("test_multi_rqs_sites",),
    "rqs_knots": ("test_rqs_knots_three_slabs",),
    "MultiRQSCouplingFn.forward": ("test_multi_rqs_chains_the_log_det",),
    "MultiRQSCouplingFn.backward": ("test_multi_rqs_chains_the_log_det",),
    "affine_sites": ("test_affine_maps",),
    "AffineCouplingFn.forward": ("test_affine_maps", "test_affine_fp16_storage", "test_log0_none_and_python_number"),
    "AffineCouplingFn.backward": ("test_affine_vjps",),
    "DistConvFn.forward": ("test_distconv_maps",),
    "DistConvFn.backward": ("test_distconv_vjps_and_knot_gradient",),
    "DistConvSitesFn.forward": ("test_distconv_maps",),
    "DistConvSitesFn.backward": ("test_distconv_vjps_and_knot_gradient",),
    "_conv_launch": ("test_conv_layer_and_gradients",),
    "conv_weight_grad": ("test_conv_layer_and_gradients", "test_split16_weight_gradient"),
    "conv_first_split16": ("test_split16_chain",),
    "conv_layer_split16": ("test_split16_chain",),
    "conv_affine_split16": ("test_split16_chain",),
    "conv_rqs": ("test_split16_chain",),
    "Phi4ActionFn.forward": ("test_phi4_endpoints",),
    "Phi4ActionFn.backward": ("test_phi4_endpoints",),
    "Phi4ActionDensityFn.forward": ("test_phi4_endpoints",),
    "Phi4ActionDensityFn.backward": ("test_phi4_endpoints",),
    "NormalLogProbFn.forward": ("test_normal_logprob",),
    "NormalLogProbFn.backward": ("test_normal_logprob",),
    "normal_sample": ("test_normal_sample_is_one_stream", "test_hmc_paths_agree_beyond_one_slab"),
}

# wrapper of normflow__amd/_hip.py WITHOUT a slab loop -> its test at a batch beyond the limit
NO_LOOP = {
    "PadeFn": "test_pade_beyond_65535",
    "spline_eval": "test_spline_eval_beyond_65535",
    "small_lattice_coupling": "test_small_lattice_coupling_beyond_65535",
    "lattice_measure": "test_lattice_measure_beyond_65535",
    "metropolis_chains": "test_metropolis_chains_and_select_beyond_65535",
    "metropolis_select": "test_metropolis_chains_and_select_beyond_65535",
    "SpectralFilterFn": "test_spectral_filter_beyond_65535",
    "block_propose": "test_block_propose_and_accept_beyond_65535",
    "block_accept": "test_block_propose_and_accept_beyond_65535",
    "FusedLastRqsFn": ("test_fused_last_rqs_beyond_one_slab", "test_fused_last_rqs_beyond_65535"),
}


def rows_R(B):
    """The rows around every slab edge of a batch of B."""
    rows = {0, 1, MAX_B - 2, MAX_B - 1, MAX_B, MAX_B + 1, B - 1}
    if B > 2 * MAX_B:
        rows |= {2 * MAX_B - 1, 2 * MAX_B, 65535}
    return sorted(r for r in rows if 0 <= r < B)


@_on_cpu
def log0_rows(B):
    """log0[b] = b / 1024 (exact in float32): a slab that reads another slab's rows is off by 32."""
    return torch.arange(B, dtype=torch.float64) / 1024.0


@_on_cpu
def cotangents(seed, *shape):
    """Seeded N(0, 1) cotangents, distinct in every row."""
    return _randn(_gen(seed), *shape)


@_on_cpu
def tail_weights(B):
    """(B,) weights of the cotangents of a batch-REDUCED gradient: 1 below MAX_B, TAIL_WEIGHT from there on.  A sum of
    MAX_B random terms grows like sqrt(MAX_B) = 181, the few rows of the last slab like sqrt(5): with 1000 the last
    slab carries about ten times the first one's part of the sum, so a dropped or overwritten slab is an error of order
    one either way."""
    w = torch.ones(B, dtype=torch.float64)
    w[MAX_B:] = TAIL_WEIGHT
    return w


def rel_to_max(got, ref):
    """max|got - ref| / max|ref|: the metric of the weight-gradient tests (test_conv_wgrad_*_kernel_vs_autograd)."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)


# ------------------------------------------------------------------------------------------------ distconv, K = 5
@functools.lru_cache(maxsize=None)
@_on_cpu
def dc_case(stages, inverse, masked, rows=B2, V=6, K=5):
    """tile_cases.dc_case with K = 5 knots: inputs and the float64 (and float32) chain of test_site_densities._chain."""
    g = _gen(7000 + 10 * stages + 2 * int(inverse) + int(masked))
    real_in = (stages & 4) if inverse else (stages & 1)
    x = _randn(g, rows, V) if real_in else torch.rand((rows, V), generator=g, dtype=torch.float64) * 0.96 + 0.02
    knots = TC.dc_knots(seed=9, K=K)
    mask = TC.dc_mask(V) if masked else None
    val, terms = TC.dc_chain(x, knots, stages, inverse, mask)
    v32, t32 = TC.dc_chain(x.float(), knots.float(), stages, inverse, mask)
    return dict(x=x, knots=knots, mask=mask, val=val, terms=terms, val32=v32, terms32=t32)


@_on_cpu
def dc_vjp_ref(case, stages, inverse, gy, gl, per_site, rows=None, dtype=torch.float64):
    """(grad_in (rows, V), grad_knots (3, K) summed over the rows) by autograd through the restated chain."""
    sl = slice(None) if rows is None else rows
    x = case["x"][sl].to(dtype).clone().requires_grad_(True)
    k = case["knots"].to(dtype).clone().requires_grad_(True)
    val, terms = TC.dc_chain(x, k, stages, inverse, case["mask"])
    d = terms if per_site else terms.sum(1)
    return torch.autograd.grad((val * gy[sl].to(dtype)).sum() + (d * gl[sl].to(dtype)).sum(), [x, k])


# ------------------------------------------------------------------------------------------------ convolutions
@_on_cpu
def conv_case(lattice, cin, cout, rows, seed=0):
    g = _gen(8000 + 10 * cin + cout + seed)
    d = len(lattice)
    x = _randn(g, rows, cin, *lattice)
    w = 0.3 * _randn(g, cout, cin, *((3,) * d))
    b = _randn(g, cout)
    return x, w, b


@_on_cpu
def conv_grads_ref(x, w, b, go, act=None):
    """(out, grad x, grad w, grad b) of act(circular conv) in float64 by autograd through the oracle's convolution."""
    xo, wo, bo = (t.clone().requires_grad_(True) for t in (x, w, b))
    out = O._ACTS[act](O.circular_conv_fast(xo, wo, bo))
    gx, gw, gb = torch.autograd.grad(out, (xo, wo, bo), go)
    return out.detach(), gx, gw, gb

"""The split-fp16 chain and the fused small-lattice kernels depend on their inputs only.

K5c (first layer -> fp16 pairs), K5g (hidden layer on pairs), K5h (last layer + RQ spline), the fused affine layer and K5s
(a whole small-lattice atom in one launch) use static item schedules and add their partial sums in a fixed order, so a pass
is a function of (input, weights, options).  A race (an LDS-DMA read before its wait), a read of memory nobody wrote, or
state left by an earlier call would make the output depend on timing, on leftover memory or on a sample's place in the
batch; one run per kernel on fresh small tensors cannot see that.  So each kernel runs here with many items per persistent
workgroup (the pipelines stage item m + 1 while item m multiplies) and every case asserts:

  * repeat    -- three passes over the same inputs give the same bits;
  * poison    -- outputs and log-det workspace filled with NaN (0xFF bytes), 0x5A bytes or zeros before the call: the same
                 bits, finite.  A poisoned block is taken back from torch's caching allocator by pointer (or passed as out=);
                 the case fails if the kernel was not handed it, so it never passes without the poison in place;
  * position  -- a permuted batch gives the permuted rows; samples 0, B/2 and B-1 run alone give their rows of the full run;
  * fp64      -- samples 0 and B-1 (the tail of the persistent loop) against the fp64 oracle at the existing test's bound.

Then the bench network at its own size (32^4, batch 1024) and config 5 (48^4, fp16 storage) pass twice, bitwise; and the
host-side state that also feeds a launch -- the pipe option's weight layout, weights edited through `.data` -- is checked
against a freshly built network.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from normflow__amd import _hip
from normflow__amd.mask import EvenOddMask
from normflow__amd.nn import ConvAct, RQSplineCoupling_, AffineCoupling_, ModuleList_
from oracle import nf_oracle as O

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None
LIM = dict(xlim=(-5.0, 5.0), ylim=(-5.0, 5.0), extrap={'left': 'linear', 'right': 'linear'})
POISONS = (0xFF, 0x5A, 0x00)          # 0xFF bytes: NaN in fp16, fp32 and fp64; 0x5A: a finite non-zero sentinel


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max()) / max(1.0, float(b.abs().max()))


# ------------------------------------------------------------------------------------------------------------- helpers
def _bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def assert_same(got, want, what):
    """Bitwise equality; on failure: how many samples differ, the first differing (sample, index...) and the largest
    difference, so the message names the tile that went wrong."""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    ne = (_bits(got) != _bits(want)).reshape(got.shape[0], -1)
    bad = ne.any(1)
    if not bool(bad.any()):
        return
    rows = bad.nonzero().flatten()
    s = int(rows[0])
    first = int(ne[s].nonzero()[0])
    where = (s,) + tuple(int(i) for i in np.unravel_index(first, tuple(got.shape[1:])))
    d = (got[rows[:16]].double() - want[rows[:16]].double()).abs()
    dmax = float(d.nan_to_num(nan=float('inf')).max())
    raise AssertionError(f"{what}: {int(bad.sum())} of {got.shape[0]} samples differ (first: {rows[:8].tolist()}); first "
                         f"difference at (sample, index...) {where}: {got[where].item()!r} vs {want[where].item()!r}; "
                         f"max |difference| over the first 16 such samples {dmax:.3e}")


def poisoned_block(nbytes, byte):
    """Fill a block of nbytes with `byte` and hand it back to torch's caching allocator; returns its address.  The next
    allocation of that size on this stream gets this block (the caller checks that it did)."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()             # no other cached block of this size to compete with
    blk = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    blk.fill_(byte)
    ptr = blk.data_ptr()
    del blk
    return ptr


class poisoned_workspace:
    """Every `_hip._workspace` buffer (the per-workgroup log-det partials, nf_workspace_bytes of them) comes out filled with
    `byte`; counts the buffers handed out."""

    def __init__(self, byte):
        self.byte, self.calls = byte, 0

    def __enter__(self):
        self._orig = _hip._workspace

        def ws(B, V, device):
            t = self._orig(B, V, device)
            assert t.numel() >= _hip.load().nf_workspace_bytes(B, V)
            t.fill_(self.byte)
            self.calls += 1
            return t
        _hip._workspace = ws
        return self

    def __exit__(self, *exc):
        _hip._workspace = self._orig
        return False


def check_invariance(run, B, name):
    """run(idx, poison) -> tuple of batch-first outputs of the kernel on samples idx (None: the whole batch in order); with
    poison = a byte, every output and workspace buffer the kernel writes is filled with it first.  Returns the full run."""
    ref = run(None, None)
    for t in ref:
        assert bool(torch.isfinite(t).all()), f"{name}: non-finite output"
    for rep in range(2):
        for i, (a, b) in enumerate(zip(run(None, None), ref)):
            assert_same(a, b, f"{name}: repeat {rep + 1}, output {i}")
    for byte in POISONS:
        got = run(None, byte)
        for i, (a, b) in enumerate(zip(got, ref)):
            assert_same(a, b, f"{name}: outputs after 0x{byte:02X}-poisoned memory, output {i}")
        del got
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(B), device='cpu').to(DEV)
    for i, (a, b) in enumerate(zip(run(perm, None), ref)):
        assert_same(a, b[perm], f"{name}: permuted batch, output {i}")
    for s in (0, B // 2, B - 1):
        one = torch.tensor([s], device=DEV)
        for i, (a, b) in enumerate(zip(run(one, None), ref)):
            assert_same(a, b[s:s + 1], f"{name}: sample {s} alone, output {i}")
    return ref


def _take(t, idx):
    return t if idx is None else t[idx].contiguous()


def _alloc_run(fn, nbytes, poison):
    """fn() with its (single, large) output allocated in a poisoned block; asserts the kernel was handed that block."""
    if poison is None:
        return fn()
    ptr = poisoned_block(nbytes, poison)
    out = fn()
    assert out[0].data_ptr() == ptr, "the poisoned block was not reused: the poison test would be vacuous"
    return out


def _net(cout, seed, hidden=8):
    """ConvAct 1 -> h -> h -> cout with the existing tests' scaling (last layer x 0.3); (first, hidden, last) (w, b)."""
    torch.manual_seed(seed)
    net = ConvAct(1, cout, 3, conv_dim=4, hidden_sizes=[hidden, hidden], acts=['tanh', 'tanh', None]).to(DEV, torch.float32)
    with torch.no_grad():
        for p_ in list(net.parameters())[-2:]:
            p_.mul_(0.3)
    return net, [(c.weight.detach(), c.bias.detach()) for c in net if hasattr(c, 'weight')]


def _hidden16(shape, B, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    h = torch.tanh(torch.randn((B, 8) + shape, generator=g, device=DEV, dtype=torch.float32))
    return _hip.to_split16(h)


# Row lengths 32, 48 and 64 / 80; every persistent workgroup (256) takes many items of each batch.
SPLIT_CASES = [((16, 16, 16, 32), 64), ((8, 16, 16, 48), 48), ((8, 8, 16, 64), 64), ((4, 8, 8, 80), 96)]
T = _hip.ACT_CODES['tanh']


# --------------------------------------------------------------------------------------------------- K5c, K5g
@pytest.mark.parametrize("shape,B", SPLIT_CASES)
def test_k5c_first_layer_state(shape, B):
    """conv_first_split16 (K5c): x (B, 1, *L) fp32 -> the fp16 pair tensor."""
    assert _hip.load().nf_conv_first_split16_supported((C.c_int32 * 4)(*shape), (C.c_int32 * 4)(3, 3, 3, 3), 8, T)
    _, layers = _net(46, 5)
    w, b = layers[0]
    x = torch.randn((B, 1) + shape, generator=torch.Generator(device=DEV).manual_seed(1), device=DEV, dtype=torch.float32)
    V = int(np.prod(shape))

    def run(idx, poison):
        xi = _take(x, idx)
        return _alloc_run(lambda: (_hip.conv_first_split16(xi, w, b, T),), xi.shape[0] * V * 32, poison)

    (out,) = check_invariance(run, B, f"K5c {shape}")
    for s in (0, B - 1):
        ref = torch.tanh(O.circular_conv_fast(x[s:s + 1].double().cpu(), w.double().cpu(), b.double().cpu()))
        # the bound of the split-chain tests (tests/test_gpu_parity.py, tests/test_k5g_stacked.py)
        assert rel(_hip.from_split16(out[s:s + 1], shape), ref) <= 1e-5, (s, rel(_hip.from_split16(out[s:s + 1], shape), ref))


@pytest.mark.parametrize("shape,B", SPLIT_CASES)
def test_k5g_hidden_layer_state(shape, B):
    """conv_layer_split16 (K5g): pairs in, pairs out."""
    _, layers = _net(46, 6)
    w, b = layers[1]
    h16 = _hidden16(shape, B, 2)

    def run(idx, poison):
        hi = _take(h16, idx)
        return _alloc_run(lambda: (_hip.conv_layer_split16(hi, w, b, T, shape),), hi.numel() * 2, poison)

    (out,) = check_invariance(run, B, f"K5g {shape}")
    for s in (0, B - 1):
        h = _hip.from_split16(h16[s:s + 1], shape).double().cpu()
        ref = torch.tanh(O.circular_conv_fast(h, w.double().cpu(), b.double().cpu()))
        got = _hip.from_split16(out[s:s + 1], shape)
        assert rel(got, ref) <= 1e-5, (s, rel(got, ref))       # tests/test_k5g_stacked.py's bound


# ---------------------------------------------------------------------------------- K5h and the fused affine layer
def _coupling_inputs(shape, B, seed):
    mask = EvenOddMask(shape=shape)
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = 1.5 * torch.randn((B,) + shape, generator=g, device=DEV, dtype=torch.float32)
    xa = mask.purify(x, 0).reshape(B, -1).contiguous()
    l0 = torch.randn(B, generator=g, device=DEV, dtype=torch.float32)
    return mask, xa, l0


def _fused_run(call, B, V, ldt=torch.float32):
    """run() of a wrapper that takes out=(y, logJ) and a log-det workspace: poison both."""
    def run_for(xa, l0, h16, idx, poison):
        xi, li, hi = _take(xa, idx), _take(l0, idx), _take(h16, idx)
        n = xi.shape[0]
        y = torch.empty((n, V), dtype=xa.dtype, device=DEV)
        lj = torch.empty(n, dtype=ldt, device=DEV)
        if poison is None:
            call(hi, xi, li, (y, lj))
            return y, lj
        _bits(y).view(torch.uint8).fill_(poison)
        _bits(lj).view(torch.uint8).fill_(poison)
        with poisoned_workspace(poison) as ws:
            call(hi, xi, li, (y, lj))
        assert ws.calls >= 1, "the kernel took no workspace: the poison test would be vacuous"
        return y, lj
    return run_for


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("shape,B", SPLIT_CASES)
def test_k5h_fused_last_layer_state(shape, B, inverse):
    """conv_rqs(..., unit_input=True, lattice=...) (K5h): pairs + x_active -> spline output and log|J|, forward and inverse."""
    V = int(np.prod(shape))
    _, layers = _net(46, 7)
    w, b = layers[2]
    h16 = _hidden16(shape, B, 3)
    mask, xa, l0 = _coupling_inputs(shape, B, 4)
    a = mask.checkerboard_parity(0)
    opts = _hip.make_rqs_opts(16, LIM["xlim"], LIM["ylim"], LIM["extrap"], _hip.LAYOUT_PAIR)

    def call(hi, xi, li, out):
        _hip.conv_rqs(hi, w, b, xi, li, a, opts, inverse, unit_input=True, lattice=shape, out=out)
        assert _hip.load().nf_conv_last_path() == 3, "the split-fp16 fused kernel did not run"

    run_for = _fused_run(call, B, V)
    y, lj = check_invariance(lambda idx, poison: run_for(xa, l0, h16, idx, poison), B, f"K5h {shape} inverse={inverse}")
    am = O.channel_mask(shape, 0)
    for s in (0, B - 1):
        out = O.circular_conv_fast(_hip.from_split16(h16[s:s + 1], shape).double().cpu(), w.double().cpu(), b.double().cpu())
        x64 = xa[s:s + 1].reshape((1,) + shape).double().cpu()
        if not inverse:
            yo, lo = O.rqs_coupling_atom(x64, out, am, log0=l0[s:s + 1].double().cpu(), **LIM)
            # north_star's 1e-5 (tests/test_gpu_parity.py::test_split_fp16_fused_last_layer)
            assert rel(y[s:s + 1].reshape(yo.shape), yo) <= 1e-5 and rel(lj[s:s + 1], lo) <= 1e-5, s
        else:
            # the well-conditioned statement of the inverse (check_fused_round_trip): the fp64 forward map of the kernel's
            # x lands on the input, and the log-dets cancel
            yo, lo = O.rqs_coupling_atom(y[s:s + 1].reshape(x64.shape).double().cpu(), out, am, log0=lj[s:s + 1].double().cpu(), **LIM)
            assert rel(yo, x64) <= 2e-5 and rel(lo, l0[s:s + 1]) <= 1e-5 * max(1.0, float(lj[s].abs())), s


@pytest.mark.parametrize("shape,B", SPLIT_CASES[:3])
def test_fused_affine_layer_state(shape, B):
    """conv_affine_split16: pairs + x_active -> affine coupling output and log|J|."""
    V = int(np.prod(shape))
    _, layers = _net(2, 8)
    w, b = layers[2]
    h16 = _hidden16(shape, B, 5)
    mask, xa, l0 = _coupling_inputs(shape, B, 6)
    a = mask.checkerboard_parity(0)

    def call(hi, xi, li, out):
        _hip.conv_affine_split16(hi, w, b, xi, li, a, False, shape, out=out)

    run_for = _fused_run(call, B, V)
    y, lj = check_invariance(lambda idx, poison: run_for(xa, l0, h16, idx, poison), B, f"fused affine {shape}")
    am = O.channel_mask(shape, 0)
    for s in (0, B - 1):
        out = O.circular_conv_fast(_hip.from_split16(h16[s:s + 1], shape).double().cpu(), w.double().cpu(), b.double().cpu())
        yo, lo = O.affine_coupling_atom(xa[s:s + 1].reshape((1,) + shape).double().cpu(), out, am, log0=l0[s:s + 1].double().cpu())
        # tests/test_gpu_parity.py::test_fused_affine_layer_on_the_split_chain's bound
        assert rel(y[s:s + 1].reshape(yo.shape), yo) <= 1e-5 and rel(lj[s:s + 1], lo) <= 1e-5, s


# --------------------------------------------------------------------------------------------------------------- K5s
@pytest.mark.parametrize("shape,B,kind", [((16, 16, 16), 1024, 'rqs3d'), ((16, 16, 16), 1024, 'rqs'), ((16, 16, 16), 1024, 'affine'),
                                          ((16, 16), 4096, 'affine')])
def test_k5s_small_lattice_state(shape, B, kind):
    """small_lattice_coupling (rqs with out= given, affine and rqs): a whole atom of a small lattice per launch."""
    m = 16
    cout = 2 if kind == 'affine' else 3 * m - 2
    torch.manual_seed(9)
    d = len(shape)
    acts = ['tanh', 'tanh', None]
    net = ConvAct(1, cout, 3, conv_dim=d, hidden_sizes=[8, 8], acts=acts).to(DEV, torch.float32)
    with torch.no_grad():
        for p_ in list(net.parameters())[-2:]:
            p_.mul_(0.3)
    mask = EvenOddMask(shape=shape)
    g = torch.Generator(device=DEV).manual_seed(10)
    x = 1.3 * torch.randn((B,) + shape, generator=g, device=DEV, dtype=torch.float32)
    xa, xf = mask.purify(x, 0), mask.purify(x, 1)
    l0 = torch.randn(B, generator=g, device=DEV, dtype=torch.float32)
    plan = net.small3d_plan()
    assert plan is not None
    packed, biases, pacts, pcout = plan
    a = mask.checkerboard_parity(0)
    lim4 = dict(xlim=(-4.0, 4.0), ylim=(-4.0, 4.0), extrap={'left': 'linear', 'right': 'linear'})
    opts = None if kind == 'affine' else _hip.make_rqs_opts(m, lim4["xlim"], lim4["ylim"], lim4["extrap"], _hip.LAYOUT_PAIR)

    def run(idx, poison):
        xai, xfi, li = _take(xa, idx), _take(xf, idx), _take(l0, idx)
        n = xai.shape[0]
        if kind == 'rqs3d':
            y = torch.empty_like(xai)
            lj = torch.empty(n, dtype=torch.float32, device=DEV)
            if poison is not None:
                _bits(y).view(torch.uint8).fill_(poison)
                _bits(lj).view(torch.uint8).fill_(poison)
            return _hip.small_lattice_coupling(0, xfi, xai, packed, biases, li, a, pcout, pacts, opts, False, out=(y, lj))
        call = lambda: _hip.small_lattice_coupling(1 if kind == 'affine' else 0, xfi, xai, packed, biases, li, a, pcout, pacts,
                                                   opts, False)
        return _alloc_run(call, xai.numel() * 4, poison)

    y, lj = check_invariance(run, B, f"K5s {kind} {shape}")
    convs = [mod for mod in net if hasattr(mod, 'weight')]
    layers = [(c.weight.detach().double().cpu(), c.bias.detach().double().cpu()) for c in convs]
    am = O.channel_mask(shape, 0)
    idx = [0, B - 1]
    out = O.conv_act(xf[idx].double().cpu().unsqueeze(1), layers, acts)
    if kind == 'affine':
        yo, lo = O.affine_coupling_atom(xa[idx].double().cpu(), out, am, log0=l0[idx].double().cpu())
    else:
        yo, lo = O.rqs_coupling_atom(xa[idx].double().cpu(), out, am, log0=l0[idx].double().cpu(), **lim4)
    # tests/test_gpu_parity.py::test_small3d_fused_layer_vs_oracle / test_small_lattice_affine_and_2d_vs_oracle: 1e-5
    assert rel(y[idx], yo) <= 1e-5 and rel(lj[idx], lo) <= 1e-5, (rel(y[idx], yo), rel(lj[idx], lo))


# ------------------------------------------------------------------------------------- whole networks at full size
def _bench_net(lattice, layers):
    """bench.build_net as bench.py runs it: float32 torch defaults, weights initialised on the CPU."""
    import bench
    dtype, device = torch.get_default_dtype(), torch.get_default_device()
    torch.set_default_dtype(torch.float32)
    torch.set_default_device("cpu")
    try:
        return bench.build_net(lattice, layers, 16, DEV, seed=2024)
    finally:
        torch.set_default_dtype(dtype)
        torch.set_default_device(device)


def test_headline_network_two_passes_bitwise_and_k5h_atoms_vs_fp64(parity_report):
    """bench.py's timed pass at its own size (32^4, 8 RQ-spline layers, batch 1024, input seed 1234): two passes under no_grad
    give the same bits (bench.py's --dump-outputs claim).  Then 4 samples spread through the batch, pushed through the 8
    atoms as a sub-batch: the rows equal the full run's bitwise, and every layer's K5h atom is within the 1e-5 of
    test_headline_network_full_size_vs_fp64_oracle of the fp64 oracle on that atom's own inputs."""
    lattice, B = (32, 32, 32, 32), 1024
    net_, cpl = _bench_net(lattice, 8)
    g = torch.Generator(device=DEV).manual_seed(1234)
    x = torch.randn((B,) + lattice, device=DEV, dtype=torch.float32, generator=g)
    with torch.no_grad():
        y1, l1 = net_(x)
        assert _hip.load().nf_conv_last_path() == 3, "the split-fp16 kernels did not run"
        y2, l2 = net_(x)
    assert_same(l2, l1, "headline 32^4 x 1024: log|J|, pass 2 vs pass 1")
    assert_same(y2, y1, "headline 32^4 x 1024: y, pass 2 vs pass 1")
    del y2, l2
    samples = [0, 341, 682, 1023]
    idx = torch.tensor(samples, device=DEV)
    parts = list(cpl.mask.split(x[idx]))
    log0 = torch.zeros(len(samples), device=DEV, dtype=torch.float32)
    convs_of = lambda net: [(c.weight.detach().double().cpu(), c.bias.detach().double().cpu()) for c in net if hasattr(c, 'weight')]
    worst = 0.0
    for k, net in enumerate(cpl.nets):
        p = k % 2
        with torch.no_grad():
            got, lnew = cpl.atomic_forward(x_active=parts[p], x_frozen=parts[1 - p], parity=p, net=net, log0=log0)
        assert _hip.load().nf_conv_last_path() == 3
        out = O.conv_act(parts[1 - p].double().cpu().unsqueeze(1), convs_of(net), ['tanh', 'tanh', None])
        yo, lo = O.rqs_coupling_atom(parts[p].double().cpu(), out, O.channel_mask(lattice, p), log0=log0.double().cpu(), **LIM)
        del out
        ey, el = rel(got, yo), rel(lnew, lo)
        worst = max(worst, ey, el)
        assert ey <= 1e-5 and el <= 1e-5, (k, ey, el)
        parts[p], log0 = got, lnew
    parity_report("headline 32^4 b1024, 4 samples x 8 atoms", "worst y / logJ vs fp64", worst, 1e-5)
    assert_same(cpl.mask.cat(*parts), y1[idx], "headline: the 4 samples as a sub-batch vs their rows of the full batch")
    assert_same(log0, l1[idx], "headline: log|J| of the 4 samples as a sub-batch vs the full batch")


def test_config5_network_two_passes_bitwise():
    """Config 5's construction (48^4, fp16 parameters and field, affine + RQ-spline blocks on the split chain) at batch 12:
    two passes give the same bits, and the batch's last sample alone gives its row."""
    torch.manual_seed(48)
    shape, B, m = (48, 48, 48, 48), 12, 16
    mask = EvenOddMask(shape=shape)
    blocks = []
    for kind in ('affine', 'rqs'):
        Cc = 2 if kind == 'affine' else 3 * m - 2
        nets = [ConvAct(1, Cc, 3, conv_dim=4, hidden_sizes=[8, 8], acts=['tanh', 'tanh', None]) for _ in range(2)]
        for net in nets:
            with torch.no_grad():
                for p_ in list(net.parameters())[-2:]:
                    p_.mul_(0.3)
        blocks.append(AffineCoupling_(nets, mask=mask) if kind == 'affine' else RQSplineCoupling_(nets, mask=mask, **LIM))
    net_ = ModuleList_(blocks)
    net_.to(device=DEV, dtype=torch.float16)
    x = torch.randn((B,) + shape, device=DEV, dtype=torch.float32, generator=torch.Generator(device=DEV).manual_seed(5)).half()
    with torch.no_grad():
        y1, l1 = net_(x)
        assert _hip.load().nf_conv_last_path() == 3, "the split-fp16 kernels did not run"
        y2, l2 = net_(x)
        assert_same(y2, y1, "config 5 48^4 x 12: y, pass 2 vs pass 1")
        assert_same(l2, l1, "config 5 48^4 x 12: log|J|, pass 2 vs pass 1")
        del y2, l2
        y3, l3 = net_(x[B - 1:].contiguous())
    assert_same(y3, y1[B - 1:], "config 5: the last sample alone")
    assert_same(l3, l1[B - 1:], "config 5: log|J| of the last sample alone")


# ------------------------------------------------------------------------------------------- host-side state
def test_pipe_toggle_repacks_the_weights():
    """A layer whose weight layout depends on NF_OPT_PIPE (row-packed with it, fragment order without), run under pipe on,
    off, on: each result against the fp64 conv (the fp32 kernels' bound of test_conv_kernel_vs_oracle)."""
    shape, B = (4, 4, 4, 32), 6
    lib = _hip.load()
    lat4, k4 = (C.c_int32 * 4)(*shape), (C.c_int32 * 4)(3, 3, 3, 3)
    assert lib.nf_conv_weight_layout(lat4, k4, 8, 46, 0, 0, _hip.NF_F32) == 1
    g = torch.Generator(device='cpu').manual_seed(12)
    x = torch.randn((B, 8) + shape, generator=g, dtype=torch.float64, device='cpu')
    w = 0.05 * torch.randn((46, 8, 3, 3, 3, 3), generator=g, dtype=torch.float64, device='cpu')
    b = 0.3 * torch.randn(46, generator=g, dtype=torch.float64, device='cpu')
    ref = O.circular_conv_fast(x, w, b)
    xd, wd, bd = (t.to(DEV, torch.float32) for t in (x, w, b))
    tol = 1e-6 + 2e-7 * 0.3 * 8 * 81
    for pipe in (True, False, True):
        with torch.no_grad(), _hip.options(pipe=pipe):
            out = _hip.conv_layer(xd, wd, bd, 0)
            assert (_hip.load().nf_conv_last_path() == 1) == pipe
        assert rel(out, ref) <= tol, (pipe, rel(out, ref))


def _data_edit_case(kind):
    """(network, input) for the .data-edit test: kind 'affine16x16', 'rqs16^3', 'hidden4' (4-D, hidden width 4: the padded
    split chain), 'hidden16' (4-D, hidden width 16: the wide split kernels)."""
    torch.manual_seed(21)
    lim = dict(xlim=(-4.0, 4.0), ylim=(-4.0, 4.0), extrap={'left': 'linear', 'right': 'linear'})
    if kind == 'affine16x16':
        shape, d, cout, hidden, B = (16, 16), 2, 2, 8, 64
    elif kind == 'rqs16^3':
        shape, d, cout, hidden, B = (16, 16, 16), 3, 46, 8, 16
    elif kind == 'hidden4':
        shape, d, cout, hidden, B = (2, 4, 2, 32), 4, 46, 4, 5
    else:
        shape, d, cout, hidden, B = (2, 2, 4, 32), 4, 46, 16, 5
    nets = [ConvAct(1, cout, 3, conv_dim=d, hidden_sizes=[hidden, hidden], acts=['tanh', 'tanh', None]) for _ in range(2)]
    for net in nets:
        with torch.no_grad():
            for p_ in list(net.parameters())[-2:]:
                p_.mul_(0.3)
    mask = EvenOddMask(shape=shape)
    cpl = AffineCoupling_(nets, mask=mask) if cout == 2 else RQSplineCoupling_(nets, mask=mask, **lim)
    net_ = ModuleList_([cpl]).to(DEV, torch.float32)
    x = torch.randn((B,) + shape, device=DEV, dtype=torch.float32, generator=torch.Generator(device=DEV).manual_seed(22))
    return net_, x


@pytest.mark.parametrize("kind", ['affine16x16', 'rqs16^3', 'hidden4', 'hidden16'])
def test_data_edit_then_invalidate_equals_a_fresh_network(kind):
    """The documented procedure after editing weights through .data -- which bumps no version counter -- is
    `invalidate_weight_checks()`.  After a warm pass, a .data edit of one conv weight and that call, the eager pass and a
    GraphedFlow replay (the graph captured before the edit) equal a freshly built network with the edited weights, bitwise."""
    import copy
    from normflow__amd import GraphedFlow
    net_, x = _data_edit_case(kind)
    with torch.no_grad():
        y0, l0 = net_(x)
    graphed = GraphedFlow(net_, x)
    assert_same(graphed(x)[0], y0, f"{kind}: replay before the edit")
    conv = [mod for mod in net_[0].nets[0] if hasattr(mod, 'weight')][1]
    conv.weight.data.mul_(0.5)
    _hip.invalidate_weight_checks()
    fresh = copy.deepcopy(net_)            # new parameter tensors, new modules: no cache of any kind
    with torch.no_grad():
        yf, lf = fresh(x)
        ye, le = net_(x)
    assert not torch.equal(yf, y0), "the edit did not change the network"
    assert_same(ye, yf, f"{kind}: eager pass after the .data edit")
    assert_same(le, lf, f"{kind}: eager log|J| after the .data edit")
    yg, lg = graphed(x)
    assert_same(yg, yf, f"{kind}: GraphedFlow replay after the .data edit")
    assert_same(lg, lf, f"{kind}: GraphedFlow log|J| after the .data edit")

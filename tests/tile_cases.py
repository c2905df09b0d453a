"""Shapes that take the tiled element-wise kernels across workgroup, loop and sample boundaries, and the seeded inputs
and float64 references the tests of those regimes share (tests/test_tile_cases_host.py on the CPU,
tests/test_tile_boundaries.py on the GPU).  A plain module: no fixtures, no GPU work.

Every kernel concerned launches through `make_tiling` (csrc/nf_internal.h): a workgroup of `block` lanes walks `iters`
strides of one sample and writes one double partial per (sample, workgroup).  A case names the regime it must hit;
`assert_regime` holds it to the library's own planner (nf_plan_tiling / nf_rqs_plan_block), so a later change of the
planner cannot leave these tests passing on shapes that no longer reach the code they are about.

A case is P = 3 distinct samples tiled to B rows, row b = base[b % 3] (3 is coprime to every tile size): the float64
reference is needed for three rows only, every other row must equal its base row bitwise.
"""
import ctypes
import functools
import math
from collections import namedtuple

import torch

from normflow__amd import _hip
from oracle import nf_oracle as O

P = 3
LAT4 = (3, 5, 7, 11)          # 1155 sites, pairwise awkward extents: every carry of the coordinate chain fires
LAT4E = (3, 5, 7, 22)         # 2310 sites, even fastest axis (pair layout)
LAT1 = (1155,)
LAT2 = (35, 33)
LEAD2 = (2, 5, 7, 33)         # 2310 sites, leading extent 2: the forward and the backward neighbour coincide
ONE4 = (3, 1, 35, 11)         # 1155 sites with an explicit axis of extent 1: the site is its own neighbour there
BIG_V = 2 ** 22 + 3

Case = namedtuple("Case", "name lattice B units block iters blocks_x")


def sites(lattice):
    return math.prod(lattice)


def _c(name, lattice, B, block, iters, blocks_x, div=1, units=None):
    return Case(name, lattice, B, sites(lattice) // div if units is None else units, block, iters, blocks_x)


# name, lattice, B, workgroup size -> iters, workgroups per sample.  The literals restate the rule; the host test holds
# them to `restated_plan` and to the library.
CASES = {c.name: c for c in (
    _c("i1_w10", LAT4E, 3, 256, 1, 10),
    _c("i2_w3", LAT4, 4096, 256, 2, 3),
    _c("i4_w2", LAT4, 8192, 256, 4, 2),
    _c("i8_w2", LAT4E, 8192, 256, 8, 2),
    _c("odd_i1_w5", LAT4, 3, 256, 1, 5),
    _c("pair_i1_w5", LAT4E, 3, 256, 1, 5, div=2),
    _c("pair_i2_w3", LAT4E, 4096, 256, 2, 3, div=2),
    _c("pair_i4_w2", LAT4E, 8192, 256, 4, 2, div=2),
    _c("b64_i1_w19", LAT4, 3, 64, 1, 19),
    _c("b64_i8_w3", LAT4, 4096, 64, 8, 3),
    _c("b128_i1_w10", LAT4, 3, 128, 1, 10),
    _c("b128_i4_w3", LAT4, 4096, 128, 4, 3),
    _c("pair_b64_i8_w3", LAT4E, 4096, 64, 8, 3, div=2),
    _c("pair_b128_i4_w3", LAT4E, 4096, 128, 4, 3, div=2),
    _c("d1_i1_w5", LAT1, 3, 256, 1, 5),
    _c("d1_i2_w3", LAT1, 4096, 256, 2, 3),
    _c("d2_i1_w5", LAT2, 3, 256, 1, 5),
    _c("d2_i2_w3", LAT2, 4096, 256, 2, 3),
    _c("one4_i2_w3", ONE4, 4096, 256, 2, 3),
    _c("lead2_i1_w10", LEAD2, 3, 256, 1, 10),
    _c("lead2_i8_w2", LEAD2, 8192, 256, 8, 2),
    _c("sample32_2398", (2398,), 8192, 256, 2, 2, units=600),      # nf_normal_sample fp32: ceil(V / 4) Philox calls
    _c("sample32_2400", (2400,), 8192, 256, 2, 2, units=600),
    _c("sample64_2398", (2398,), 8192, 256, 4, 2, units=1199),     # fp64: ceil(V / 2)
    _c("sample64_2400", (2400,), 8192, 256, 4, 2, units=1200),
    _c("big_i2", (BIG_V,), 1, 256, 2, 8193),
    # (B, 1, 1, 2049, 2047) configurations, 2^22 - 1 sites: one below the iters = 2 threshold.  The case that showed
    # ScalarPhi4Action.action leaving out -w0 phi^2 for every explicit axis of extent 1 on the device.
    _c("big_phi4_i1", (1, 1, 2049, 2047), 1, 256, 1, 16384),
    _c("big_phi4_i2", (1, 1, 2051, 2047), 1, 256, 2, 8200),
)}


def restated_plan(units, B, block=256):
    """make_tiling of csrc/nf_internal.h, restated: iters doubles while (units // (2 block iters)) B >= 8192."""
    iters = 1
    while iters < 8 and (units // (block * iters * 2)) * B >= 8192:
        iters *= 2
    return iters, -(-units // (block * iters))


def library_plan(units, B, block=256):
    it, bx = ctypes.c_int(-1), ctypes.c_int64(-1)
    rc = _hip.load().nf_plan_tiling(units, B, block, ctypes.byref(it), ctypes.byref(bx))
    assert rc == 0, _hip.load().nf_last_error_string()
    return it.value, bx.value


def assert_regime(case, units=None, block=None):
    """The library plans `case` as the table says.  `units` / `block`: what the caller is about to launch, which must be
    the case's own (a test that tiles the pair layout on a full-layout case would cover something else)."""
    case = CASES[case] if isinstance(case, str) else case
    assert units is None or units == case.units, (case.name, units, case.units)
    assert block is None or block == case.block, (case.name, block, case.block)
    got = library_plan(case.units, case.B, case.block)
    assert got == (case.iters, case.blocks_x), (case.name, got, (case.iters, case.blocks_x))
    return case


def rqs_block(m, dtype, layout=0, fixed_x=None):
    """nf_rqs_plan_block for a linear-tailed family of m knots."""
    opts = _hip.make_rqs_opts(m, (-5.0, 5.0), (-5.0, 5.0), LIM["extrap"], layout, knots_x=fixed_x)
    return _hip.load().nf_rqs_plan_block(ctypes.byref(opts), {torch.float32: 0, torch.float64: 1, torch.float16: 2}[dtype])


def pade_plan(B, outer, C, inner):
    """(iters, blocks_x, G) of nf_pade, read from nf_pade_workspace_bytes: one 16-byte partial per unit, B G blocks_x
    units, blocks_x = ceil(nk / (256 iters)) with iters a power of two."""
    units = _hip.load().nf_pade_workspace_bytes(B, outer, C, inner) // 16
    RS = outer * C // B
    G = C if RS % C == 0 else 1
    nk = RS // G * inner
    blocks_x = units // (B * G)
    iters = 1
    while -(-nk // (256 * iters)) > blocks_x:
        iters *= 2
    assert -(-nk // (256 * iters)) == blocks_x and units == B * G * blocks_x
    return iters, blocks_x, G


# Pade layouts: field shape per sample, channel axis, and the B that gives iters 1 / 2 / 4 / 8 (C = 3) -- nf_pade's own
# rule, iters doubles while B G ceil(nk / (256 iters)) > 32768.
PADE_MID = dict(shape=(7, 3, 165), axis=2)      # (B, 7, 3, 165): outer = 7 B, inner = 165: step_q = 1, step_r = 91, wraps
PADE_LAST = dict(shape=(35, 33, 3), axis=-1)    # (B, 35, 33, 3): outer = 1155 B, inner = 1
PADE_ITERS = {3: 1, 2400: 2, 4096: 4, 8192: 8}
PADE_C1_ITERS = {3: 1, 8192: 2}                 # C = 1, (B, 1155): G = 1


def _on_cpu(fn):
    """The references are built on the CPU whatever torch's default device is (importing normflow__amd makes it the GPU
    where there is one)."""
    @functools.wraps(fn)
    def wrapped(*a, **kw):
        with torch.device("cpu"):
            return fn(*a, **kw)
    return wrapped


def tile_index(B, device=None):
    return torch.arange(B, device=device) % P


@_on_cpu
def log0_rows(B):
    """A distinct log0 per row (float64, CPU)."""
    return torch.randn(B, generator=_gen(77), dtype=torch.float64, device='cpu')


@_on_cpu
def counts(B):
    """How many of the B rows are copies of base row p."""
    return torch.tensor([len(range(p, B, P)) for p in range(P)], dtype=torch.float64)


def workgroup_share(terms, case, bx=0, row=0):
    """The part of a per-sample sum that workgroup (row, bx) of `case` contributes: `terms` (P, units) per-unit terms in
    the order the kernel walks them."""
    per = case.block * case.iters
    return float(terms.reshape(P, -1)[row, bx * per:(bx + 1) * per].double().sum())


def assert_sees_lost_partial(what, share, bound):
    """The condition on every reduced quantity: a result that lacks one workgroup's partial must miss the bound by 10x."""
    assert abs(share) >= 10.0 * bound, f"{what}: one workgroup's share {share:.3e} is not 10 x the bound {bound:.3e}"


def rel(a, b):
    """The metric of tests/test_gpu_parity.py: max|a - b| / max(1, max|b|)."""
    a, b = a.detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max()) / max(1.0, float(b.abs().max())) if b.numel() else 0.0


TOL = {torch.float64: dict(val=1e-9, grad=1e-8), torch.float32: dict(val=1e-5, grad=2e-4)}     # test_gpu_parity.TOL
LIM = dict(xlim=(-5.0, 5.0), ylim=(-5.0, 5.0), extrap={'left': 'linear', 'right': 'linear'})


def floor_tol(base, o32, o64):
    """The project's floor rule for a direction that is ill-conditioned in single precision:
    max(base, 2 x the error of the same oracle run in float32 against its float64 run)."""
    return max(base, 2.0 * rel(o32, o64))


def _gen(seed):
    return torch.Generator(device='cpu').manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(shape, generator=g, dtype=torch.float64, device='cpu')


@_on_cpu
def vjp_cotangents(g, site_shape, logj_shape):
    """Cotangents whose weighted sum over a tiled batch stays of the size of ONE sample's gradient: row 1 gets row 0's
    negated (rows 0 and 1 then share their inputs, so their parameter gradients cancel exactly), row 2's are scaled by
    2^-10.  Otherwise a batch-summed gradient of B = 8192 rows hides one workgroup's share (1/16384 of the sum) under
    the relative fp32 gradient bound of 2e-4."""
    gy, gl = _randn(g, *site_shape), _randn(g, *logj_shape)
    gy[1], gl[1] = -gy[0], -gl[0]
    gy[2], gl[2] = gy[2] * 2.0 ** -10, gl[2] * 2.0 ** -10
    return gy, gl


# ------------------------------------------------------------------------------------------------ RQ-spline couplings
@_on_cpu
def rqs_site_ref(xa, out, am, inverse, knots_x=None):
    """O.rqs_coupling_atom with the per-sample sum left out: (value, log-derivative per site)."""
    kx, ky, kd = O.knots_from_logits(out, LIM["xlim"], LIM["ylim"], knots_x, None)
    kx, ky, kd = (O._bcast_like(k, out) for k in (kx, ky, kd))
    full = (out.shape[0], kd.shape[1]) + tuple(out.shape[2:])
    kx, ky, kd = (k.expand(full) for k in (kx, ky, kd))
    kx, ky, kd = O.augment_knots(kx, ky, kd, axis=1, **LIM["extrap"])
    f = O.rqs_invert if inverse else O.rqs_evaluate
    val, g = f(kx, ky, kd, xa.unsqueeze(1), axis=1)
    return val.squeeze(1) * am, torch.log(g.squeeze(1)) * am


@functools.lru_cache(maxsize=None)
@_on_cpu
def rqs_case(lattice, m, parity, inverse, fixed_x=False, rows=P, seed=0, with32=True):
    """Seeded inputs as the existing tests draw them (x ~ N(0,1), logits ~ N(0, 0.5^2), limits +-5, linear tails) and the
    float64 oracle, all flattened to (rows, V): dict of x (active sites only), out (rows, C, V), act (V) 0/1, val, terms,
    and the same oracle run in float32 (val32, terms32)."""
    g = _gen(1000 + 10 * m + 2 * parity + int(inverse) + 100 * int(fixed_x) + seed)
    C = (0 if fixed_x else m - 1) + (m - 1) + m
    am = O.channel_mask(lattice, parity)
    x = _randn(g, rows, *lattice) * am
    out = 0.5 * _randn(g, rows, C, *lattice)
    kx = None
    if fixed_x:
        kx = torch.linspace(-5.0, 5.0, m, dtype=torch.float64) + torch.cat((torch.zeros(1), 0.3 * torch.rand(m - 2, generator=g) - 0.15, torch.zeros(1))).double()
    val, terms = rqs_site_ref(x, out, am, inverse, kx)
    v32, t32 = (rqs_site_ref(x.float(), out.float(), am.float(), inverse, None if kx is None else kx.float())
                if with32 else (val, terms))
    fl = lambda t: t.reshape(t.shape[0], -1)
    return dict(x=fl(x), out=out.reshape(rows, C, -1), act=am.reshape(-1), val=fl(val), terms=fl(terms), val32=fl(v32),
                terms32=fl(t32), knots_x=kx, lattice=lattice)


@_on_cpu
def rqs_vjp_ref(case, inverse, gy, gl):
    """Cotangents of (input, logits) of the map that ran, by autograd through the oracle."""
    am = case["act"]
    v = case["x"].clone().requires_grad_(True)
    out = case["out"].clone().requires_grad_(True)
    val, terms = rqs_site_ref(v, out, am, inverse, case["knots_x"])
    gv, gout = torch.autograd.grad((val * gy).sum() + (terms.sum(1) * gl).sum(), [v, out])
    return gv * am, gout * am


# ------------------------------------------------------------------------------------------------ affine / shift
@functools.lru_cache(maxsize=None)
@_on_cpu
def affine_case(lattice, n_ch, parity, inverse, rows=P):
    g = _gen(2000 + 10 * n_ch + 2 * parity + int(inverse))
    am = O.channel_mask(lattice, parity)
    x = _randn(g, rows, *lattice) * am
    out = 0.5 * _randn(g, rows, n_ch, *lattice)
    val, terms = affine_site_ref(x, out, am, inverse)
    v32, t32 = affine_site_ref(x.float(), out.float(), am.float(), inverse)
    fl = lambda t: t.reshape(t.shape[0], -1)
    return dict(x=fl(x), out=out.reshape(rows, n_ch, -1), act=am.reshape(-1), val=fl(val), terms=fl(terms), val32=fl(v32),
                terms32=fl(t32), lattice=lattice)


@_on_cpu
def affine_site_ref(x, out, am, inverse):
    """O.affine_coupling_atom / O.shift_coupling_atom with the sum left out."""
    if out.shape[1] == 1:
        return O.shift_coupling_atom(x, out, am, inverse=inverse)[0], torch.zeros_like(x)
    s = (out[:, 1] * am).abs()
    return O.affine_coupling_atom(x, out, am, inverse=inverse)[0], s if inverse else -s


@_on_cpu
def affine_vjp_ref(case, inverse, gy, gl):
    am = case["act"]
    v, out = case["x"].clone().requires_grad_(True), case["out"].clone().requires_grad_(True)
    val, terms = affine_site_ref(v, out, am, inverse)
    gv, gout = torch.autograd.grad((val * gy).sum() + (terms.sum(1) * gl).sum(), [v, out], allow_unused=True)
    return gv * am, gout * am


# ------------------------------------------------------------------------------------------------ distconv (K4)
@_on_cpu
def dc_knots(seed=5, K=7):
    """(3, K) shared knots of a SplineNet_ with random logits."""
    g = _gen(seed)
    kx, ky, kd = O.shared_spline_knots(0.8 * _randn(g, K - 1), 0.8 * _randn(g, K - 1), 0.8 * _randn(g, K))
    return torch.stack((kx, ky, kd))


@_on_cpu
def dc_mask(V):
    return (torch.arange(V) % 3 != 1).to(torch.uint8)


@_on_cpu
def dc_chain(x, knots, stages, inverse, mask=None):
    """`_chain` of tests/test_site_densities.py with the activity mask: (value, log-derivative per site)."""
    from test_site_densities import _chain
    if mask is None:
        return _chain(x, knots, stages, inverse)
    on = mask.bool().expand(x.shape)
    u, lg = _chain(torch.where(on, x, torch.full_like(x, 0.5)), knots, stages, inverse)
    return torch.where(on, u, x), torch.where(on, lg, torch.zeros_like(lg))


@functools.lru_cache(maxsize=None)
@_on_cpu
def dc_case(V, stages, inverse, masked, rows=P, twin=False):
    """twin: row 1 repeats row 0's input (the VJP tests, see vjp_cotangents)."""
    g = _gen(3000 + 10 * stages + 2 * int(inverse) + int(masked))
    real_in = (stages & 4) if inverse else (stages & 1)
    x = _randn(g, rows, V) if real_in else torch.rand((rows, V), generator=g, dtype=torch.float64) * 0.96 + 0.02
    if twin:
        x[1] = x[0]
    knots = dc_knots()
    mask = dc_mask(V) if masked else None
    val, terms = dc_chain(x, knots, stages, inverse, mask)
    v32, t32 = dc_chain(x.float(), knots.float(), stages, inverse, mask)
    return dict(x=x, knots=knots, mask=mask, val=val, terms=terms, val32=v32, terms32=t32)


@_on_cpu
def dc_vjp_ref(case, stages, inverse, gy, gl, per_site, dtype=torch.float64):
    """(grad_in, grad_knots per base row (P, 3, K)) by autograd through the restated chain."""
    x = case["x"].to(dtype).clone().requires_grad_(True)
    gin, gk = [], []
    for p in range(x.shape[0]):
        k = case["knots"].to(dtype).clone().requires_grad_(True)
        val, terms = dc_chain(x[p:p + 1], k, stages, inverse, case["mask"])
        d = terms if per_site else terms.sum(1)
        a, b = torch.autograd.grad((val * gy[p:p + 1].to(dtype)).sum() + (d * gl[p:p + 1].to(dtype)).sum(), [x, k])
        gin.append(a[p])
        gk.append(b)
    return torch.stack(gin), torch.stack(gk)


# ------------------------------------------------------------------------------------------------ Pade / real maps
@_on_cpu
def pade_module(kind, C, axis, seed=7):
    """A float64 CPU module of the kind with random per-channel weights."""
    from normflow__amd.nn import Pade11_, Pade22_, Pade32_, Tanh_
    with torch.device("cpu"):
        if kind == _hip.TANH:
            return Tanh_()
        mod = {_hip.PADE11: Pade11_, _hip.PADE22: Pade22_, _hip.PADE32: Pade32_}[kind](n_channels=C, channels_axis=axis).double()
    g = _gen(seed + kind)
    with torch.no_grad():
        for p in mod.parameters():
            p.copy_(0.7 * _randn(g, *p.shape))
    return mod


def pade_restate(mod, x, inverse):
    """The float64 restatements the Pade tests use: `restate` of tests/test_pade.py (Pade11_, Pade22_) and of
    tests/test_realmaps.py (Tanh_, Pade32_)."""
    from normflow__amd.nn import Pade11_, Pade22_
    if isinstance(mod, (Pade11_, Pade22_)):
        from test_pade import restate
    else:
        from test_realmaps import restate
    return restate(mod, x, inverse)


@functools.lru_cache(maxsize=None)
@_on_cpu
def pade_case(kind, shape, axis, inverse, rows=P, twin=False):
    C = 1 if axis is None else shape[axis if axis < 0 else axis - 1]
    mod = pade_module(kind, C, axis if axis is not None else 1)
    g = _gen(4000 + kind + int(inverse))
    if kind in (_hip.PADE11, _hip.PADE22):
        x = torch.rand((rows,) + shape, generator=g, dtype=torch.float64) * 0.96 + 0.02
    elif kind == _hip.TANH and inverse:
        x = torch.rand((rows,) + shape, generator=g, dtype=torch.float64) * 1.9 - 0.95
    else:
        x = 1.5 * _randn(g, rows, *shape)
    if twin:
        x[1] = x[0]
    with torch.no_grad():
        val, terms = pade_restate(mod, x, inverse)
        mod32 = pade_module(kind, C, axis if axis is not None else 1).float()
        v32, t32 = pade_restate(mod32, x.float().double(), inverse)     # float32 inputs and weights, exact arithmetic
    return dict(x=x, mod=mod, val=val, terms=terms, val32=v32, terms32=t32)


@_on_cpu
def pade_vjp_ref(case, inverse, gy, gl, per_site):
    """(grad_x, [grad of every weight per base row (P, C)]) by autograd through the restatement."""
    mod = case["mod"]
    params = list(mod.parameters())
    x = case["x"].clone().requires_grad_(True)
    gin, gw = [], []
    for p in range(x.shape[0]):
        val, terms = pade_restate(mod, x[p:p + 1], inverse)
        d = terms if per_site else terms.reshape(1, -1).sum(1)
        got = torch.autograd.grad((val * gy[p:p + 1]).sum() + (d * gl[p:p + 1]).sum(), [x] + params, allow_unused=True)
        gin.append(got[0][p])
        gw.append([t for t in got[1:]])
    return torch.stack(gin), [torch.stack([row[i] for row in gw]) for i in range(len(params))]


# ------------------------------------------------------------------------------------------------ end points
ACTION = dict(m_sq=0.9, lambd=0.5, kappa=0.6, a=1.1)


def phi4_terms(cfgs, w0, w2, w4):
    """Per-site terms of the action as nf_phi4_action sums them: w2 phi^2 + w4 phi^4 - w0 phi(x) sum_mu phi(x - mu)."""
    t = cfgs * cfgs * (w2 + w4 * cfgs * cfgs)
    for mu in range(1, cfgs.dim()):
        t = t - w0 * cfgs * torch.roll(cfgs, 1, mu)
    return t


@functools.lru_cache(maxsize=None)
@_on_cpu
def phi4_case(lattice, rows=P):
    from normflow__amd.action import ScalarPhi4Action
    act = ScalarPhi4Action(**ACTION)
    x = _randn(_gen(5000 + len(lattice)), rows, *lattice)
    terms = phi4_terms(x, *act.get_coef(len(lattice)))
    S = act.action(x)                                            # the host restatement (CPU tensors)
    assert rel(terms.reshape(rows, -1).sum(1), S) < 1e-12
    return dict(x=x, act=act, terms=terms.reshape(rows, -1), S=S, density=act.action_density(x))


@functools.lru_cache(maxsize=None)
@_on_cpu
def normal_case(V, affine, rows=P):
    g = _gen(6000 + int(affine))
    x = _randn(g, rows, V)
    loc = 0.5 * _randn(g, V) if affine else None
    scale = torch.rand(V, generator=g, dtype=torch.float64) + 0.5 if affine else None
    z = (x - loc) / scale if affine else x
    terms = -0.5 * z * z - (torch.log(scale) if affine else 0.0) - 0.5 * math.log(2 * math.pi)
    return dict(x=x, loc=loc, scale=scale, terms=terms)

"""Pade11_ / Pade22_ on an MI355X (nf_pade, nf_pade_vjp): values and log J against the reference's outputs
(tests/golden/pade.npz), per sample, per site and with a log0, in both directions; the round trip; gradients against
autograd through an fp64 restatement of the reference's formulas and torch.autograd.gradcheck; bitwise reproducible
parameter gradients; training eager and graphed; a field of more than 2^31 elements.

Errors are |got - ref| / max(1, |ref|) per element.  fp64: 1e-12.  fp32: the conditioned bound of tests/cond_bound.py is
built for the RQ-spline couplings and does not apply, so 2e-6.  Both plus what rounding moves the exact result by at
that site (see _slack): the reference's own root of the Pade22_ inverse, which cancels where |a| is small, and in fp32
the rounding of the input and the weights (a sample's log J: the sum of its sites' moves).  In fp64 the kernel is also
held to the exact result itself at 1e-12."""
import math

import pytest
import torch

import normflow__amd as nf
from normflow__amd import _hip
from normflow__amd.nn import Module_, ModuleList_, Expit_, Logit_, Pade11_, Pade22_

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
TOL = {torch.float64: 1e-12, torch.float32: 2e-6}
LN2 = math.log(2.0)


@pytest.fixture
def density():
    """Module_.propagate_density switched on for one block (a class attribute, as in the reference)."""
    class _Switch:
        def __enter__(self):
            Module_.propagate_density = True

        def __exit__(self, *exc):
            Module_.propagate_density = False
    yield _Switch()
    Module_.propagate_density = False


# ---------------------------------------------------------------------------------------------- fp64 restatement
def _params(mod, x):
    """Per-channel (d0, d1) of the module, shaped to broadcast against x (modules_.py:156-163, 210-220)."""
    sp = lambda w: torch.nn.functional.softplus(w, beta=LN2)
    shape = [1] * x.dim()
    if mod.n_channels > 1:
        shape[mod.channels_axis] = mod.n_channels
    if isinstance(mod, Pade11_):
        return sp(mod.w1.double()).reshape(shape), None
    return sp(mod.w0.double()).reshape(shape), sp(mod.w1.double()).reshape(shape)


def restate(mod, x, inverse, literal=False):
    """(value, per-site log-derivative) of the reference's formulas in fp64 (modules_.py:144-154, 181-208); the Pade22
    inverse by the same root in its cancellation-free form, or with literal=True as the reference writes it."""
    d0, d1 = _params(mod, x)
    if isinstance(mod, Pade11_):
        den = x + (1 - x) / d0 if inverse else x + (1 - x) * d0
        return x / den, (-1 if inverse else 1) * torch.log(d0) - 2 * torch.log(den)
    if inverse:
        b = (d1 + d0 - 2) * x - d0
        a = -1 - b
        if literal:
            z = torch.where(a == 0, -x / b, (-b - torch.sqrt(b * b - 4 * a * x)) / (2 * a))
        else:
            z = 2 * x / (-b + torch.sqrt(b * b - 4 * a * x))
    else:
        z = x
    den = 1 + (d1 + d0 - 2) * z * (1 - z)
    g1 = (d0 + 2 * (1 - d0) * z + (d1 + d0 - 2) * z ** 2) / den ** 2
    if inverse:
        return z, -torch.log(g1)
    return z * (z + d0 * (1 - z)) / den, torch.log(g1)


def _err(got, ref):
    got, ref = got.detach().double().cpu(), torch.as_tensor(ref).double().cpu()
    return ((got - ref).abs() / ref.abs().clamp(min=1.0))


def _slack(mod64, mod, x64, inverse):
    """Per element, how far two roundings move the exact result (the fp64 restatement with the cancellation-free root):
    the reference's own root (-b - sqrt(b^2 - 4ay)) / (2a), which cancels where |a| << |b| (Pade22_ inverse: a = -s y
    when d0 = 1, at y = 1e-7), and, for an fp32 module, rounding the input and the weights to fp32.  Returns the exact
    (value, per-site log) and the absolute moves of value, per-sample log J and per-site log."""
    with torch.no_grad():
        x = x64.to(DEV)
        ey, es = restate(mod64, x, inverse)
        my, ms = torch.zeros_like(ey), torch.zeros_like(es)
        variants = []
        if inverse and isinstance(mod64, Pade22_):
            variants.append((mod64, x, True))
        if next(mod.parameters()).dtype == torch.float32:
            variants.append((mod, x.float().double(), False))
        for m, xv, lit in variants:
            vy, vs = restate(m, xv, inverse, literal=lit)
            my, ms = my + (vy - ey).abs(), ms + (vs - es).abs()
    ml = ms.reshape(ms.shape[0], -1).sum(1)
    return ey.cpu(), es.cpu(), my.cpu(), ml.cpu(), ms.cpu()


def _case_module(z, name, dtype):
    kw = dict(n_channels=int(z[f"{name}/n_channels"]), channels_axis=int(z[f"{name}/channels_axis"]))
    mod = Pade11_(**kw) if int(z[f"{name}/kind"]) == 11 else Pade22_(symmetric=bool(z[f"{name}/symmetric"]), **kw)
    state = {k.split("/", 2)[2]: torch.from_numpy(z[k]) for k in z.files if k.startswith(f"{name}/state/")}
    mod.load_state_dict(state)
    return mod.to(DEV, dtype)


NAMES = ['p11_c1', 'p11_c3_ax1', 'p11_c3_axm1', 'p11_zero', 'p22_c1', 'p22_c3_ax1', 'p22_c3_axm1', 'p22_sym_c3_ax1',
         'p22_sym_c1', 'p22_d0one', 'p22_zero']


# ---------------------------------------------------------------------------------------------- values vs fixture
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("name", NAMES)
def test_values_and_logj_vs_reference(golden, density, parity_report, name, dtype):
    z = golden("pade")
    mod = _case_module(z, name, dtype)
    x64 = torch.from_numpy(z[f"{name}/x"])
    x = x64.to(DEV, dtype)
    B = x.shape[0]
    log0 = torch.linspace(-1.0, 2.0, B, dtype=dtype, device=DEV)
    log0_sites = log0.reshape((B,) + (1,) * (x.dim() - 1)).expand(x.shape).contiguous()
    tol = TOL[dtype]
    mod64 = _case_module(z, name, torch.float64)
    for d, inverse in (("fwd", False), ("bwd", True)):
        ref_y, ref_l, ref_s = (torch.from_numpy(z[f"{name}/{d}_{k}"]) for k in ("y", "logj", "sites"))
        ex_y, ex_s, my, ml, ms = _slack(mod64, mod, x64, inverse)
        rel = lambda m, ref: m / ref.abs().clamp(min=1.0)
        by, bl, bs = rel(my, ref_y), rel(ml, ref_l), rel(ms, ref_s)
        with torch.no_grad():
            y, logj = mod.backward(x) if inverse else mod(x)
            y2, logj2 = mod.backward(x, log0=log0) if inverse else mod(x, log0=log0)
            with density:
                y3, sites = mod.backward(x) if inverse else mod(x)
                _, sites0 = mod.backward(x, log0=log0_sites) if inverse else mod(x, log0=log0_sites)
        assert y.shape == x.shape and logj.shape == (B,) and sites.shape == x.shape
        for got in (y, y2, y3):
            assert torch.isfinite(got).all()
            e = _err(got, ref_y)
            assert (e <= tol + by).all(), (d, e.max().item())
        assert torch.equal(y, y2) and torch.equal(y, y3)
        e_l = _err(logj, ref_l)
        assert (e_l <= tol + bl).all(), (d, e_l.max().item())
        e_l0 = _err(logj2, ref_l + log0.double().cpu())
        assert (e_l0 <= tol + bl).all(), (d, e_l0.max().item())
        e_s = _err(sites, ref_s)
        assert (e_s <= tol + bs).all(), (d, e_s.max().item())
        ref_s0 = ref_s + log0_sites.double().cpu()
        assert (_err(sites0, ref_s0) <= tol + bs).all()
        if dtype == torch.float64:          # and against the exact result itself, where the fixture's root is not exact
            assert (_err(y, ex_y) <= tol).all() and (_err(sites, ex_s) <= tol).all()
            assert (_err(logj, ex_s.reshape(B, -1).sum(1)) <= tol).all()
        parity_report(f"pade {name} {str(dtype)[6:]}", f"{d} y/logJ/sites",
                      max((e - by).max().item(), (e_l - bl).max().item(), (e_s - bs).max().item()), tol,
                      "error beyond the rounding slack")


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_round_trip_end_points_and_a_zero(golden, dtype):
    """backward(forward(x)) == x with log J 0; the end points 0 and 1 map to themselves; d0 = 1 (a = 0) stays finite."""
    z = golden("pade")
    for name in NAMES:
        mod = _case_module(z, name, dtype)
        x = torch.from_numpy(z[f"{name}/x"]).to(DEV, dtype)
        with torch.no_grad():
            y, lj = mod(x)
            xb, l0 = mod.backward(y, log0=lj)
            assert torch.isfinite(y).all() and torch.isfinite(lj).all()
            ends = (x == 0) | (x == 1)
            assert torch.equal(y[ends], x[ends])
            tol = 1e-12 if dtype == torch.float64 else 5e-6
            assert (xb - x).abs().max().item() < tol, name
            assert l0.abs().max().item() < tol * x[0].numel(), name
    for name in ('p22_zero', 'p11_zero'):            # the zero-initialised modules are the identity
        mod = _case_module(z, name, dtype)
        x = torch.from_numpy(z[f'{name}/x']).to(DEV, dtype)
        tol = 1e-14 if dtype == torch.float64 else 1e-6
        with torch.no_grad():
            for y, lj in (mod(x), mod.backward(x)):
                assert (y - x).abs().max().item() < tol and lj.abs().max().item() < tol * x[0].numel()


# ---------------------------------------------------------------------------------------------- gradients
def _grad_modules():
    torch.manual_seed(5)
    out = []
    for mod in (Pade11_(), Pade11_(3, 1), Pade11_(3, -1), Pade22_(), Pade22_(3, 1), Pade22_(3, -1),
                Pade22_(3, 1, symmetric=True), Pade22_(symmetric=True)):
        with torch.no_grad():
            for p in mod.parameters():
                p.copy_(1.2 * torch.randn(p.shape))
        out.append(mod.to(DEV, torch.float64))
    return out


def _field(mod, B=5):
    if mod.n_channels == 1 or mod.channels_axis == 1:
        shape = (B, 3, 4, 6)
    else:
        shape = (B, 4, 6, 3)
    return torch.rand(shape, dtype=torch.float64, device=DEV) * 0.98 + 0.01


@pytest.mark.parametrize("per_site", [False, True])
@pytest.mark.parametrize("inverse", [False, True])
def test_gradients_vs_autograd_through_restatement(density, parity_report, inverse, per_site):
    for mod in _grad_modules():
        x = _field(mod)
        gy = torch.randn_like(x)
        gl = torch.randn_like(x) if per_site else torch.randn(x.shape[0], dtype=x.dtype, device=DEV)
        log0 = torch.randn_like(gl)
        # kernel path
        xk = x.clone().requires_grad_(True)
        l0k = log0.clone().requires_grad_(True)
        for p in mod.parameters():
            p.grad = None
        if per_site:
            with density:
                y, lj = mod.backward(xk, log0=l0k) if inverse else mod(xk, log0=l0k)
        else:
            y, lj = mod.backward(xk, log0=l0k) if inverse else mod(xk, log0=l0k)
        ((y * gy).sum() + (lj * gl).sum()).backward()
        got = [xk.grad, l0k.grad] + [p.grad.clone() for p in mod.parameters()]
        # restatement
        xr = x.clone().requires_grad_(True)
        params = list(mod.parameters())
        y_r, s_r = restate(mod, xr, inverse)
        l_r = s_r if per_site else s_r.reshape(x.shape[0], -1).sum(1)
        ref = torch.autograd.grad((y_r * gy).sum() + (l_r * gl).sum(), [xr] + params)
        ref = [ref[0], gl] + list(ref[1:])
        err = max(_err(g, r).max().item() for g, r in zip(got, ref))
        assert err < 1e-10, (type(mod).__name__, mod.n_channels, mod.channels_axis, err)
        parity_report(f"pade grad {type(mod).__name__} C{mod.n_channels} ax{mod.channels_axis}",
                      f"{'inv' if inverse else 'fwd'} {'site' if per_site else 'sample'}", err, 1e-10)


@pytest.mark.parametrize("kind", [_hip.PADE11, _hip.PADE22])
def test_gradcheck_fp64(kind):
    torch.manual_seed(1)
    for inverse in (False, True):
        for per_site in (False, True):
            for layout, shape in (((3, 3, 1, 8), (3, 2, 4)), ((2, 2, 3, 2), (2, 3, 2)), ((2, 12, 3, 1), (2, 3, 2, 3)),
                                  ((3, 1, 3, 4), (3, 4))):          # C = 1; channels axis 1, last, 0 (the batch)
                C = layout[2]
                v = (torch.rand(shape, dtype=torch.float64, device=DEV) * 0.9 + 0.05).requires_grad_(True)
                d0 = (torch.rand(C, dtype=torch.float64, device=DEV) * 2 + 0.3).requires_grad_(True)
                d1 = (torch.rand(C, dtype=torch.float64, device=DEV) * 2 + 0.3).requires_grad_(True)
                if kind == _hip.PADE11:
                    fn = lambda v, d0: _hip.PadeFn.apply(v, d0, None, None, kind, inverse, per_site, layout)
                    args = (v, d0)
                else:
                    fn = lambda v, d0, d1: _hip.PadeFn.apply(v, d0, d1, None, kind, inverse, per_site, layout)
                    args = (v, d0, d1)
                assert torch.autograd.gradcheck(fn, args)


def test_parameter_gradients_are_bitwise_reproducible(density):
    torch.manual_seed(2)
    mod = Pade22_(3, 1).to(DEV, torch.float32)
    with torch.no_grad():
        mod.w0.copy_(torch.tensor([0.3, -0.7, 1.1]))
        mod.w1.copy_(torch.tensor([-0.4, 0.9, 0.2]))
    x = torch.rand((64, 3, 16, 16), dtype=torch.float32, device=DEV)
    grads = []
    for per_site in (False, True, False, True):
        for p in mod.parameters():
            p.grad = None
        if per_site:
            with density:
                y, lj = mod(x)
        else:
            y, lj = mod(x)
        (y.square().sum() + lj.sum()).backward()
        y, lj = mod.backward(y.detach())
        (y.sum() + lj.square().sum()).backward()
        grads.append((per_site, [p.grad.clone() for p in mod.parameters()]))
    for (s0, g0), (s1, g1) in zip(grads[:2], grads[2:]):
        assert s0 == s1 and all(torch.equal(a, b) for a, b in zip(g0, g1))


# ---------------------------------------------------------------------------------------------- training
def test_training_eager_and_graphed_and_sanity_check():
    from normflow__amd.prior import NormalPrior
    from normflow__amd.action import ScalarPhi4Action
    hist, models = [], []
    for graphed in (False, True):
        torch.manual_seed(3)
        model = nf.Model(prior=NormalPrior(shape=(4, 4)), net_=ModuleList_([Expit_(), Pade22_(), Logit_()]),
                         action=ScalarPhi4Action(kappa=0.3, m_sq=-1.0, lambd=0.8))
        torch.manual_seed(9)
        model.fit(n_epochs=8, batch_size=128, hyperparam=dict(lr=0.05, weight_decay=0.0),
                  checkpoint_dict=dict(print_stride=1000, print_batch_size=256), graphed=graphed)
        hist.append(list(model.fit.train_history['loss']))
        models.append(model)
    assert all(math.isfinite(v) for v in hist[0]) and len(hist[0]) == 8
    assert hist[0] == hist[1], (hist[0][-3:], hist[1][-3:])
    pade = models[0].net_[1]
    assert pade.w0.abs().max().item() > 0 and pade.w1.abs().max().item() > 0      # the parameters were trained
    assert torch.equal(pade.w0, models[1].net_[1].w0) and torch.equal(pade.w1, models[1].net_[1].w1)
    (x, y, xb), (lj, l0) = nf.backward_sanitychecker(models[0], return_details=True)
    assert (x - xb).abs().max().item() < 1e-10 and l0.abs().max().item() < 1e-9


# ---------------------------------------------------------------------------------------------- 64-bit indexing
def test_more_than_2_31_elements_fp32():
    """(2^21 + 1, 1024) fp32: 2^31 + 1024 elements (~17 GB with the output).  Values checked at sampled elements,
    the last ones included, and log J of sampled samples, against the fp64 restatement."""
    B, V = 2 ** 21 + 1, 1024
    mod = Pade22_().to(DEV, torch.float32)
    with torch.no_grad():
        mod.w0.fill_(0.6)
        mod.w1.fill_(-0.9)
    g = torch.Generator(device=DEV).manual_seed(4)
    x = torch.rand((B, V), dtype=torch.float32, device=DEV, generator=g)
    assert x.numel() > 2 ** 31
    with torch.no_grad():
        y, lj = mod(x)
    torch.cuda.synchronize()
    idx = torch.cat([torch.randint(0, x.numel(), (200000,), device=DEV, generator=g),
                     torch.arange(x.numel() - 4096, x.numel(), device=DEV)])
    xs = x.reshape(-1)[idx].double()
    ref_y, _ = restate(mod, xs, False)
    assert (_err(y.reshape(-1)[idx], ref_y) <= 2e-6).all()
    rows = torch.cat([torch.randint(0, B, (64,), device=DEV, generator=g), torch.tensor([B - 2, B - 1], device=DEV)])
    _, ref_s = restate(mod, x[rows].double(), False)
    assert (_err(lj[rows], ref_s.sum(1)) <= 2e-6 * 4).all()
    del x, y
    torch.cuda.empty_cache()

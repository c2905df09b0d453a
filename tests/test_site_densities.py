"""Per-site densities on K4 (nf_distconv_sites, nf_distconv_sites_vjp), the reference's nn wrappers and
ScalarPhi4Action.action_density (nf_phi4_action_density and its VJP) on an MI355X.

Values against the reference's outputs (tests/golden/sites.npz); per-site densities summed against the summed K4 pass;
the masked wrapper pass against its generic composition; round trips; gradients against autograd through an fp64
restatement of the chain, and torch.autograd.gradcheck; training eager and graphed; a field of more than 2^31 elements.

Errors are |got - ref| / max(1, |ref|) per element.  fp64: 1e-12, 1e-10 where a spline inverse is involved (the root's
conditioning).  fp32: 2e-6 plus what fp32 rounding moves the exact result by (the stages evaluated in fp32 one by one,
see _rounded_chain; a sample's log J: the sum of its sites' moves), as tests/test_pade.py does."""
import math

import pytest
import torch

import normflow__amd as nf
from normflow__amd import _hip
from normflow__amd.action import ScalarPhi4Action
from normflow__amd.mask import EvenOddMask
from normflow__amd.nn import (Module_, ModuleList_, Expit_, Logit_, SplineNet_, Pade22_, DistConvertor_,
                              InvisibilityMaskWrapperModule_, MultiChannelModule_, MultiOutChannelModule_)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SYM = dict(xlim=(0.5, 1), ylim=(0.5, 1), extrap={'left': 'anti'})


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


def _err(got, ref):
    got, ref = got.detach().double().cpu(), torch.as_tensor(ref).double().cpu()
    return (got - ref).abs() / ref.abs().clamp(min=1.0)


def _state(z, pre):
    return {k[len(pre) + 6:]: torch.from_numpy(z[k]) for k in z.files if k.startswith(pre + "state/")}


LEAVES = {'expit': lambda: Expit_(), 'logit': lambda: Logit_(), 'spline': lambda: SplineNet_(6),
          'spline_sym': lambda: SplineNet_(6, **SYM), 'dc': lambda: DistConvertor_(6),
          'dc_sym': lambda: DistConvertor_(6, symmetric=True)}


def _leaf(z, name, dtype):
    mod = LEAVES[name]()
    mod.load_state_dict(_state(z, f"leaf/{name}/"))
    return _to(mod, dtype)


def _to(mod, dtype):
    for p in mod.parameters():
        p.data = p.data.to(DEV, dtype)
    return mod


def _knots_and_stages(mod, inverse):
    """The K4 description of a leaf or of a DistConvertor_ triple."""
    if isinstance(mod, DistConvertor_):
        return 7, inverse, mod.spline_layer_.knots()
    stages, inv, knots = mod._k4(inverse)
    return stages, inv, knots


def _rounded_chain(v, knots, stages, inverse):
    """The chain stage by stage, each stage evaluated in fp32 on its own (input, knots and every intermediate value
    rounded to fp32, each stage's own fp32 arithmetic): (value, per-site log J, sum of the stages' |log J| terms, whose
    fp32 roundings the fused kernel's sum carries).  Its distance from the exact result is the slack: the fused kernel
    may add 2e-6 to what evaluating its stages in fp32 one by one moves the result by."""
    acc, terms = torch.zeros_like(v), torch.zeros_like(v)
    for bit in ((4, 2, 1) if inverse else (1, 2, 4)):
        if stages & bit:
            v, s = _hip.DistConvSitesFn.apply(v.float(), knots if bit == 2 else None, None, None, bit, inverse, True)
            v, s = v.double(), s.double()
            acc, terms = acc + s, terms + s.abs()
    return v, acc, terms


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("name", list(LEAVES))
def test_leaves_vs_reference(golden, density, parity_report, name, dtype):
    """Per sample and per site, forward and backward, with and without log0; the class flag and the instance flag."""
    z = golden("sites")
    pre = f"leaf/{name}/"
    mod = _leaf(z, name, dtype)
    spline = name != 'expit' and name != 'logit'
    for d, inverse in (("fwd", False), ("bwd", True)):
        x64 = torch.from_numpy(z[pre + d + "_x"])
        x = x64.to(DEV, dtype)
        B = x.shape[0]
        ref_y, ref_l, ref_s = (torch.from_numpy(z[pre + d + k]) for k in ("_y", "_logj", "_sites"))
        tol = (1e-10 if spline and inverse else 1e-12) if dtype == torch.float64 else 2e-6
        if dtype == torch.float32:
            mod64 = _leaf(z, name, torch.float64)
            stages, inv, knots32 = _knots_and_stages(mod, inverse)
            _, _, knots64 = _knots_and_stages(mod64, inverse)
            with torch.no_grad():
                v = x64.to(DEV).reshape(B, -1)
                e_y, e_s = _hip.DistConvSitesFn.apply(v, knots64, None, None, stages, inv, True)
                r_y, r_s, r_t = _rounded_chain(v, knots32, stages, inv)
            my = (r_y - e_y).abs().reshape(x.shape).cpu()
            ms = ((r_s - e_s).abs() + 6e-8 * r_t).reshape(x.shape).cpu()
        else:
            my = ms = torch.zeros(x.shape, dtype=torch.float64, device='cpu')
        ml = ms.reshape(B, -1).sum(1)
        rel = lambda m, ref: m / ref.abs().clamp(min=1.0)
        by, bl, bs = rel(my, ref_y), rel(ml, ref_l), rel(ms, ref_s)
        log0 = torch.linspace(-1.0, 2.0, B, dtype=dtype, device=DEV)
        log0_sites = log0.reshape((B,) + (1,) * (x.dim() - 1)).expand(x.shape).contiguous()
        with torch.no_grad():
            y, logj = mod.backward(x) if inverse else mod(x)
            with density:
                y2, sites = mod.backward(x) if inverse else mod(x)
                _, sites0 = mod.backward(x, log0=log0_sites) if inverse else mod(x, log0=log0_sites)
        assert logj.shape == (B,) and sites.shape == x.shape and y2.shape == x.shape
        assert (_err(y2, y) <= (0 if dtype == torch.float64 else 1e-6)).all()     # two kernel instances
        e_y, e_l, e_s = _err(y, ref_y), _err(logj, ref_l), _err(sites, ref_s)
        assert (e_y <= tol + by).all(), (d, e_y.max().item())
        assert (e_l <= tol + bl).all(), (d, e_l.max().item())
        assert (e_s <= tol + bs).all(), (d, e_s.max().item())
        assert (_err(sites0, ref_s + log0_sites.double().cpu()) <= tol + bs).all()
        if not isinstance(mod, ModuleList_):                # the instance flag, in both directions
            mod.propagate_density = True
            try:
                with torch.no_grad():
                    y3, sites3 = mod.backward(x) if inverse else mod(x)
            finally:
                del mod.propagate_density
            assert torch.equal(y3, y2) and torch.equal(sites3, sites)
        parity_report(f"sites {name} {str(dtype)[6:]}", f"{d} y/logJ/sites",
                      max((e_y - by).max().item(), (e_l - bl).max().item(), (e_s - bs).max().item()), tol,
                      "error beyond the rounding slack")


def test_site_sums_equal_the_summed_pass(density):
    """fp64: per-site densities summed per sample == the existing summed K4 pass (nf_distconv) within 1e-12."""
    torch.manual_seed(11)
    for make in (lambda: SplineNet_(8), lambda: SplineNet_(8, **SYM), Expit_, Logit_, lambda: DistConvertor_(8),
                 lambda: DistConvertor_(8, symmetric=True)):
        mod = make()
        with torch.no_grad():
            for p in mod.parameters():
                p.copy_(0.7 * torch.randn(p.shape))
        mod = _to(mod, torch.float64)
        for inverse in (False, True):
            unit = (isinstance(mod, SplineNet_) or (isinstance(mod, Logit_) and not inverse)
                    or (isinstance(mod, Expit_) and inverse))
            x = (torch.rand(5, 6, 7, dtype=torch.float64, device=DEV) * 0.96 + 0.02 if unit
                 else torch.randn(5, 6, 7, dtype=torch.float64, device=DEV) * 2)
            with torch.no_grad():
                y, logj = mod.backward(x) if inverse else mod(x)
                with density:
                    y2, sites = mod.backward(x) if inverse else mod(x)
            assert (_err(y2, y) <= 1e-15).all()
            assert (_err(sites.reshape(5, -1).sum(1), logj) <= 1e-12).all(), (type(mod).__name__, inverse)


def test_distconvertor_mixed_flags_run_stage_by_stage(golden):
    z = golden("sites")
    mod = _leaf(z, 'dc', torch.float64)
    assert [k for k, _ in mod._steps()] == ['fused']
    mod[1].propagate_density = True
    assert [k for k, _ in mod._steps()] == ['single'] * 3
    x = torch.from_numpy(z["leaf/dc/fwd_x"]).to(DEV)
    for m in mod:
        m.propagate_density = True
    with torch.no_grad():
        y, s = mod(x)
    for m in mod:
        del m.propagate_density
    assert [k for k, _ in mod._steps()] == ['fused']
    assert (_err(y, z["leaf/dc/fwd_y"]) <= 1e-12).all() and (_err(s, z["leaf/dc/fwd_sites"]) <= 1e-12).all()


def test_round_trips(density):
    torch.manual_seed(12)
    mask = EvenOddMask(shape=(6, 7))
    for make in (lambda: SplineNet_(8), lambda: SplineNet_(8, **SYM), lambda: DistConvertor_(8)):
        for dtype, tol in ((torch.float64, 1e-10), (torch.float32, 1e-4)):
            mod = make()
            with torch.no_grad():
                for p in mod.parameters():
                    p.copy_(0.7 * torch.randn(p.shape))
            mod = _to(mod, dtype)
            x = torch.rand(4, 6, 7, dtype=dtype, device=DEV) * 0.96 + 0.02
            if isinstance(mod, DistConvertor_):
                x = torch.logit(x)
            with torch.no_grad():
                with density:
                    y, s = mod(x)
                    xb, s0 = mod.backward(y, log0=s)
                assert (xb - x).abs().max().item() < tol and s0.abs().max().item() < tol
                if isinstance(mod, SplineNet_):
                    wrap = InvisibilityMaskWrapperModule_(mod, mask=mask)
                    y, lj = wrap(x)
                    xb, l0 = wrap.backward(y, log0=lj)
                    assert (xb - x).abs().max().item() < tol and l0.abs().max().item() < tol * 42


# ---------------------------------------------------------------------------------------------- the wrappers
def _mask(z):
    mask = EvenOddMask(shape=tuple(z["mask"].shape))
    assert torch.equal(mask._mask.cpu(), torch.from_numpy(z["mask"]))
    return mask.to(DEV)


def _generic(wrap, x, log0, inverse):
    """The reference's composition (src/nn/_core.py:219-231), spelled out."""
    m = wrap.mask
    x_v, x_inv = m.split(x)
    x_v, dens = wrap.net_.backward(x_v) if inverse else wrap.net_.forward(x_v)
    lj = wrap.sum_density(m.purify(dens, channel=0))
    return m.cat(m.purify(x_v, channel=0), x_inv), log0 + lj


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("name", ['spline', 'pade22', 'expit', 'logit'])
def test_wrapper_vs_reference_and_generic_composition(golden, parity_report, name, dtype):
    z = golden("sites")
    pre = f"wrap/{name}/"
    leaf = {'spline': lambda: SplineNet_(6), 'pade22': lambda: Pade22_(), 'expit': Expit_, 'logit': Logit_}[name]()
    leaf.load_state_dict(_state(z, pre))
    leaf = leaf.to(DEV, dtype)
    wrap = InvisibilityMaskWrapperModule_(leaf, mask=_mask(z))
    assert leaf.propagate_density is True and wrap.label == f"wrapper:{leaf.label}"
    visible = torch.from_numpy(z["mask"]).bool()
    tol = 1e-10 if dtype == torch.float64 else 2e-5
    for d, inverse in (("fwd", False), ("bwd", True)):
        if pre + d + "_x" not in z.files:
            continue
        x = torch.from_numpy(z[pre + d + "_x"]).to(DEV, dtype)
        for tag, flag in (("sum", False), ("sites", True)):
            wrap.propagate_density = flag
            ref_y, ref_l = torch.from_numpy(z[pre + d + f"_{tag}_y"]), torch.from_numpy(z[pre + d + f"_{tag}_logj"])
            with torch.no_grad():
                y, lj = wrap.backward(x) if inverse else wrap(x)
                k4 = wrap._activity(x) is not None
                assert k4 == (name != 'pade22')
            assert lj.shape == ref_l.shape
            if name == 'logit':
                # the reference evaluates log(0) * 0 at the invisible sites: NaN there (and in every sum); here those
                # sites are copied, and equal to the reference wherever it is finite
                assert torch.isfinite(y).all() and torch.isfinite(lj).all()
                inv = ~visible.expand(y.shape)
                assert torch.equal(y.cpu()[inv], x.cpu()[inv])
                fin = torch.isfinite(ref_y)
                assert torch.equal(fin, ~inv)
                assert (_err(y.cpu()[fin], ref_y[fin]) <= tol).all()
                if flag:
                    assert (_err(lj.cpu()[fin], ref_l[fin]) <= tol).all() and (lj.cpu()[inv] == 0).all()
                else:
                    assert not torch.isfinite(ref_l).any()
                continue
            e_y, e_l = _err(y, ref_y), _err(lj, ref_l)
            assert (e_y <= tol).all() and (e_l <= tol * (1 if flag else 12)).all(), (d, tag, e_y.max(), e_l.max())
            # the masked pass equals its generic composition
            with torch.no_grad():
                gy, gl = _generic(wrap, x, 0, inverse)
            assert (_err(y, gy) <= (1e-12 if dtype == torch.float64 else 1e-6)).all()
            assert (_err(lj, gl) <= (1e-12 if dtype == torch.float64 else 1e-5)).all()
            parity_report(f"wrap {name} {str(dtype)[6:]}", f"{d} {tag}", max(e_y.max().item(), e_l.max().item()), tol)
    wrap.propagate_density = False


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_multichannel_modules_vs_reference(golden, dtype):
    z = golden("sites")
    tol = 1e-10 if dtype == torch.float64 else 2e-5
    for pre, make in (("multi/keep/", lambda: MultiChannelModule_([SplineNet_(5), Pade22_()], keep_channels_axis=True)),
                      ("multi/drop/", lambda: MultiChannelModule_([SplineNet_(5), Pade22_()], keep_channels_axis=False)),
                      ("multiout/", lambda: MultiOutChannelModule_([SplineNet_(5), Pade22_()]))):
        mod = make()
        state = _state(z, pre)
        assert set(mod.state_dict()) == set(state)
        mod.load_state_dict(state)
        assert mod.npar == sum(v.numel() for v in state.values())
        mod = mod.to(DEV, dtype)
        x = torch.from_numpy(z[pre + "x"]).to(DEV, dtype)
        for d, inverse in (("fwd", False), ("bwd", True)):
            with torch.no_grad():
                y, lj = mod.backward(x) if inverse else mod(x)
            assert y.shape == z[pre + d + "_y"].shape and lj.shape == z[pre + d + "_logj"].shape
            assert (_err(y, z[pre + d + "_y"]) <= tol).all() and (_err(lj, z[pre + d + "_logj"]) <= tol * 24).all()


# ---------------------------------------------------------------------------------------------- gradients
def _chain(x, knots, stages, inverse):
    """fp64 torch restatement of the K4 chain (modules_.py:93-114, spline.py:185-287): (value, per-site log|f'|)."""
    pre, post = (stages & 4, stages & 1) if inverse else (stages & 1, stages & 4)
    u, lg = x, torch.zeros_like(x)
    if pre:
        u = torch.sigmoid(x)
        lg = lg + torch.log(u * (1 - u))
    if stages & 2:
        kx, ky, kd = knots[0], knots[1], knots[2]
        K = kx.shape[0]
        key = ky if inverse else kx
        j = (torch.searchsorted(key.detach().contiguous(), u.detach().reshape(-1).contiguous()) - 1).clamp(0, K - 2)
        j = j.reshape(u.shape)
        x0, x1, y0, y1, d0, d1 = kx[j], kx[j + 1], ky[j], ky[j + 1], kd[j], kd[j + 1]
        bw, bh = x1 - x0, y1 - y0
        sl = bh / bw
        curv = d0 + d1 - 2 * sl
        if not inverse:
            th = (u - x0) / bw
        else:
            eta = (u - y0) / bh
            a2 = -curv * eta + d0 - sl
            bb = a2 + sl
            a0 = sl * eta
            disc = torch.sqrt((bb * bb - 4 * a0 * a2).clamp(min=0))
            pos = bb >= 0
            th = torch.where(pos, 2 * a0 / torch.where(pos, bb + disc, 1.0),
                             (bb - disc) / (2 * torch.where(pos, 1.0, a2)))
        om = 1 - th
        t1 = th * om
        den = sl + curv * t1
        P = d1 * th * th + 2 * sl * t1 + d0 * om * om
        lgs = torch.log(sl * sl * P / (den * den))
        if not inverse:
            u, lg = y0 + bh * (sl * th * th + d0 * t1) / den, lg + lgs
        else:
            u, lg = x0 + bw * th, lg - lgs
    if post:
        lg = lg - torch.log(u * (1 - u))
        u = torch.log(u / (1 - u))
    return u, lg


def _grad_knots():
    torch.manual_seed(21)
    out = []
    for kw in ({}, SYM):
        s = SplineNet_(7, **kw)
        with torch.no_grad():
            for p in s.parameters():
                p.copy_(0.8 * torch.randn(p.shape))
        out.append(_to(s, torch.float64).knots().detach())
    return out


def _inputs(stages, inverse, shape):
    real_in = (stages & 4) if inverse else (stages & 1)
    if real_in:
        return torch.randn(shape, dtype=torch.float64, device=DEV) * 2
    return torch.rand(shape, dtype=torch.float64, device=DEV) * 0.96 + 0.02


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("per_site", [False, True])
@pytest.mark.parametrize("inverse", [False, True])
def test_sites_vjp_vs_autograd_through_restatement(parity_report, inverse, per_site, masked):
    B, V = 4, 45
    act = (torch.arange(V, device=DEV) % 3 != 1).to(torch.uint8) if masked else None
    worst = 0.0
    for knots in _grad_knots():
        for stages in (1, 2, 4, 3, 6, 7):
            x = _inputs(stages, inverse, (B, V))
            gy = torch.randn_like(x)
            gl = torch.randn_like(x) if per_site else torch.randn(B, dtype=x.dtype, device=DEV)
            log0 = torch.randn_like(gl)
            xk, kk, l0k = (t.clone().requires_grad_(True) for t in (x, knots, log0))
            kin = kk if stages & 2 else None
            y, dens = _hip.DistConvSitesFn.apply(xk, kin, l0k, act, stages, inverse, per_site)
            ((y * gy).sum() + (dens * gl).sum()).backward()
            got = [xk.grad, l0k.grad] + ([kk.grad] if stages & 2 else [])
            xr, kr = x.clone().requires_grad_(True), knots.clone().requires_grad_(True)
            on = act.bool().expand(B, V) if masked else torch.ones(B, V, dtype=torch.bool, device=DEV)
            safe = torch.where(on, xr, torch.full_like(xr, 0.5))
            u, lg = _chain(safe, kr, stages, inverse)
            y_r = torch.where(on, u, xr)
            s_r = torch.where(on, lg, torch.zeros_like(lg))
            d_r = s_r if per_site else s_r.sum(1)
            ref = torch.autograd.grad((y_r * gy).sum() + (d_r * gl).sum(), [xr, kr], allow_unused=True)
            refs = [ref[0], gl] + ([ref[1]] if stages & 2 else [])
            assert torch.allclose(y.detach(), y_r.detach(), rtol=1e-10, atol=1e-10)
            err = max(_err(g, r).max().item() for g, r in zip(got, refs))
            assert err < 1e-10, (stages, inverse, per_site, masked, err)
            worst = max(worst, err)
    parity_report("distconv sites vjp", f"{'inv' if inverse else 'fwd'} {'site' if per_site else 'sum'}"
                  f"{' mask' if masked else ''}", worst, 1e-10)


def test_gradcheck_fp64():
    torch.manual_seed(22)
    knots = _grad_knots()[1].clone()
    act = (torch.arange(10, device=DEV) % 2).to(torch.uint8)
    for inverse in (False, True):
        for per_site in (False, True):
            for mask in (None, act):
                for stages in (7, 2):
                    x = _inputs(stages, inverse, (3, 10)).requires_grad_(True)
                    k = knots.clone().requires_grad_(True)
                    fn = lambda x, k: _hip.DistConvSitesFn.apply(x, k, None, mask, stages, inverse, per_site)
                    assert torch.autograd.gradcheck(fn, (x, k))


# ---------------------------------------------------------------------------------------------- action density
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_action_density_vs_reference_and_action(golden, dtype):
    z = golden("sites")
    m_sq, lambd, kappa, a = (float(v) for v in z["action/coef"])
    act = ScalarPhi4Action(m_sq=m_sq, lambd=lambd, kappa=kappa, a=a)
    tol = 1e-12 if dtype == torch.float64 else 2e-6
    for name in ("d1", "d2", "d3", "d4"):
        x = torch.from_numpy(z[f"action/{name}/x"]).to(DEV, dtype)
        with torch.no_grad():
            dens = act.action_density(x)
            tot = act.action(x)
        assert dens.shape == x.shape and dens.dtype == dtype
        n = x[0].numel()
        assert (_err(dens, z[f"action/{name}/density"]) <= tol * 4).all(), name
        assert (_err(dens.double().reshape(x.shape[0], -1).sum(1), z[f"action/{name}/action"]) <= tol * n).all()
        assert (_err(dens.double().reshape(x.shape[0], -1).sum(1), tot) <= tol * n).all()


def test_action_density_vjp_and_gradcheck():
    torch.manual_seed(23)
    act = ScalarPhi4Action(m_sq=-0.9, lambd=0.5, kappa=0.7, a=1.2)
    for shape in ((3, 9), (2, 4, 5), (2, 2, 3, 4), (2, 3, 2, 4, 5), (2, 1, 4, 3)):
        x = torch.randn(shape, dtype=torch.float64, device=DEV)
        g = torch.randn_like(x)
        xk = x.clone().requires_grad_(True)
        (act.action_density(xk) * g).sum().backward()
        xr = x.cpu().clone().requires_grad_(True)
        (act.action_density(xr) * g.cpu()).sum().backward()          # host restatement
        assert (_err(xk.grad, xr.grad) <= 1e-10).all(), shape
        assert torch.autograd.gradcheck(lambda t: act.action_density(t), (x.clone().requires_grad_(True),))


# ---------------------------------------------------------------------------------------------- training
def test_training_eager_and_graphed_with_a_wrapped_spline():
    """A flow whose net_ holds a wrapped SplineNet_: its masked sum pass and VJP in training, eager and graphed.  The
    knot gradients keep the LDS double atomics of nf_distconv_vjp, so the two loss histories may differ by fp32
    rounding only."""
    from normflow__amd.prior import NormalPrior
    hist, models = [], []
    for graphed in (False, True):
        torch.manual_seed(3)
        mask = EvenOddMask(shape=(4, 4))
        net_ = ModuleList_([Expit_(), InvisibilityMaskWrapperModule_(SplineNet_(6), mask=mask), Logit_()])
        model = nf.Model(prior=NormalPrior(shape=(4, 4)), net_=net_,
                         action=ScalarPhi4Action(kappa=0.3, m_sq=-1.0, lambd=0.8))
        torch.manual_seed(9)
        model.fit(n_epochs=8, batch_size=128, hyperparam=dict(lr=0.05, weight_decay=0.0),
                  checkpoint_dict=dict(print_stride=1000, print_batch_size=256), graphed=graphed)
        hist.append(list(model.fit.train_history['loss']))
        models.append(model)
    assert all(math.isfinite(v) for v in hist[0]) and len(hist[0]) == 8 == len(hist[1])
    for a, b in zip(*hist):
        assert abs(a - b) <= 1e-6 * max(1.0, abs(a)), (hist[0], hist[1])
    spline = models[0].net_[1].net_
    assert spline.weights_x.abs().max().item() > 0           # the knots were trained
    (x, y, xb), (lj, l0) = nf.backward_sanitychecker(models[0], return_details=True)
    assert (x - xb).abs().max().item() < 1e-4 and l0.abs().max().item() < 1e-3


# ---------------------------------------------------------------------------------------------- 64-bit indexing
def test_more_than_2_31_elements_per_site_fp32():
    """(2^21 + 1, 1024) fp32 through the per-site SplineNet_ pass: 2^31 + 1024 elements (~26 GB with the outputs).
    Values and densities checked at sampled elements, the last ones included, against the fp64 restatement."""
    B, V = 2 ** 21 + 1, 1024
    torch.manual_seed(24)
    s = SplineNet_(8)
    with torch.no_grad():
        for p in s.parameters():
            p.copy_(0.7 * torch.randn(p.shape))
    s = s.to(DEV, torch.float32)
    s.propagate_density = True
    g = torch.Generator(device=DEV).manual_seed(4)
    x = torch.rand((B, V), dtype=torch.float32, device=DEV, generator=g)
    assert x.numel() > 2 ** 31
    with torch.no_grad():
        y, sites = s(x)
    torch.cuda.synchronize()
    idx = torch.cat([torch.randint(0, x.numel(), (200000,), device=DEV, generator=g),
                     torch.arange(x.numel() - 4096, x.numel(), device=DEV)])
    xs = x.reshape(-1)[idx].double()
    ref_y, ref_s = _chain(xs, s.knots().detach().double(), 2, False)
    assert (_err(y.reshape(-1)[idx], ref_y) <= 2e-5).all()
    assert (_err(sites.reshape(-1)[idx], ref_s) <= 2e-5).all()
    del x, y, sites
    torch.cuda.empty_cache()

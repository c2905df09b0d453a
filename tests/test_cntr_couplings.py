"""The controlled couplings on an MI355X: the reference's outputs replayed (tests/golden/cntr.npz), and every path an atom
can take held to the CPU oracle with a control that is non-zero on ALL sites -- the active sites of the first atom
included, whose control values the reference's net convolves like any others.

The oracle of a controlled block is composed here from oracle/nf_oracle.py: `O.conv_act` on the control for net 0, on the
frozen half for the others, then the ordinary coupling atoms.

Bounds.  fp64 against the fixture: 1e-9 (what DESIGN.md quotes for atoms.npz in fp64).  fp32 against the fixture: 1e-5
for the values and log J of shift and affine blocks and 2e-4 for gradients, the base bounds of
test_gpu_parity.test_coupling_blocks_with_convact_against_goldens; the fp32 spline is held atom by atom to the per-site
conditioned bound of tests/cond_bound.py, on the logits its own net produced (themselves held to the oracle's at 1e-5).
Fused fp32 paths against the oracle: 1e-5 relative for values and log J (smoke()), 2e-4 of each gradient's largest entry
(test_fused_last_layer_spline_vjp_vs_autograd_through_oracle)."""
import numpy as np
import pytest
import torch

import cond_bound as CB
from normflow__amd import _hip
from normflow__amd.mask import EvenOddMask
from normflow__amd.nn import (ConvAct, ModuleList_, AffineCoupling_, DirectCntrCoupling_, CntrShiftCoupling_,
                              CntrAffineCoupling_, CntrRQSplineCoupling_, CntrMultiRQSplineCoupling_)
from normflow__amd.nn.scalar.couplings_ import set_training_fusion
from oracle import nf_oracle as O

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
LIN = {'left': 'linear', 'right': 'linear'}
LIM3 = dict(xlim=(-3.0, 3.0), ylim=(-3.0, 3.0), extrap=LIN)
LIM5 = dict(xlim=(-5.0, 5.0), ylim=(-5.0, 5.0), extrap=LIN)
CLS = {'shift': CntrShiftCoupling_, 'affine': CntrAffineCoupling_, 'rqs': CntrRQSplineCoupling_}
ATOM = {'shift': O.shift_coupling_atom, 'affine': O.affine_coupling_atom, 'rqs': O.rqs_coupling_atom,
        'multirqs': O.multi_rqs_coupling_atom}


def T(a, dtype=torch.float64, dev=None):
    return torch.from_numpy(np.asarray(a)).to(device=dev or DEV, dtype=dtype)


def rel(a, b):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max()) / max(1.0, float(b.abs().max()))


class Generator:
    """A control generator that hands out one tensor and counts its calls."""

    def __init__(self, control):
        self.control, self.calls = control, []

    def __call__(self, batch_size):
        self.calls.append(batch_size)
        assert self.control.shape[0] == batch_size
        return self.control


# ---------------------------------------------------------------------------------------------- the oracle, composed
def oracle_leaves(cpl):
    """The block's parameters as fp64 CPU leaves (by name) and its nets as oracle callables built on them (a Conv4d keeps
    its weight in the reference's lower-dimensional layout)."""
    leaves = {n: p.detach().double().cpu().requires_grad_(True) for n, p in cpl.named_parameters()}
    nets = []
    for i, net in enumerate(cpl.nets):
        layers, acts = [], []
        for j, mod in enumerate(net):
            pre = f"nets.{i}.{j}."
            if pre + "_conv_lower_dim.weight" in leaves:
                w = O.conv4d_standard_weight(leaves[pre + "_conv_lower_dim.weight"], mod.out_channels, mod.kernel_size[0])
            elif pre + "weight" in leaves:
                w = leaves[pre + "weight"]
            else:
                acts[-1] = {'Tanh': 'tanh'}[type(mod).__name__]
                continue
            layers.append((w, leaves.get(pre + "bias")))
            acts.append(None)
        nets.append(lambda t, layers=layers, acts=acts: O.conv_act(t, layers, acts))
    return leaves, nets


def oracle_block(x, control, nets, kind, shape, *, inverse=False, log0=0, trace=None, **opts):
    """`O.coupling_block` with `control` as net 0's input (control=None: the ordinary block).  `trace` collects every atom's
    (k, parity, active part, net input, logits)."""
    masks = [O.channel_mask(shape, c, dtype=x.dtype) for c in (0, 1)]
    parts = [x * masks[0], x * masks[1]]
    order = range(len(nets))
    for k in (reversed(order) if inverse else order):
        p = k % 2
        frozen = control if (k == 0 and control is not None) else parts[1 - p]
        out = nets[k](frozen if kind == 'multirqs' else frozen.unsqueeze(1))
        if trace is not None:
            trace.append((k, p, parts[p], frozen, out))
        parts[p], log0 = ATOM[kind](parts[p], out, masks[p], inverse=inverse, log0=log0, **opts)
    return parts[0] + parts[1], log0


def make_block(kind, shape, hidden, m, dtype, control, n_nets=2, seed=0, lim=LIM5, cls=None):
    torch.manual_seed(seed)
    n_out = {'shift': 1, 'affine': 2, 'rqs': 3 * m - 2}[kind]
    acts = ['tanh'] * len(hidden) + [None]
    nets = [ConvAct(1, n_out, 3, conv_dim=len(shape), hidden_sizes=list(hidden), acts=acts) for _ in range(n_nets)]
    with torch.no_grad():       # tame the randn-initialised biases of the last layer: well-conditioned splines
        for net in nets:
            for p in list(net.parameters())[-2:]:
                p.mul_(0.3)
    gen = Generator(control)
    kw = dict(lim) if kind == 'rqs' else {}
    cpl = (cls or CLS[kind])(nets, mask=EvenOddMask(shape=shape), control_generator=gen, **kw)
    return cpl.to(device=DEV, dtype=dtype), gen, kw


def active_bump(control, shape, amount=0.7):
    """The control with `amount` added on the active sites of the first atom (parity 0) only."""
    act = O.channel_mask(shape, 0, dtype=torch.float64).to(control.device, control.dtype)
    return control + amount * act


# ---------------------------------------------------------------------------------------------- the fixture, replayed
def _load(z, tag, kind, d, shape, dtype):
    n_out = {'shift': 1, 'affine': 2, 'rqs': 13}[kind]
    nets = [ConvAct(1, n_out, 3, conv_dim=d, hidden_sizes=[4], acts=['tanh', None]) for _ in range(3)]
    gen = Generator(T(z[f"{tag}/control"]))              # handed over in fp64: the block casts it to the field's dtype
    cpl = CLS[kind](nets, mask=EvenOddMask(shape=shape), control_generator=gen, **(LIM3 if kind == 'rqs' else {}))
    sd = {k.split("/param/")[1]: torch.from_numpy(z[k]) for k in z.files if k.startswith(f"{tag}/param/")}
    missing, unexpected = cpl.load_state_dict(sd, strict=False)
    assert not unexpected and set(missing) <= {"mask._mask", "mask._c_mask"}
    return cpl.to(device=DEV, dtype=dtype), gen


@pytest.mark.parametrize("d", [2, 4])
@pytest.mark.parametrize("kind", ["shift", "affine", "rqs"])
def test_fixture_fp64(golden, parity_report, kind, d):
    z = golden("cntr")
    tag = f"{kind}/d{d}"
    shape = tuple(int(v) for v in z[f"{tag}/shape"])
    cpl, gen = _load(z, tag, kind, d, shape, torch.float64)
    x = T(z[f"{tag}/x"]).requires_grad_(True)
    y, logJ = cpl(x)
    if not torch.is_tensor(logJ):
        assert kind == 'shift' and logJ == 0
        logJ = torch.zeros(x.shape[0], dtype=x.dtype, device=DEV)
    errs = {'y': rel(y, z[f"{tag}/y"]), 'logJ': rel(logJ, z[f"{tag}/logJ"])}
    names = [n for n, _ in cpl.named_parameters()]
    grads = torch.autograd.grad((y ** 2).mean() + logJ.mean(), [x] + [p for _, p in cpl.named_parameters()],
                                allow_unused=True)
    errs['grad_x'] = rel(grads[0], z[f"{tag}/grad_x"])
    for n, gp in zip(names, grads[1:]):
        errs[f'g/{n}'] = rel(gp if gp is not None else torch.zeros(1), z[f"{tag}/gparam/{n}"])
    assert gen.calls == [3] and cpl.control is gen.control
    with torch.no_grad():
        if kind != 'rqs':
            xh, lrt = cpl.backward(T(z[f"{tag}/y"]), T(z[f"{tag}/logJ"]))
            errs['xhat'], errs['logJ_rt'] = rel(xh, z[f"{tag}/xhat"]), rel(lrt, z[f"{tag}/logJ_rt"])
        else:           # the package's own round trip, forward-residual form (the reference's spline inverse is not a fixture)
            xh, lrt = cpl.backward(y.detach(), logJ.detach())
            y2, _ = cpl(xh)
            errs['roundtrip y'], errs['roundtrip logJ'] = rel(y2, y), float(lrt.abs().max())
            assert rel(xh, x) <= 1e-6
    worst = max(errs, key=errs.get)
    parity_report(f"cntr {tag} fp64", f"worst: {worst}", errs[worst], 1e-9)
    assert errs[worst] <= 1e-9, errs
    assert len(gen.calls) == (1 if kind != 'rqs' else 2)           # backward never calls the generator


@pytest.mark.parametrize("d", [2, 4])
@pytest.mark.parametrize("kind", ["shift", "affine"])
def test_fixture_fp32_shift_affine(golden, parity_report, kind, d):
    z = golden("cntr")
    tag = f"{kind}/d{d}"
    shape = tuple(int(v) for v in z[f"{tag}/shape"])
    cpl, gen = _load(z, tag, kind, d, shape, torch.float32)
    x = T(z[f"{tag}/x"], torch.float32).requires_grad_(True)
    y, logJ = cpl(x)
    if not torch.is_tensor(logJ):
        logJ = torch.zeros(x.shape[0], dtype=x.dtype, device=DEV)
    assert y.dtype == torch.float32
    ey, el = rel(y, z[f"{tag}/y"]), rel(logJ, z[f"{tag}/logJ"])
    parity_report(f"cntr {tag} fp32", "y / logJ", max(ey, el), 1e-5)
    assert ey <= 1e-5 and el <= 1e-5, (ey, el)
    names = [n for n, _ in cpl.named_parameters()]
    grads = torch.autograd.grad((y ** 2).mean() + logJ.mean(), [x] + [p for _, p in cpl.named_parameters()],
                                allow_unused=True)
    eg = max([rel(grads[0], z[f"{tag}/grad_x"])] +
             [rel(gp if gp is not None else torch.zeros(1), z[f"{tag}/gparam/{n}"]) for n, gp in zip(names, grads[1:])])
    parity_report(f"cntr {tag} fp32", "gradients", eg, 2e-4)
    assert eg <= 2e-4, eg
    with torch.no_grad():
        xh, lrt = cpl.backward(T(z[f"{tag}/y"], torch.float32), T(z[f"{tag}/logJ"], torch.float32))
    assert rel(xh, z[f"{tag}/xhat"]) <= 1e-5 and rel(lrt, z[f"{tag}/logJ_rt"]) <= 1e-5


@pytest.mark.parametrize("d", [2, 4])
def test_fixture_fp32_spline_atoms_vs_conditioned_bound(golden, parity_report, d):
    """The fp32 spline block, atom by atom on the fp64 trajectory of the fixture: the logits of each atom's own net against
    the oracle's conv (1e-5), and the atom's values and log J against the per-site conditioned bound on those logits."""
    z = golden("cntr")
    tag = f"rqs/d{d}"
    shape = tuple(int(v) for v in z[f"{tag}/shape"])
    cpl, gen = _load(z, tag, 'rqs', d, shape, torch.float32)
    cpl64, _ = _load(z, tag, 'rqs', d, shape, torch.float64)
    _, onets = oracle_leaves(cpl64)
    trace = []
    with torch.no_grad():
        yo, lo = oracle_block(T(z[f"{tag}/x"], dev='cpu'), T(z[f"{tag}/control"], dev='cpu'), onets, 'rqs', shape,
                              trace=trace, **LIM3)
    assert rel(yo, z[f"{tag}/y"]) <= 1e-9 and rel(lo, z[f"{tag}/logJ"]) <= 1e-9         # the composed oracle is the reference
    for k, p, xa64, xf64, out64 in trace:
        xa, xf = xa64.to(DEV, torch.float32), xf64.to(DEV, torch.float32)
        with torch.no_grad():
            out32 = cpl.nets[k](xf.unsqueeze(1))
            val, lj = cpl.atomic_forward(x_active=xa, x_frozen=xf, parity=p, net=cpl.nets[k], log0=0)
        assert rel(out32, out64) <= 1e-5, (k, rel(out32, out64))
        act = O.channel_mask(shape, p, dtype=torch.float64).bool().reshape(-1)
        B = xa.shape[0]
        xs = xa.double().cpu().reshape(B, -1)[:, act]                                          # what the kernel was given
        logits = out32.double().cpu().reshape(B, out32.shape[1], -1)[:, :, act]
        y_ref, logg, b_y, b_l = CB.rqs_forward_bound(xs.reshape(-1), logits.permute(0, 2, 1).reshape(-1, out32.shape[1]),
                                                     **LIM3)
        got = val.double().cpu().reshape(B, -1)[:, act].reshape(-1).numpy()
        ry = float((np.abs(got - y_ref) / b_y).max())
        sums, bsum = logg.reshape(B, -1).sum(1), b_l.reshape(B, -1).sum(1) + CB.EPS32 * np.abs(logg.reshape(B, -1).sum(1))
        rl = float((np.abs(lj.double().cpu().numpy() - sums) / bsum).max())
        parity_report(f"cntr {tag} fp32 atom {k}", "y/site, logJ/sample", max(ry, rl), CB.C_SITE, "err / conditioned bound")
        assert ry <= CB.C_SITE and rl <= CB.C_SITE, (k, ry, rl)
        assert (val.reshape(B, -1)[:, ~act.to(DEV)] == 0).all()


# ---------------------------------------------------------------------------------------------- every path
def _paths_case(kind, shape, hidden, m, dtype, B=3, seed=0):
    torch.manual_seed(100 + seed)
    control = 1.1 * torch.randn((B,) + shape, dtype=torch.float64, device=DEV)
    x = 1.3 * torch.randn((B,) + shape, dtype=torch.float64, device=DEV)
    cpl, gen, kw = make_block(kind, shape, hidden, m, dtype, control.to(dtype), seed=seed)
    return cpl, gen, kw, x.to(dtype), control.to(dtype)


def _oracle_of(cpl, kind, shape, x, control, kw, **extra):
    _, onets = oracle_leaves(cpl)
    with torch.no_grad():
        return oracle_block(x.double().cpu(), control.double().cpu(), onets, kind, shape, **kw, **extra)


@pytest.mark.parametrize("kind", ["affine", "rqs"])
def test_path_generic_fp64(parity_report, kind):
    """(a) (4, 6) fp64: the materialising path (logits through the conv kernels, then nf_affine / nf_rqs), with gradients and
    under no_grad, forward and backward; and per-site propagate_density under no_grad."""
    shape = (4, 6)
    cpl, gen, kw, x, control = _paths_case(kind, shape, [4], 5, torch.float64)
    yo, lo = _oracle_of(cpl, kind, shape, x, control, kw)
    y, lj = cpl(x.clone().requires_grad_(True))
    with torch.no_grad():
        y_ng, lj_ng = cpl(x)
        xb, l0 = cpl.backward(y_ng, log0=lj_ng)
    e = max(rel(y, yo), rel(lj, lo), rel(y_ng, yo), rel(lj_ng, lo))
    parity_report(f"cntr path generic fp64 {kind}", "y / logJ", e, 1e-9)
    assert e <= 1e-9 and rel(xb, x) <= 1e-6 and float(l0.abs().max()) <= 1e-6
    gen.control = active_bump(control, shape)
    with torch.no_grad():
        y_b, _ = cpl(x)
    assert float((y_b - y_ng).abs().max()) > 1e-3           # the control's values on the first atom's active sites count
    yo_b, lo_b = _oracle_of(cpl, kind, shape, x, gen.control, kw)
    assert rel(y_b, yo_b) <= 1e-9
    # per-site densities: the sites sum to the oracle's log J, the values do not change
    cpl.propagate_density = True
    with torch.no_grad():
        y_s, sites = cpl(x)
    assert sites.shape == x.shape and rel(y_s, yo_b) <= 1e-9 and rel(sites.reshape(x.shape[0], -1).sum(1), lo_b) <= 1e-9


@pytest.mark.parametrize("kind", ["affine", "rqs"])
def test_path_small_lattice_fp32(parity_report, kind):
    """(b) (6, 16) fp32 under no_grad, hidden [8, 8], m = 16: the one-launch small-lattice kernel takes the control atom."""
    shape = (6, 16)
    cpl, gen, kw, x, control = _paths_case(kind, shape, [8, 8], 16, torch.float32, seed=1)
    opts = _hip.make_rqs_opts(16, kw['xlim'], kw['ylim'], kw['extrap'], _hip.LAYOUT_PAIR) if kind == 'rqs' else None
    xa = cpl.mask.purify(x, 0)
    _, onets = oracle_leaves(cpl)
    with torch.no_grad():
        got = cpl._small_lattice_atom(0 if kind == 'rqs' else 1, False, xa, control, 0, cpl.nets[0], 0, opts)
        assert got is not None, "the small-lattice kernel did not take the controlled atom"
        out = onets[0](control.double().cpu().unsqueeze(1))
        va, la = ATOM[kind](xa.double().cpu(), out, O.channel_mask(shape, 0), **kw)
        y, lj = cpl(x)
    yo, lo = _oracle_of(cpl, kind, shape, x, control, kw)
    e = max(rel(got[0], va), rel(got[1], la), rel(y, yo), rel(lj, lo))
    parity_report(f"cntr path small-lattice fp32 {kind}", "atom and block, y / logJ", e, 1e-5)
    assert e <= 1e-5, (rel(got[0], va), rel(got[1], la), rel(y, yo), rel(lj, lo))
    gen.control = active_bump(control, shape)
    with torch.no_grad():
        y_b, lj_b = cpl(x)
    assert float((y_b - y).abs().max()) > 1e-3
    yo_b, lo_b = _oracle_of(cpl, kind, shape, x, gen.control, kw)
    assert rel(y_b, yo_b) <= 1e-5 and rel(lj_b, lo_b) <= 1e-5


@pytest.mark.parametrize("kind", ["affine", "rqs"])
def test_path_split_fp16_chain_fp32(parity_report, kind):
    """(c) (2, 2, 2, 32) fp32 under no_grad, hidden [8, 8]: the split-fp16 chain with the last layer fused into the coupling
    kernel takes the control atom."""
    shape = (2, 2, 2, 32)
    cpl, gen, kw, x, control = _paths_case(kind, shape, [8, 8], 16, torch.float32, seed=2)
    xa = cpl.mask.purify(x, 0)
    _, onets = oracle_leaves(cpl)
    with torch.no_grad():
        got = cpl._fused_atom(False, xa, control, 0, cpl.nets[0], 0)
        assert got is not None, "the fused atom did not take the controlled layer"
        if kind == 'rqs':         # (the fused affine layer does not report through nf_conv_last_path; it exists on the chain only)
            assert _hip.load().nf_conv_last_path() == 3, "the split-fp16 fused kernel did not run"
        out = onets[0](control.double().cpu().unsqueeze(1))
        va, la = ATOM[kind](xa.double().cpu(), out, O.channel_mask(shape, 0), **kw)
        y, lj = cpl(x)
        xb, l0 = cpl.backward(y, log0=lj)
        y2, _ = cpl(xb)
    yo, lo = _oracle_of(cpl, kind, shape, x, control, kw)
    e = max(rel(got[0], va), rel(got[1], la), rel(y, yo), rel(lj, lo))
    parity_report(f"cntr path split-fp16 fp32 {kind}", "atom and block, y / logJ", e, 1e-5)
    assert e <= 1e-5, (rel(got[0], va), rel(got[1], la), rel(y, yo), rel(lj, lo))
    assert rel(y2, y) <= 1e-3                                  # smoke()'s forward residual of the round trip
    gen.control = active_bump(control, shape)
    with torch.no_grad():
        y_b, lj_b = cpl(x)
    assert float((y_b - y).abs().max()) > 1e-3
    yo_b, lo_b = _oracle_of(cpl, kind, shape, x, gen.control, kw)
    assert rel(y_b, yo_b) <= 1e-5 and rel(lj_b, lo_b) <= 1e-5


@pytest.mark.parametrize("kind", ["affine", "rqs"])
def test_path_training_fused_fp32(parity_report, kind):
    """(d) the shape of (c) with gradients required and set_training_fusion(0): the spline's logit-free training node (the
    affine layer: conv nodes + nf_affine) takes the control atom; values at 1e-5, every gradient at 2e-4 of its largest
    entry, against autograd through the oracle."""
    shape = (2, 2, 2, 32)
    cpl, gen, kw, x, control = _paths_case(kind, shape, [8, 8], 16, torch.float32, seed=3)
    old = set_training_fusion(0)
    try:
        if kind == 'rqs':
            xa = cpl.mask.purify(x, 0).requires_grad_(True)
            assert cpl._train_fused_atom(False, xa, control, 0, cpl.nets[0], 0) is not None, \
                "the logit-free training node did not take the controlled layer"
        xk = x.clone().requires_grad_(True)
        y, lj = cpl(xk)
        names = [n for n, _ in cpl.named_parameters()]
        got = torch.autograd.grad((y ** 2).mean() + lj.mean(), [xk] + [p for _, p in cpl.named_parameters()])
        gen.control = active_bump(control, shape)
        y_b, _ = cpl(xk)
    finally:
        set_training_fusion(old)
    leaves, onets = oracle_leaves(cpl)
    xo = x.double().cpu().requires_grad_(True)
    yo, lo = oracle_block(xo, control.double().cpu(), onets, kind, shape, **kw)
    ref = torch.autograd.grad((yo ** 2).mean() + lo.mean(), [xo] + [leaves[n] for n in names])
    e = max(rel(y, yo), rel(lj, lo))
    parity_report(f"cntr path training fp32 {kind}", "y / logJ", e, 1e-5)
    assert e <= 1e-5, (rel(y, yo), rel(lj, lo))
    worst = 0.0
    for n, g, r in zip(['x'] + names, got, ref):
        err = float((g.double().cpu() - r).abs().max()) / float(r.abs().max())
        worst = max(worst, err)
        assert err <= 2e-4, (n, err)
    parity_report(f"cntr path training fp32 {kind}", "gradients", worst, 2e-4, "of each gradient's largest entry")
    assert float((y_b - y).abs().max()) > 1e-3


# ---------------------------------------------------------------------------------------------- chain, multi, direct
def test_chain_over_one_mask_stays_controlled():
    """ModuleList_([CntrAffineCoupling_, AffineCoupling_]) over one mask object hands the parts over (nn/_core.py:_run_chain):
    the same (y, log J) as block after block by hand, forward and backward; the generator is called once per forward and
    never in backward."""
    shape, B = (4, 6), 3
    torch.manual_seed(7)
    control = 1.1 * torch.randn((B,) + shape, dtype=torch.float64, device=DEV)
    cntr, gen, _ = make_block('affine', shape, [4], 0, torch.float64, control, n_nets=3, seed=4)
    nets = [ConvAct(1, 2, 3, conv_dim=2, hidden_sizes=[4], acts=['tanh', None]) for _ in range(2)]
    plain = AffineCoupling_(nets, mask=cntr.mask).to(device=DEV, dtype=torch.float64)
    chain = ModuleList_([cntr, plain])
    x = 1.3 * torch.randn((B,) + shape, dtype=torch.float64, device=DEV)
    with torch.no_grad():
        y, lj = chain(x)
        assert gen.calls == [B]
        xb, l0 = chain.backward(y, log0=lj)
        assert gen.calls == [B]
        y1, l1 = cntr(x)
        y2, l2 = plain(y1, l1)
        assert gen.calls == [B, B]
        x1, m1 = plain.backward(y2, l2)
        x0, m0 = cntr.backward(x1, m1)
        assert gen.calls == [B, B]
    assert rel(y, y2) <= 1e-12 and rel(lj, l2) <= 1e-12 and rel(xb, x0) <= 1e-12 and rel(l0, m0) <= 1e-12
    assert rel(xb, x) <= 1e-9 and float(l0.abs().max()) <= 1e-9
    leaves, onets = oracle_leaves(cntr)
    _, pnets = oracle_leaves(plain)
    with torch.no_grad():
        yo, lo = oracle_block(x.double().cpu(), control.double().cpu(), onets, 'affine', shape)
        yo, lo = oracle_block(yo, None, pnets, 'affine', shape, log0=lo)
    assert rel(y, yo) <= 1e-9 and rel(lj, lo) <= 1e-9
    gen.control = active_bump(control, shape)
    with torch.no_grad():
        y_b, _ = chain(x)
    assert float((y_b - y).abs().max()) > 1e-3              # a chain that skipped the control would not move


def test_multi_spline_variant_fp64(parity_report):
    """CntrMultiRQSplineCoupling_, n_s = 2 on (4, 6) in fp64, against O.multi_rqs_coupling_atom composed with the control."""
    shape, B, ns, m = (4, 6), 3, 2, 5
    torch.manual_seed(8)
    control = 1.1 * torch.randn((B, ns) + shape, dtype=torch.float64, device=DEV)
    x = 1.3 * torch.randn((B, ns) + shape, dtype=torch.float64, device=DEV)
    nets = [ConvAct(ns, ns * (3 * m - 2), 3, conv_dim=2, hidden_sizes=[4], acts=['tanh', None]) for _ in range(2)]
    with torch.no_grad():
        for net in nets:
            for p in list(net.parameters())[-2:]:
                p.mul_(0.3)
    gen = Generator(control)
    kw = dict(xlims=[(-5.0, 5.0), (-4.0, 4.0)], ylims=[(-5.0, 5.0), (-4.0, 4.0)], extraps=[LIN, LIN])
    cpl = CntrMultiRQSplineCoupling_(nets, mask=EvenOddMask(shape=shape), control_generator=gen, **kw)
    cpl = cpl.to(device=DEV, dtype=torch.float64)
    _, onets = oracle_leaves(cpl)
    with torch.no_grad():
        y, lj = cpl(x)
        xb, l0 = cpl.backward(y, log0=lj)
        yo, lo = oracle_block(x.cpu(), control.cpu(), onets, 'multirqs', shape, **kw)
    e = max(rel(y, yo), rel(lj, lo))
    parity_report("cntr multi-spline fp64", "y / logJ", e, 1e-9)
    assert e <= 1e-9 and rel(xb, x) <= 1e-6 and float(l0.abs().max()) <= 1e-6 and gen.calls == [B]
    gen.control = control + 0.7 * O.channel_mask(shape, 0).to(DEV)
    with torch.no_grad():
        y_b, _ = cpl(x)
    assert float((y_b - y).abs().max()) > 1e-3


def test_direct_variant_equals_the_generated_one():
    class D(DirectCntrCoupling_, AffineCoupling_):
        pass
    shape, B = (4, 6), 3
    torch.manual_seed(9)
    control = 1.1 * torch.randn((B,) + shape, dtype=torch.float64, device=DEV)
    cntr, gen, _ = make_block('affine', shape, [4], 0, torch.float64, control, n_nets=3, seed=5)
    direct = D(list(cntr.nets), mask=cntr.mask)
    x = 1.3 * torch.randn((B,) + shape, dtype=torch.float64, device=DEV)
    log0 = torch.linspace(-1.0, 1.0, B, dtype=torch.float64, device=DEV)
    with torch.no_grad():
        y, lj = cntr(x, log0)
        (yd, cd), ld = direct((x, control), log0)
        (xd, cb), l0 = direct.backward((yd, control), ld)
        xc, lc = cntr.backward(y, lj)
    assert cd is control and cb is control
    assert torch.equal(yd, y) and torch.equal(ld, lj) and torch.equal(xd, xc) and torch.equal(l0, lc)
    assert rel(xd, x) <= 1e-9 and rel(l0, log0) <= 1e-9
    # a ModuleList_ does not merge the direct block into a chain: it has no parts_forward
    assert getattr(direct, 'parts_forward', None) is None

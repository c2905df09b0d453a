"""Pin the CPU oracle (oracle/nf_oracle.py) to the reference: every golden vector in
tests/golden/*.npz was produced by running the reference itself (make_golden.py);
the oracle must reproduce it in fp64 to <=1e-12 (values) / <=1e-10 (gradients)."""
import numpy as np
import pytest
import torch

from oracle import nf_oracle as O

T = lambda a: torch.from_numpy(np.asarray(a))
TOL = 1e-12


def close(a, b, tol=TOL):
    a, b = T(a) if not torch.is_tensor(a) else a, T(b) if not torch.is_tensor(b) else b
    scale = max(1.0, float(b.abs().max())) if b.numel() else 1.0
    err = float((a.detach() - b).abs().max()) if b.numel() else 0.0
    assert err <= tol * scale, f"max err {err:g} > {tol*scale:g}"


ATOM_OPTS = {
    "rqs_lin": dict(xlim=(-2.0, 2.0), ylim=(-2.5, 1.5), extrap={'left': 'linear', 'right': 'linear'}),
    "rqs_anti": dict(xlim=(0.0, 2.0), ylim=(0.0, 2.0), extrap={'left': 'anti', 'right': 'linear'}),
    "rqs_none": dict(xlim=(0.0, 1.0), ylim=(0.0, 1.0), extrap={}),
    "rqs_onesided": dict(xlim=(0.0, 1.0), ylim=(0.0, 1.0), extrap={'right': 'linear'}),
    "rqs_fixedx": dict(xlim=(-1.0, 1.0), ylim=(-1.0, 1.0), extrap={'left': 'linear', 'right': 'linear'}),
    "multirqs": dict(xlims=[(-2.0, 2.0), (-1.0, 3.0)], ylims=[(-2.0, 2.0), (-3.0, 1.0)],
                     extraps=[{'left': 'linear', 'right': 'linear'}] * 2),
}


def atom_fn(tag):
    kind = tag.split("/")[0]
    if kind == "affine":
        return O.affine_coupling_atom, {}
    if kind == "shift":
        return O.shift_coupling_atom, {}
    if kind == "multirqs":
        return O.multi_rqs_coupling_atom, ATOM_OPTS[kind]
    return O.rqs_coupling_atom, ATOM_OPTS[kind]


def atom_cases():
    import os
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "atoms.npz"))
    return [str(c) for c in z["_cases"]]


def on_knots(tag, x, out, amask, opts):
    """make_golden.py puts every third input of the rqs_lin cases exactly on a knot (the tie rule of the bin search).  The
    knots are softmax / cumsum results whose last bits follow the CPU's vector code path: on another CPU the stored input
    sits an ulp or two beside the oracle's knot, and the gradient there takes the other one-sided derivative.  Those
    inputs are checked to be the knots of the stored case and put back on the oracle's knots, bit for bit."""
    if not tag.startswith("rqs_lin"):
        return x
    kx, ky, kd = O.knots_from_logits(out, opts["xlim"], opts["ylim"])
    kx = O.augment_knots(kx, ky, kd, axis=1, **opts["extrap"])[0]
    B, n = x.shape[0], kx.shape[1]
    flat, kflat, active = x.clone().reshape(B, -1), kx.reshape(B, n, -1), amask.reshape(-1)
    for j in range(0, flat.shape[1], 3):
        if active[j]:
            k = kflat[:, (j // 3) % n, j]
            assert float((flat[:, j] - k).abs().max()) <= 1e-12, (tag, j)
            flat[:, j] = k
    return flat.reshape(x.shape)


@pytest.mark.parametrize("tag", atom_cases())
def test_atom_forward_inverse_grads(golden, tag):
    z = golden("atoms")
    g = lambda k: T(z[f"{tag}/{k}"])
    fn, opts = atom_fn(tag)
    opts = dict(opts)
    if tag.startswith("rqs_fixedx"):
        opts["knots_x"] = g("knots_x")
    shape, parity = tuple(int(v) for v in z[f"{tag}/shape"]), int(z[f"{tag}/parity"])
    amask = O.channel_mask(shape, parity)
    x = on_knots(tag, g("x_active"), g("out"), amask, opts).requires_grad_(True)
    out = g("out").clone().requires_grad_(True)
    y, logJ = fn(x, out, amask, log0=g("log0"), **opts)
    close(y, g("y"))
    close(logJ, g("logJ"))
    loss = logJ.mean() + (y ** 2).mean()
    inputs = [t for t in (x, out) if loss.requires_grad]
    gx, gout = torch.autograd.grad(loss, (x, out), allow_unused=True)
    close(gx if gx is not None else torch.zeros_like(x), g("grad_x"), 1e-10)
    close(gout if gout is not None else torch.zeros_like(out), g("grad_out"), 1e-10)
    # inverse: the reference's own inverse is unreliable in linear tails,
    # so compare with the reference inverse only where it round-trips, and pin the rest by
    # the round trip against the forward golden.
    xh, lrt = fn(g("y"), g("out"), amask, inverse=True, log0=g("logJ"), **opts)
    close(xh, g("x_active"), 1e-9)
    close(lrt, g("log0"), 1e-9)
    ref_ok = (T(z[f"{tag}/xhat"]) - g("x_active")).abs() < 1e-9
    close(xh[ref_ok], g("xhat")[ref_ok], 1e-9)


def dc_cases():
    import os
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "distconv.npz"))
    return [str(c) for c in z["_cases"]]


@pytest.mark.parametrize("tag", dc_cases())
def test_distconvertor(golden, tag):
    z = golden("distconv")
    g = lambda k: T(z[f"{tag}/{k}"])
    sym = "sym1" in tag
    smooth = "sm1" in tag
    x = g("x").clone().requires_grad_(True)
    wx = g("wx").clone().requires_grad_(True)
    wy = g("wy").clone().requires_grad_(True)
    wd = None if smooth else g("wd").clone().requires_grad_(True)
    y, logJ = O.dist_convertor(x, wx, wy, wd, symmetric=sym, log0=g("log0"))
    close(y, g("y"))
    close(logJ, g("logJ"))
    loss = logJ.mean() + (y ** 2).mean()
    ps = [x, wx, wy] + ([] if smooth else [wd])
    grads = torch.autograd.grad(loss, ps)
    for gr, name in zip(grads, ["grad_x", "grad_wx", "grad_wy", "grad_wd"]):
        close(gr, g(name), 1e-10)
    with torch.no_grad():
        xh, lrt = O.dist_convertor(g("y"), wx, wy, wd, symmetric=sym, inverse=True, log0=g("logJ"))
    close(xh, g("x"), 1e-9)
    close(lrt, g("log0"), 1e-9)
    close(xh, g("xhat"), 1e-9)
    close(lrt, g("logJ_rt"), 1e-9)


def _block_nets(z, tag, d, n_nets=3, conv=O.circular_conv_fast):
    nets = []
    for k in range(n_nets):
        layers = []
        for i in (0, 2, 4):
            pre = f"{tag}/param/nets.{k}.{i}."
            if d == 4:
                wl = T(z[pre + "_conv_lower_dim.weight"])
                b = T(z[pre + "bias"])
                w = O.conv4d_standard_weight(wl, b.shape[0], 3)
            else:
                w, b = T(z[pre + "weight"]), T(z[pre + "bias"])
            layers.append((w, b))
        nets.append(lambda t, layers=layers: O.conv_act(t, layers, ['tanh', 'tanh', None], conv=conv))
    return nets


@pytest.mark.parametrize("kind", ["affine", "rqs"])
@pytest.mark.parametrize("d", [1, 2, 3, 4])
@pytest.mark.parametrize("conv", ["fast", "direct"])
def test_coupling_block_with_convact(golden, kind, d, conv):
    z = golden("blocks")
    tag = f"{kind}/d{d}"
    shape = tuple(int(v) for v in z[f"{tag}/shape"])
    convf = O.circular_conv_fast if conv == "fast" else O.circular_conv_direct
    nets = _block_nets(z, tag, d, conv=convf)
    opts = {} if kind == "affine" else dict(xlim=(-3.0, 3.0), ylim=(-3.0, 3.0),
                                            extrap={'left': 'linear', 'right': 'linear'})
    x = T(z[f"{tag}/x"])
    y, logJ = O.coupling_block(x, nets, kind, shape, **opts)
    close(y, z[f"{tag}/y"], 1e-11)
    close(logJ, z[f"{tag}/logJ"], 1e-11)
    xh, lrt = O.coupling_block(T(z[f"{tag}/y"]), nets, kind, shape, inverse=True,
                               log0=T(z[f"{tag}/logJ"]), **opts)
    # round trip through 3 layers whose random-init nets give min g ~ 1e-4 (d=4 case):
    # conditioning, not arithmetic, sets the floor here (the reference's own round trip
    # fails outright at d=3,4: its inverse bug in linear tails)
    close(xh, x, 1e-7)
    close(lrt, torch.zeros_like(lrt), 1e-7)
    close(T(z[f"{tag}/mask"]).double(), O.channel_mask(shape, 0))


def test_callers_c1_and_endpoints(golden):
    z = golden("callers")
    x = T(z["c1/x"])
    logr = O.normal_log_prob(x)
    close(logr, z["c1/logr"])
    y, logJ = O.dist_convertor(x, T(z["c1/wx"]), T(z["c1/wy"]), T(z["c1/wd"]), symmetric=True)
    close(y, z["c1/y"])
    close(logJ, z["c1/logJ"])
    logq = logr - logJ
    logp = -O.phi4_action(y, kappa=0, m_sq=-1.2, lambd=0.5)
    close(logq, z["c1/logq"])
    close(logp, z["c1/logp"])
    close(O.kl_loss(logq, logp), z["c1/loss"])
    xb, mlogJ = O.dist_convertor(y, T(z["c1/wx"]), T(z["c1/wy"]), T(z["c1/wd"]), symmetric=True, inverse=True)
    close(O.normal_log_prob(xb) + mlogJ, z["c1/log_prob"], 1e-9)
    kap, msq, lam = (float(v) for v in z["phi4/coef"])
    for d in (1, 2, 3, 4):
        cfg = T(z[f"phi4/d{d}/cfg"])
        close(O.phi4_action(cfg, kappa=kap, m_sq=msq, lambd=lam), z[f"phi4/d{d}/S"])
        close(O.normal_log_prob(cfg), z[f"phi4/d{d}/logr"])
    for key in [k for k in z.files if k.startswith("mask/")]:
        _, shp, p = key.split("/")
        shape = tuple(int(s) for s in shp.split("x"))
        assert np.array_equal(O.even_odd_mask(shape, parity=int(p[1:])).numpy(), z[key])


def test_survey_appendix_b_known_answers():
    """SURVEY Appendix B micro-semantics (verified there by running the reference)."""
    kx = torch.tensor([0, .25, .5, 1.]).double()
    ky = torch.tensor([0, .4, .6, 1.]).double()
    kd = torch.tensor([1, 2, .5, 1.]).double()
    ax, ay, ad = O.augment_knots(kx, ky, kd, 'linear', 'linear')
    assert torch.allclose(ax, torch.tensor([-1, 0, .25, .5, 1, 2.]).double())
    assert torch.allclose(ay, torch.tensor([-1, 0, .4, .6, 1, 2.]).double())
    assert torch.allclose(ad, torch.tensor([1, 1, 2, .5, 1, 1.]).double())
    x = torch.tensor([-3, -1, -.5, 0, .1, .25, .3, .5, .9, 1, 1.5, 2, 7.]).double()
    seg = O._segment_index(ax.reshape(-1, 1), x.reshape(1, -1), 0).ravel()
    assert seg.tolist() == [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 4]
    y, g = O.rqs_evaluate(ax.reshape(-1, 1), ay.reshape(-1, 1), ad.reshape(-1, 1), x.reshape(1, -1), axis=0)
    ye = [-3, -1, -.5, 0, .1278, .4, .4746, .6, .9020, 1, 1.5, 2, 7]
    ge = [1, 1, 1, 1, 1.5390, 2, 1.1175, .5, .9538, 1, 1, 1, 1]
    assert np.allclose(y.ravel().numpy(), ye, atol=5e-5)
    assert np.allclose(g.ravel().numpy(), ge, atol=5e-5)
    assert abs(float(O.softplus_ln2(torch.zeros(1).double())) - 1.0) < 1e-15


def test_reference_fp32_fixture_covers_every_case_and_matches_oracle_fp32(golden):
    """tests/golden/ref_fp32.npz (the reference run in float32 on the goldens' inputs, make_golden_fp32.py) is what the GPU
    tests take their loosened fp32 bounds from.  (1) it has an entry for every case and quantity; (2) the CPU oracle run
    in float32 lands within a small factor of the reference's own float32 error on the forward map -- so the oracle in
    float32 is a fair stand-in floor for GPU tests whose inputs have no reference fixture."""
    import os
    r = np.load(os.path.join(os.path.dirname(__file__), "golden", "ref_fp32.npz"))
    z = golden("atoms")
    rel = lambda a, b: float((T(a).double() - T(b).double()).abs().max()) / max(1.0, float(T(b).double().abs().max()))
    worst = 0.0
    for tag in atom_cases():
        for key in ("y", "logJ", "grad_x", "grad_out", "xhat", "logJ_rt"):
            assert f"atoms/{tag}/{key}" in r.files
        fn, opts = atom_fn(tag)
        opts = dict(opts)
        if tag.startswith("rqs_fixedx"):
            opts["knots_x"] = T(z[f"{tag}/knots_x"]).float()
        shape, parity = tuple(int(v) for v in z[f"{tag}/shape"]), int(z[f"{tag}/parity"])
        g32 = lambda k: T(z[f"{tag}/{k}"]).float()
        y, lj = fn(g32("x_active"), g32("out"), O.channel_mask(shape, parity, dtype=torch.float32), log0=g32("log0"), **opts)
        for key, ours in (("y", y), ("logJ", lj)):
            e_ref, e_or = rel(r[f"atoms/{tag}/{key}"], z[f"{tag}/{key}"]), rel(ours, z[f"{tag}/{key}"])
            worst = max(worst, e_or / max(e_ref, 1e-6))
    assert worst <= 4.0, worst
    for fam, name in (("distconv", "distconv"), ("blocks", "blocks")):
        zz = golden(name)
        for tag in [str(c) for c in zz["_cases"]]:
            assert f"{fam}/{tag}/y" in r.files and f"{fam}/{tag}/logJ" in r.files and f"{fam}/{tag}/grad_x" in r.files


def test_philox_known_answers_and_prior_sampler_oracle():
    """The oracle's Philox4x32-10 against Random123's published known-answer vectors (kat_vectors: three (counter, key) ->
    output triples), then the sampler restatement built on it: moments of the draws and logr = log N(x) exactly."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = O.philox4x32_10(np.array(ctr, dtype=np.uint32), np.array(key, dtype=np.uint32))
        assert tuple(int(v) for v in got) == want
    for dt in (torch.float32, torch.float64):
        x, logr = O.normal_prior_sample(77, 3, 4000, 37, dtype=dt)
        assert abs(float(x.double().mean())) < 0.01 and abs(float(x.double().std()) - 1.0) < 0.01
        close(logr.double(), O.normal_log_prob(x.double()), 1e-5 if dt == torch.float32 else 1e-12)
    loc, scale = torch.linspace(-1, 1, 10), torch.linspace(0.5, 2.0, 10)
    x, logr = O.normal_prior_sample(5, 0, 20000, 10, loc=loc, scale=scale, dtype=torch.float64)
    assert float((x.mean(dim=0) - loc).abs().max()) < 0.05 and float((x.std(dim=0) / scale - 1).abs().max()) < 0.03
    ref = torch.distributions.Normal(loc.double(), scale.double()).log_prob(x).sum(dim=1)
    close(logr, ref, 1e-12)


# ------------------------------------------------------------------ small 16-wide lattices (the shapes of nf_conv_s.hip)
def small16_cases():
    import os
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "small16.npz"))
    return [str(c) for c in z["_cases"]]


SMALL16_LIM = dict(xlim=(-3.0, 3.0), ylim=(-3.0, 3.0), extrap={'left': 'linear', 'right': 'linear'})


def small16_nets(z, tag, n_nets=2, dtype=torch.float64):
    nets = []
    for k in range(n_nets):
        layers = [(T(z[f"{tag}/param/nets.{k}.{i}.weight"]).to(dtype), T(z[f"{tag}/param/nets.{k}.{i}.bias"]).to(dtype)) for i in (0, 2, 4)]
        nets.append(lambda x, layers=layers: O.conv_act(x, layers, ['tanh', 'tanh', None]))
    return nets


@pytest.mark.parametrize("tag", small16_cases())
def test_small16_blocks_against_reference(golden, tag):
    """Whole Coupling_ blocks on 2-D / 3-D lattices with a 16-site fastest axis, as the reference computes them
    (tests/golden/make_golden_small16.py): the fixtures the small-lattice fused kernel is held to on the GPU."""
    z = golden("small16")
    kind = tag.split("/")[0]
    shape = tuple(int(v) for v in z[f"{tag}/shape"])
    opts = SMALL16_LIM if kind == "rqs" else {}
    y, logJ = O.coupling_block(T(z[f"{tag}/x"]), small16_nets(z, tag), kind, shape, **opts)
    close(y, z[f"{tag}/y"])
    close(logJ, z[f"{tag}/logJ"])
    xh, lrt = O.coupling_block(T(z[f"{tag}/y"]), small16_nets(z, tag), kind, shape, inverse=True, log0=T(z[f"{tag}/logJ"]), **opts)
    close(xh, z[f"{tag}/x"], 1e-8)
    close(lrt, np.zeros_like(z[f"{tag}/logJ"]), 1e-8)

"""GPU parity tests (pytest -m gpu): the HIP path, called through the C ABI
(libnormflow_hip.so via normflow__amd._hip), against
  * the golden vectors produced by the reference itself (tests/golden/*.npz), and
  * the CPU oracle on the same seeded inputs,
plus size-independent properties at BASELINE.json's full sizes.

Tolerances (north_star: "within 1e-5 relative fp32 tolerance"):
  fp64 kernels : 1e-9  relative (only formula re-association separates them from the fp64 reference)
  fp32 kernels : 1e-5  relative on the transformed field and on log|J| (north_star's bound); gradients 2e-4.
                 RQ-spline atoms on the reference's goldens: the PER-SITE CONDITIONED BOUND of tests/cond_bound.py
                 (C_SITE x [sum_q |df/dq| delta_q + roundoff], computed in float64 from the oracle's knots), the same
                 constant the reference's own float32 outputs (tests/golden/ref_fp32.npz) are held to in
                 tests/test_cond_bound.py -- for y and log g at every site, and summed over a sample's sites for log|J|.
                 Elsewhere, where a case is ill-conditioned in single precision: max(1e-5, 2 * err_ref_fp32),
                 err_ref_fp32 = the error of the reference's own float32 run OF THAT CASE against its float64 run; cases
                 without a reference fixture (inputs seeded on the GPU) use the CPU oracle run in float32 the same way.
                 Every bound a case passed is printed in the run's "parity report" section.
relative = max|a-b| / max(1, max|b|).
"""
import os
import numpy as np
import pytest
import torch

import normflow__amd  # noqa: F401
from normflow__amd import _hip
from normflow__amd.mask import EvenOddMask
from normflow__amd.nn import (ConvAct, AffineCoupling_, RQSplineCoupling_, ShiftCoupling_,
                              MultiRQSplineCoupling_, DistConvertor_, ModuleList_)
from oracle import nf_oracle as O
from test_oracle_golden import ATOM_OPTS, atom_cases, dc_cases
import cond_bound as CB

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None
TOL = {torch.float64: dict(val=1e-9, grad=1e-8), torch.float32: dict(val=1e-5, grad=2e-4)}


def T(a, dtype=torch.float64, dev=None):
    return torch.from_numpy(np.asarray(a)).to(device=dev or DEV, dtype=dtype)


def rel(a, b):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    if b.numel() == 0:
        return 0.0
    return float((a - b).abs().max()) / max(1.0, float(b.abs().max()))


_REF32 = None


def ref32(fam, key):
    """float32 output of the reference itself for golden `fam`/`key` (tests/golden/ref_fp32.npz)."""
    global _REF32
    if _REF32 is None:
        _REF32 = np.load(os.path.join(os.path.dirname(__file__), "golden", "ref_fp32.npz"), allow_pickle=False)
    return torch.from_numpy(_REF32[f"{fam}/{key}"]).double()


def _one_floor(z, fam, key, sel=None, target=None):
    a = ref32(fam, key)
    b = torch.from_numpy(np.asarray(z[key] if target is None else target)).double().reshape(a.shape)
    if sel is not None:
        a, b = a.reshape(-1, sel.numel())[:, sel.cpu()], b.reshape(-1, sel.numel())[:, sel.cpu()]
    return rel(a, b)


def floor_tol(z, fam, key, base, sel=None, target=None):
    """max(base, 2 * err_ref_fp32): err_ref_fp32 = relative error of the reference's float32 run OF THIS CASE against
    `target` (default: its own float64 golden `key`), optionally on a subset `sel` of the last axis.  (The RQ-spline atoms
    do not use this: they are held to the per-site conditioned bound of tests/cond_bound.py.)"""
    return max(base, 2.0 * _one_floor(z, fam, key, sel, target))


def compact(t, act):
    """(B, C, V) full-lattice tensor -> (B, C, V/2): the active site's column of every pair."""
    B, C, V = t.shape
    pick = act.reshape(-1, 2)[:, 0].bool()             # True: site 2h is the active one
    pairs = t.reshape(B, C, V // 2, 2)
    return torch.where(pick, pairs[..., 0], pairs[..., 1]).contiguous()


def uncompact(t, act):
    B, C, Vh = t.shape
    pick = act.reshape(-1, 2)[:, 0].bool()
    z = torch.zeros_like(t)
    return torch.stack((torch.where(pick, t, z), torch.where(pick, z, t)), dim=-1).reshape(B, C, 2 * Vh)


def check_fused_round_trip(cpl, net, acts, xa, xf, yf, lf, l0, parity, shape, lim, nb=4):
    """inverse(forward) through the fused kernels.  (a) whole batch, the well-conditioned statement: pushing the recovered
    x forward again lands on y (2e-5: two fp32 passes).  (b) x itself and the cancelling log-Jacobians on `nb` samples,
    bounded by max(1e-5, 2 * floor), floor = the same round trip by the CPU oracle run in FLOAT32 (the reference's
    arithmetic restated; x = f^-1(y) is conditioned by 1/g, which random-init nets push to ~1e-3)."""
    B = xa.shape[0]
    xb, lb = cpl._fused_atom(True, yf, xf, parity, net, lf)
    y2, _ = cpl._fused_atom(False, xb, xf, parity, net, l0)
    assert rel(y2, yf) <= 2e-5, ("forward residual of the inverse", rel(y2, yf))
    nb = min(nb, B)
    convs = [mod for mod in net if hasattr(mod, 'weight')]
    layers = [(c.weight.detach().float().cpu(), c.bias.detach().float().cpu()) for c in convs]
    am = O.channel_mask(shape, parity, dtype=torch.float32)
    out32 = O.conv_act(xf[:nb].float().cpu().unsqueeze(1), layers, acts)
    y32, l32 = O.rqs_coupling_atom(xa[:nb].float().cpu(), out32, am, log0=l0[:nb].float().cpu(), **lim)
    x32, b32 = O.rqs_coupling_atom(y32, out32, am, inverse=True, log0=l32, **lim)
    tx = max(1e-5, 2.0 * rel(x32, xa[:nb]))
    tl = max(1e-5, 2.0 * rel(b32, l0[:nb]))
    assert rel(xb[:nb], xa[:nb]) <= tx, ("round trip x", rel(xb[:nb], xa[:nb]), tx)
    assert rel(lb[:nb], l0[:nb]) <= tl, ("round trip logJ", rel(lb[:nb], l0[:nb]), tl)
    return xb, lb


def layouts_for(shape):
    return ["full", "pair"] if shape[-1] % 2 == 0 else ["full"]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("tag", atom_cases())
def test_atoms_against_reference_goldens(golden, parity_report, tag, dtype):
    z = golden("atoms")
    kind = tag.split("/")[0]
    tol = TOL[dtype]
    shape, parity = tuple(int(v) for v in z[f"{tag}/shape"]), int(z[f"{tag}/parity"])
    act = O.channel_mask(shape, parity).to(torch.uint8).reshape(-1).to(DEV)
    g = lambda k: T(z[f"{tag}/{k}"], dtype)
    B = g("x_active").shape[0]
    for layout in layouts_for(shape):
        lay = _hip.LAYOUT_PAIR if layout == "pair" else _hip.LAYOUT_FULL
        x = g("x_active")
        multi = kind == "multirqs"
        v = (x.reshape(B, 2, -1) if multi else x.reshape(B, -1)).clone().requires_grad_(True)
        out_full = g("out").reshape(B, g("out").shape[1], -1)
        if multi and layout == "pair":
            continue
        params = (compact(out_full, act) if layout == "pair" else out_full).clone().requires_grad_(True)

        def apply(inp, inverse, log0):
            if kind in ("affine", "shift"):
                return _hip.AffineCouplingFn.apply(inp, params, log0, act, lay, inverse)
            if multi:
                o = ATOM_OPTS[kind]
                opts = [_hip.make_rqs_opts(4, o["xlims"][i], o["ylims"][i], o["extraps"][i], lay) for i in range(2)]
                return _hip.MultiRQSCouplingFn.apply(inp, params, log0, act, opts, inverse)
            o = ATOM_OPTS[kind]
            if kind == "rqs_fixedx":      # knots_x fixed: 2m-1 channels
                kx = g("knots_x").contiguous()
                opts = _hip.make_rqs_opts((params.shape[1] + 1) // 2, o["xlim"], o["ylim"], o["extrap"], lay, kx)
            else:
                opts = _hip.make_rqs_opts((params.shape[1] + 2) // 3, o["xlim"], o["ylim"], o["extrap"], lay)
            return _hip.RQSCouplingFn.apply(inp, params, log0, act, opts, inverse)

        # The rqs_lin goldens put every 3rd input EXACTLY on a knot (tie semantics of the bin
        # search) and draw wide logits (std 1.2 => bins down to ~1e-2 of the range):
        #  * d(log g)/dx is one-sided at a knot, and a 1-ulp difference in the knot position
        #    (fp32, or a re-associated fp64 cumsum) flips the side: those sites are left out of
        #    the GRADIENT comparison (values are continuous there and are compared);
        #  * in fp32, the input and the knot positions carry eps * range of rounding, which a narrow steep bin
        #    amplifies by range / bin width * d(log g)/d(theta) (rqs_lin/d1p0m10: one input sits on a knot whose left
        #    bin is 0.033 wide with d(log g)/d(theta) = -161: one float32 ulp of x moves log g by 6e-4 -- which bin the
        #    rounded knot selects decides between that and a 100x milder neighbour; the reference's float32 run happened
        #    to round the other way).  Values and log|J| are therefore held to the per-site conditioned bound.
        V = out_full.shape[-1]
        keep = torch.ones(V, dtype=torch.bool, device=DEV)
        if kind == "rqs_lin":
            keep[::3] = False
        keep_p = compact(keep.reshape(1, 1, V).to(torch.uint8) * act.reshape(1, 1, V), act).reshape(-1).bool() \
            if layout == "pair" else keep
        f32 = dtype == torch.float32
        is_rqs = kind.startswith("rqs") or multi
        y, logJ = apply(v, False, g("log0"))
        if f32 and is_rqs:
            # float32 spline atoms: the per-site conditioned bound (tests/cond_bound.py) with the constant C_SITE that the
            # reference's own float32 outputs are held to in tests/test_cond_bound.py -- per site for y and log g, and the
            # sum of the sites' bounds for log|J|.  No sibling maxima, no fixture-family tolerances.
            opts_b = dict(ATOM_OPTS[kind])
            if kind == "rqs_fixedx":
                opts_b["knots_x"] = T(z[f"{tag}/knots_x"], dev="cpu")
            bf = CB.case_bounds(z, tag, opts_b)
            S, am = bf["val"].shape[1], torch.from_numpy(bf["am"])
            ys = y.detach().double().cpu().reshape(B, S, -1)[:, :, am].numpy()
            ry = float((np.abs(ys - bf["val"]) / bf["b_val"]).max())
            ej = np.abs(logJ.detach().double().cpu().numpy() - z[f"{tag}/logJ"])
            bj = CB.C_SITE * (bf["b_logd"].sum(axis=(1, 2)) + CB.EPS32 * np.abs(z[f"{tag}/logJ"]))
            parity_report(f"{tag} [{layout}]", "HIP f32 y/site", ry, CB.C_SITE, "largest err / site bound")
            iw = int(np.argmax(ej / bj))
            parity_report(f"{tag} [{layout}]", "HIP f32 logJ/sample", ej[iw], bj[iw], "the sample with the largest err / bound")
            assert ry <= CB.C_SITE, (tag, layout, "y per site vs conditioned bound", ry)
            assert (ej <= bj).all(), (tag, layout, "logJ vs summed site bounds", float((ej / bj).max()))
            if not multi:
                o = ATOM_OPTS[kind]
                kx = g("knots_x").contiguous() if kind == "rqs_fixedx" else None
                mm = (params.shape[1] + 1) // 2 if kind == "rqs_fixedx" else (params.shape[1] + 2) // 3
                so = _hip.make_rqs_opts(mm, o["xlim"], o["ylim"], o["extrap"], lay, kx)
                _, _, lg = _hip.rqs_sites(v.detach(), params.detach(), act, None, so, False)
                lgs = lg.double().cpu().reshape(B, 1, -1)[:, :, am].numpy()
                rl = float((np.abs(lgs - bf["logd"]) / bf["b_logd"]).max())
                parity_report(f"{tag} [{layout}]", "HIP f32 log g/site", rl, CB.C_SITE, "largest err / site bound")
                assert rl <= CB.C_SITE, (tag, layout, "log g per site vs conditioned bound", rl)
        else:
            assert rel(y.reshape(x.shape), g("y")) <= tol["val"], (tag, layout, "y", rel(y.reshape(x.shape), g("y")))
            assert rel(logJ, g("logJ")) <= tol["val"], (tag, layout, "logJ", rel(logJ, g("logJ")))
        loss = logJ.mean() + (y ** 2).mean()
        gv, gp = torch.autograd.grad(loss, (v, params))
        gxr = g("grad_x").reshape(v.shape)
        assert rel(gv[..., keep], gxr[..., keep]) <= tol["grad"], (tag, layout, "grad_x")
        gref = g("grad_out").reshape(out_full.shape)
        gref = compact(gref, act) if layout == "pair" else gref
        assert rel(gp[..., keep_p], gref[..., keep_p]) <= tol["grad"], (tag, layout, "grad_out")
        # inverse + its VJP (checked against autograd through the CPU oracle)
        yin = g("y").reshape(v.shape).clone().requires_grad_(True)
        xh, lrt = apply(yin, True, g("logJ"))
        if not f32:
            assert rel(xh.reshape(x.shape), g("x_active")) <= 200 * tol["val"], (tag, layout, "xhat")
            assert rel(lrt, g("log0")) <= 200 * tol["val"], (tag, layout, "logJ_rt")
        elif is_rqs:
            # x = f^-1(y) is conditioned by 1/g (these goldens reach g ~ 1e-4): the per-site conditioned bound of the
            # inverse (cond_bound.rqs_inverse_bound; the oracle's stable root run in float32 sits inside it with the same
            # constant, tests/test_cond_bound.py).  logJ_rt = logJ - sum log g': the bound is the sum of the sites' bounds
            # plus the rounding of the float32 log0 it starts from.
            bi = CB.case_bounds(z, tag, opts_b, inverse=True)
            xs = xh.detach().double().cpu().reshape(B, S, -1)[:, :, am].numpy()
            rx = float((np.abs(xs - bi["val"]) / bi["b_val"]).max())
            el = np.abs(lrt.detach().double().cpu().numpy() - z[f"{tag}/log0"])
            bl = CB.C_SITE * (bi["b_logd"].sum(axis=(1, 2)) + 2 * CB.EPS32 * (np.abs(z[f"{tag}/logJ"]) + np.abs(z[f"{tag}/log0"])))
            parity_report(f"{tag} [{layout}]", "HIP f32 xhat/site", rx, CB.C_SITE, "largest err / site bound")
            iw = int(np.argmax(el / bl))
            parity_report(f"{tag} [{layout}]", "HIP f32 logJ_rt/sample", el[iw], bl[iw], "the sample with the largest err / bound")
            assert rx <= CB.C_SITE, (tag, layout, "xhat per site vs conditioned bound", rx)
            assert (el <= bl).all(), (tag, layout, "logJ_rt vs summed site bounds", float((el / bl).max()))
            y2, _ = apply(xh.detach(), False, None)      # and the well-conditioned statement: the forward residual
            assert rel(y2.reshape(x.shape), g("y")) <= 10 * tol["val"], (tag, layout, "inverse residual", rel(y2.reshape(x.shape), g("y")))
        else:
            # affine / shift inverse x = (y - t) e^{|s|}: float32 knows y - t to eps (|y| + |t|), amplified by e^{|s|}
            o64 = z[f"{tag}/out"]
            t64, s64 = o64[:, 0], (np.abs(o64[:, 1]) if kind == "affine" else np.zeros_like(o64[:, 0]))
            bx = CB.EPS32 * ((np.abs(z[f"{tag}/y"]) + np.abs(t64)) * np.exp(s64) + np.abs(z[f"{tag}/x_active"]) * (3 + s64))
            ex = np.abs(xh.detach().double().cpu().numpy().reshape(bx.shape) - z[f"{tag}/x_active"])
            assert (ex <= CB.C_SITE * bx + 1e-30).all(), (tag, layout, "xhat", float((ex / (bx + 1e-30)).max()))
            assert rel(lrt, g("log0")) <= tol["val"], (tag, layout, "logJ_rt")
        if dtype == torch.float64 and kind not in ("multirqs",):
            linv = lrt.mean() + (xh ** 2).mean()
            gy, gp2 = torch.autograd.grad(linv, (yin, params))
            fn = {"affine": O.affine_coupling_atom, "shift": O.shift_coupling_atom}.get(kind, O.rqs_coupling_atom)
            yo = T(z[f"{tag}/y"], dev="cpu").clone().requires_grad_(True)
            oo = T(z[f"{tag}/out"], dev="cpu").clone().requires_grad_(True)
            opts = dict(ATOM_OPTS.get(kind, {}))
            if kind == "rqs_fixedx":
                opts["knots_x"] = T(z[f"{tag}/knots_x"], dev="cpu")
            xo, lo = fn(yo, oo, O.channel_mask(shape, parity), inverse=True, log0=T(z[f"{tag}/logJ"], dev="cpu"), **opts)
            go_y, go_p = torch.autograd.grad(lo.mean() + (xo ** 2).mean(), (yo, oo), allow_unused=True)
            go_p = torch.zeros_like(oo) if go_p is None else go_p
            assert rel(gy[..., keep], go_y.reshape(v.shape).to(DEV)[..., keep]) <= 1e-6, (tag, layout, "inv grad_y")
            gref2 = go_p.reshape(out_full.shape).to(DEV)
            gref2 = compact(gref2, act) if layout == "pair" else gref2
            assert rel(gp2[..., keep_p], gref2[..., keep_p]) <= 1e-6, (tag, layout, "inv grad_p")


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("tag", dc_cases())
def test_distconvertor_against_reference_goldens(golden, tag, dtype):
    z = golden("distconv")
    tol = TOL[dtype]
    sym, smooth = "sym1" in tag, "sm1" in tag
    m = int(tag.split("m")[-1])
    dc = DistConvertor_(m, symmetric=sym, smooth=smooth)
    dc.to(device=DEV, dtype=dtype)
    sp = dc.spline_layer_
    with torch.no_grad():
        sp.weights_x.copy_(T(z[f"{tag}/wx"], dtype))
        sp.weights_y.copy_(T(z[f"{tag}/wy"], dtype))
        if not smooth:
            sp.weights_d.copy_(T(z[f"{tag}/wd"], dtype))
    x = T(z[f"{tag}/x"], dtype).requires_grad_(True)
    y, logJ = dc(x, T(z[f"{tag}/log0"], dtype))
    # fp32: expit/logit lose relative accuracy in the tails |x| >~ 7 (1 - u is not representable);
    # the goldens draw x ~ N(0, 2^2), so a handful of points sit there
    f32 = dtype == torch.float32
    ft = lambda key, base, **kw: floor_tol(z, "distconv", f"{tag}/{key}", base, **kw) if f32 else base
    assert rel(y, z[f"{tag}/y"]) <= ft("y", tol["val"]), ("y", rel(y, z[f"{tag}/y"]), ft("y", tol["val"]))
    assert rel(logJ, z[f"{tag}/logJ"]) <= ft("logJ", tol["val"]), ("logJ", rel(logJ, z[f"{tag}/logJ"]), ft("logJ", tol["val"]))
    loss = logJ.mean() + (y ** 2).mean()
    ps = [sp.weights_x, sp.weights_y] + ([] if smooth else [sp.weights_d])
    grads = torch.autograd.grad(loss, [x] + ps)
    for gr, name in zip(grads, ["grad_x", "grad_wx", "grad_wy", "grad_wd"]):
        gt = ft(name, tol["grad"])
        assert rel(gr, z[f"{tag}/{name}"]) <= gt, (name, rel(gr, z[f"{tag}/{name}"]), gt)
    with torch.no_grad():
        xh, lrt = dc.backward(T(z[f"{tag}/y"], dtype), T(z[f"{tag}/logJ"], dtype))
    xt = ft("xhat", tol["val"], target=z[f"{tag}/x"]) if f32 else 100 * tol["val"]
    lt = ft("logJ_rt", tol["val"], target=z[f"{tag}/log0"]) if f32 else 100 * tol["val"]
    assert rel(xh, z[f"{tag}/x"]) <= xt, ("xhat", rel(xh, z[f"{tag}/x"]), xt)
    assert rel(lrt, z[f"{tag}/log0"]) <= lt, ("logJ_rt", rel(lrt, z[f"{tag}/log0"]), lt)
    if dtype == torch.float64:   # VJP of the inverse chain against autograd through the oracle
        yin = T(z[f"{tag}/y"], dtype).requires_grad_(True)
        xh, lrt = dc.backward(yin, T(z[f"{tag}/logJ"], dtype))
        gi = torch.autograd.grad(lrt.mean() + (xh ** 2).mean(), [yin] + ps)
        c = lambda k: T(z[f"{tag}/{k}"], dev="cpu").clone().requires_grad_(True)
        yo, wx, wy = c("y"), c("wx"), c("wy")
        wd = None if smooth else c("wd")
        xo, lo = O.dist_convertor(yo, wx, wy, wd, symmetric=sym, inverse=True, log0=T(z[f"{tag}/logJ"], dev="cpu"))
        go = torch.autograd.grad(lo.mean() + (xo ** 2).mean(), [yo, wx, wy] + ([] if smooth else [wd]))
        for a, b in zip(gi, go):
            assert rel(a, b) <= 1e-6


def _load_block(z, tag, kind, d, shape, dtype):
    m = 6
    n_out = 2 if kind == "affine" else 3 * m - 2
    nets = [ConvAct(1, n_out, 3, conv_dim=d, hidden_sizes=[4, 4], acts=['tanh', 'tanh', None]) for _ in range(3)]
    mask = EvenOddMask(shape=shape)
    if kind == "affine":
        cpl = AffineCoupling_(nets, mask=mask)
    else:
        cpl = RQSplineCoupling_(nets, mask=mask, xlim=(-3.0, 3.0), ylim=(-3.0, 3.0),
                                extrap={'left': 'linear', 'right': 'linear'})
    sd = {k.split("/param/")[1]: torch.from_numpy(z[k]) for k in z.files if k.startswith(f"{tag}/param/")}
    missing, unexpected = cpl.load_state_dict(sd, strict=False)
    assert not unexpected and set(missing) == {"mask._mask", "mask._c_mask"}
    return cpl.to(device=DEV, dtype=dtype)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("kind", ["affine", "rqs"])
@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_coupling_blocks_with_convact_against_goldens(golden, kind, d, dtype):
    """Module boundary: reference weights in (same state_dict keys), reference y / logJ /
    grads out."""
    z = golden("blocks")
    tag = f"{kind}/d{d}"
    shape = tuple(int(v) for v in z[f"{tag}/shape"])
    cpl = _load_block(z, tag, kind, d, shape, dtype)
    f32 = dtype == torch.float32
    # fp32 at the module boundary (an fp32 conv stack in front of the coupling): the reference's own float32 run of the
    # same block sets the floor, per quantity (ref_fp32.npz); never looser than 2x that, never tighter than 1e-5 / 2e-4
    ft = lambda key, base: floor_tol(z, "blocks", f"{tag}/{key}", base) if f32 else {1e-5: 1e-9, 2e-4: 1e-7}[base]
    x = T(z[f"{tag}/x"], dtype).requires_grad_(True)
    y, logJ = cpl(x)
    assert rel(y, z[f"{tag}/y"]) <= ft("y", 1e-5), ("y", rel(y, z[f"{tag}/y"]), ft("y", 1e-5))
    assert rel(logJ, z[f"{tag}/logJ"]) <= ft("logJ", 1e-5), ("logJ", rel(logJ, z[f"{tag}/logJ"]), ft("logJ", 1e-5))
    loss = logJ.mean() + (y ** 2).mean()
    names = [n for n, _ in cpl.named_parameters()]
    grads = torch.autograd.grad(loss, [x] + [p for _, p in cpl.named_parameters()])
    assert rel(grads[0], z[f"{tag}/grad_x"]) <= ft("grad_x", 2e-4), ("grad_x", rel(grads[0], z[f"{tag}/grad_x"]))
    for n, gp in zip(names, grads[1:]):
        assert rel(gp, z[f"{tag}/gparam/{n}"]) <= ft(f"gparam/{n}", 2e-4), (n, rel(gp, z[f"{tag}/gparam/{n}"]))
    with torch.no_grad():
        xh, lrt = cpl.backward(T(z[f"{tag}/y"], dtype), T(z[f"{tag}/logJ"], dtype))
        if dtype == torch.float64:
            assert rel(xh, z[f"{tag}/x"]) <= 1e-6 and float(lrt.abs().max()) <= 1e-6
        else:
            # these random-init nets reach g ~ 1e-4, so x = f^-1(y) is ill-conditioned in fp32
            # (error ~ 1e-7 / g per layer); the well-conditioned statement is the residual:
            # pushing the recovered x forward again must land on y
            y2, lj2 = cpl(xh)
            assert rel(y2, z[f"{tag}/y"]) <= 1e-4, rel(y2, z[f"{tag}/y"])


def test_c1_readme_model_against_golden(golden):
    z = golden("callers")
    from normflow__amd import Model
    from normflow__amd.prior import NormalPrior
    from normflow__amd.action import ScalarPhi4Action
    for dtype, tol in ((torch.float64, 1e-10), (torch.float32, 1e-5)):
        net_ = DistConvertor_(knots_len=10, symmetric=True)
        net_.to(device=DEV, dtype=dtype)
        sp = net_.spline_layer_
        with torch.no_grad():
            sp.weights_x.copy_(T(z["c1/wx"], dtype))
            sp.weights_y.copy_(T(z["c1/wy"], dtype))
            sp.weights_d.copy_(T(z["c1/wd"], dtype))
        prior = NormalPrior(loc=torch.zeros(1, device=DEV, dtype=dtype), scale=torch.ones(1, device=DEV, dtype=dtype))
        model = Model(net_=net_, prior=prior, action=ScalarPhi4Action(kappa=0, m_sq=-1.2, lambd=0.5))
        x = T(z["c1/x"], dtype)
        y, logJ = net_(x)
        logq = prior.log_prob(x) - logJ
        logp = -model.action(y)
        assert rel(y, z["c1/y"]) <= tol and rel(logJ, z["c1/logJ"]) <= tol
        assert rel(logq, z["c1/logq"]) <= tol and rel(logp, z["c1/logp"]) <= 10 * tol
        assert abs(model.fit.calc_kl_mean(logq, logp).item() - float(z["c1/loss"])) <= 20 * tol
        assert rel(model.posterior.log_prob(T(z["c1/y"], dtype)), z["c1/log_prob"]) <= 50 * tol


def test_readme_training_reaches_analytic_logz():
    """End-to-end statistical KAT: 0-dim phi^4, m^2=-1.2, lambda=0.5,
    log Z = 1.112773; Model.fit() unchanged on the HIP path."""
    from normflow__amd import Model
    from normflow__amd.prior import NormalPrior
    from normflow__amd.action import ScalarPhi4Action
    torch.manual_seed(11)
    net_ = DistConvertor_(knots_len=10, symmetric=True)
    net_.to(device=DEV, dtype=torch.float64)
    prior = NormalPrior(loc=torch.zeros(1, device=DEV, dtype=torch.float64),
                        scale=torch.ones(1, device=DEV, dtype=torch.float64))
    model = Model(net_=net_, prior=prior, action=ScalarPhi4Action(kappa=0, m_sq=-1.2, lambd=0.5))
    model.fit(n_epochs=300, batch_size=512, hyperparam=dict(lr=0.01, weight_decay=0.0),
              checkpoint_dict=dict(print_stride=100, print_batch_size=4096))
    h = model.fit.train_history
    assert abs(h['logz'][-1][0] - 1.112773) < 0.01
    assert h['accept_rate'][-1][0] > 0.85
    assert float(h['ess'][-1]) > 0.9


# ------------------------------------------------------------ seeded oracle comparisons
def _rand_case(shape, B, m, seed, dtype, out_std=0.5, x_std=1.0):
    g = torch.Generator(device='cpu').manual_seed(seed)
    x = x_std * torch.randn((B,) + shape, generator=g, dtype=torch.float64, device='cpu')
    out = out_std * torch.randn((B, 3 * m - 2) + shape, generator=g, dtype=torch.float64, device='cpu')
    return x, out


@pytest.mark.parametrize("m", [2, 3, 4, 8, 10, 16, 24])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_rqs_kernel_vs_oracle_all_m(m, dtype):
    """Register-resident (m = 4, 8, 16) and LDS-column (other m) kernels, both layouts,
    synthetic inputs of SURVEY 8(d): x ~ N(0,1) (scaled to reach the tails), logits ~ N(0, 0.5^2)."""
    shape, B = (6, 4, 8), 5
    tol = TOL[dtype]
    x, out = _rand_case(shape, B, m, 100 + m, dtype, x_std=3.0)
    opts = dict(xlim=(-5.0, 5.0), ylim=(-5.0, 5.0), extrap={'left': 'linear', 'right': 'linear'})
    for parity in (0, 1):
        am = O.channel_mask(shape, parity)
        xa = x * am
        yo, lo = O.rqs_coupling_atom(xa, out, am, **opts)
        act = am.to(torch.uint8).reshape(-1).to(DEV)
        for lay in (_hip.LAYOUT_FULL, _hip.LAYOUT_PAIR):
            full = out.reshape(B, 3 * m - 2, -1).to(DEV, dtype)
            params = compact(full, act) if lay == _hip.LAYOUT_PAIR else full
            o = _hip.make_rqs_opts(m, opts["xlim"], opts["ylim"], opts["extrap"], lay)
            y, lj = _hip.RQSCouplingFn.apply(xa.reshape(B, -1).to(DEV, dtype), params, None, act, o, False)
            assert rel(y.reshape(x.shape), yo) <= tol["val"]
            assert rel(lj, lo) <= tol["val"]
            xb, lb = _hip.RQSCouplingFn.apply(y, params, lj, act, o, True)
            assert rel(xb.reshape(x.shape), xa) <= 50 * tol["val"]
            assert float(lb.abs().max()) <= 50 * tol["val"] * max(1.0, float(lo.abs().max()))


def test_edge_cases_empty_ragged_extreme():
    o = _hip.make_rqs_opts(4, (-1, 1), (-1, 1), {'left': 'linear', 'right': 'linear'}, 0)
    act = torch.ones(7, dtype=torch.uint8, device=DEV)
    # empty batch
    y, lj = _hip.RQSCouplingFn.apply(torch.zeros(0, 7, device=DEV), torch.zeros(0, 10, 7, device=DEV), None, act, o, False)
    assert y.shape == (0, 7) and lj.shape == (0,)
    # odd V (ragged against the 256-thread tile), all-frozen mask => identity-free zeros, logJ = log0
    none = torch.zeros(7, dtype=torch.uint8, device=DEV)
    l0 = torch.arange(3, device=DEV, dtype=torch.float64)
    y, lj = _hip.RQSCouplingFn.apply(torch.randn(3, 7, device=DEV), torch.randn(3, 10, 7, device=DEV), l0, none, o, False)
    assert float(y.abs().max()) == 0.0 and torch.equal(lj, l0)
    # zero logits => identity map inside the limits, log|J| = 0 (softplus_ln2(0) = 1, equal bins)
    x = torch.linspace(-3, 3, 70, device=DEV).reshape(10, 7)
    y, lj = _hip.RQSCouplingFn.apply(x, torch.zeros(10, 10, 7, device=DEV), None, act, o, False)
    assert float((y - x).abs().max()) < 1e-14 and float(lj.abs().max()) < 1e-13
    # extreme logits: huge derivative logit (softplus threshold branch) and very negative one
    p = torch.zeros(1, 10, 7, device=DEV)
    p[:, 6:] = 40.0
    p[:, 7] = -40.0
    y, lj = _hip.RQSCouplingFn.apply(torch.zeros(1, 7, device=DEV) + 0.1, p, None, act, o, False)
    yo, lo = O.rqs_coupling_atom(torch.full((1, 7), 0.1, dtype=torch.float64, device='cpu'), p.cpu(),
                                 torch.ones(7, dtype=torch.float64, device='cpu'), xlim=(-1, 1), ylim=(-1, 1),
                                 extrap={'left': 'linear', 'right': 'linear'})
    assert rel(y, yo) < 1e-9 and rel(lj, lo) < 1e-9
    # batch larger than one grid's y extent is cut into slabs
    Bbig = _hip.MAX_B + 5
    x = torch.randn(Bbig, 2, device=DEV, dtype=torch.float32)
    p = 0.3 * torch.randn(Bbig, 2, 2, device=DEV, dtype=torch.float32)
    a2 = torch.ones(2, dtype=torch.uint8, device=DEV)
    y, lj = _hip.AffineCouplingFn.apply(x, p, None, a2, 0, False)
    assert rel(y, p[:, 0] + x * torch.exp(-p[:, 1].abs())) < 1e-6 and rel(lj, -p[:, 1].abs().sum(1)) < 1e-6
    with pytest.raises(TypeError):                     # no bf16 kernels
        _hip.RQSCouplingFn.apply(torch.zeros(1, 7, device=DEV, dtype=torch.bfloat16),
                                 torch.zeros(1, 10, 7, device=DEV, dtype=torch.bfloat16), None, act, o, False)
    with pytest.raises(_hip.NormflowHipError):         # fp16 storage exists for knots_len 4/8/16 only
        o5 = _hip.make_rqs_opts(5, (-1, 1), (-1, 1), {'left': 'linear', 'right': 'linear'}, _hip.LAYOUT_FULL)
        _hip.RQSCouplingFn.apply(torch.zeros(1, 7, device=DEV, dtype=torch.float16),
                                 torch.zeros(1, 13, 7, device=DEV, dtype=torch.float16), None, act, o5, False)


# -------------------------------------------------- BASELINE sizes: size-independent properties
def _big_properties(shape, B, m, dtype):
    V = int(np.prod(shape))
    torch.manual_seed(5)
    mask = EvenOddMask(shape=shape)
    act = mask.activity(0).reshape(-1).to(DEV)
    x = torch.randn(B, V, device=DEV, dtype=dtype)
    xa = x * act.to(dtype)
    pc = 0.5 * torch.randn(B, 3 * m - 2, V // 2, device=DEV, dtype=dtype)
    lim = dict(xlim=(-5.0, 5.0), ylim=(-5.0, 5.0), extrap={'left': 'linear', 'right': 'linear'})
    op = _hip.make_rqs_opts(m, lim["xlim"], lim["ylim"], lim["extrap"], _hip.LAYOUT_PAIR)
    of = _hip.make_rqs_opts(m, lim["xlim"], lim["ylim"], lim["extrap"], _hip.LAYOUT_FULL)
    y, lj = _hip.RQSCouplingFn.apply(xa, pc, None, act, op, False)
    # (1) frozen sites are exactly zero, active sites finite and monotone-consistent
    assert float((y * (1 - act.to(dtype))).abs().max()) == 0.0 and bool(torch.isfinite(y).all())
    # (2) round trip: inverse(forward) = id and the log-Jacobians cancel
    xb, lb = _hip.RQSCouplingFn.apply(y, pc, lj, act, op, True)
    scale = max(1.0, float(lj.abs().max()))
    rt = (1e-10, 1e-9) if dtype == torch.float64 else (2e-4, 2e-5)
    assert float((xb - xa).abs().max()) <= rt[0] * 50
    assert float(lb.abs().max()) <= rt[1] * scale * 50
    # (3) pair layout == full layout (same arithmetic, different addressing)
    nsub = min(B, 2)
    yf, ljf = _hip.RQSCouplingFn.apply(xa[:nsub], uncompact(pc[:nsub], act), None, act, of, False)
    assert rel(yf, y[:nsub]) <= (1e-14 if dtype == torch.float64 else 1e-6)
    assert rel(ljf, lj[:nsub]) <= (1e-12 if dtype == torch.float64 else 1e-6)
    # (4) samples are independent: a permuted batch gives the permuted result, bitwise
    perm = torch.randperm(B, device=DEV)
    yp, ljp = _hip.RQSCouplingFn.apply(xa[perm], pc[perm], None, act, op, False)
    assert torch.equal(yp, y[perm]) and torch.equal(ljp, lj[perm])
    # (5) one sample against the fp64 CPU oracle
    am = O.channel_mask(shape, 0)
    yo, lo = O.rqs_coupling_atom(xa[:1].double().cpu().reshape((1,) + shape),
                                 uncompact(pc[:1], act).double().cpu().reshape((1, 3 * m - 2) + shape), am, **lim)
    assert rel(y[:1].reshape((1,) + shape), yo) <= TOL[dtype]["val"]
    assert rel(lj[:1], lo) <= TOL[dtype]["val"]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_config3_full_size_properties(dtype):
    """BASELINE config 3: 16^3, m=16, batch 1024."""
    _big_properties((16, 16, 16), 1024, 16, dtype)


def test_config4_full_lattice_properties():
    """BASELINE config 4 lattice (32^4, m=16) at the per-GPU kernel slab that bench.py uses."""
    _big_properties((32, 32, 32, 32), 8, 16, torch.float32)


def _network_properties(shape, B, kinds, m=16):
    """Whole coupling blocks on a full-size lattice through the package API (ConvAct nets on the MFMA kernels,
    fused last layer under no_grad): size-independent properties -- fused inference == the differentiable
    (unfused) path, inverse(forward) = id with cancelling log-Jacobians, samples independent (bitwise)."""
    torch.manual_seed(9)
    d = len(shape)
    dt = torch.float32
    mask = EvenOddMask(shape=shape)
    lim = dict(xlim=(-5.0, 5.0), ylim=(-5.0, 5.0), extrap={'left': 'linear', 'right': 'linear'})
    blocks = []
    for kind in kinds:
        C = 3 * m - 2 if kind == 'rqs' else 2
        nets = [ConvAct(1, C, 3, conv_dim=d, hidden_sizes=[8, 8], acts=['tanh', 'tanh', None]) for _ in range(2)]
        for net in nets:
            with torch.no_grad():
                for p in list(net.parameters())[-2:]:
                    p.mul_(0.3)
        blocks.append(RQSplineCoupling_(nets, mask=mask, **lim) if kind == 'rqs' else AffineCoupling_(nets, mask=mask))
    net_ = ModuleList_(blocks)
    net_.to(device=DEV, dtype=dt)
    x = torch.randn((B,) + shape, device=DEV, dtype=dt)
    with torch.no_grad():
        y, lj = net_(x)
        xb, lb = net_.backward(y, lj)
        perm = torch.randperm(B, device=DEV)
        yp, ljp = net_(x[perm])
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(lj).all())
    assert rel(xb, x) <= 2e-4 and float(lb.abs().max()) <= 2e-5 * max(1.0, float(lj.abs().max())) * 50
    assert torch.equal(yp, y[perm]) and torch.equal(ljp, lj[perm])
    y2, lj2 = net_(x[:1].clone().requires_grad_(True))        # differentiable path: logits materialised, K2 kernel
    # (the fused path runs split-fp16 products in all three conv layers, the differentiable path fp32 ones: two roundings of
    #  the same exact result, each within north_star's 1e-5 of the fp64 oracle -- see the per-kernel tests -- so within 2e-5
    #  of each other)
    assert rel(y2, y[:1]) <= 2e-5 and rel(lj2, lj[:1]) <= 1e-5, (rel(y2, y[:1]), rel(lj2, lj[:1]))


def test_config4_network_properties():
    """BASELINE config 4 blocks (32^4, RQ-spline m=16, ConvAct 1-8-8-46) at a small batch."""
    _network_properties((32, 32, 32, 32), 3, ['rqs', 'rqs'])


def test_config5_lattice_network_properties():
    """BASELINE config 5 lattice (48^4 -- not a power of two: clipped boxes, narrow staging) with mixed
    affine + spline blocks, fp32."""
    _network_properties((48, 48, 48, 48), 2, ['affine', 'rqs'])


def test_posterior_sample_and_sanity_on_lattice():
    """Model.posterior.sample / log_prob / backward_sanitychecker unchanged on a 2-D lattice
    with mixed blocks (BASELINE config 2 shapes: 16x16, affine)."""
    from normflow__amd import Model, backward_sanitychecker
    from normflow__amd.prior import NormalPrior
    from normflow__amd.action import ScalarPhi4Action
    torch.manual_seed(3)
    shape = (16, 16)
    dt = torch.float64
    mask = EvenOddMask(shape=shape)
    mk = lambda c: ConvAct(1, c, 3, conv_dim=2, hidden_sizes=[8, 8], acts=['tanh', 'tanh', None])
    net_ = ModuleList_([AffineCoupling_([mk(2) for _ in range(4)], mask=mask),
                        RQSplineCoupling_([mk(22) for _ in range(2)], mask=mask, xlim=(-5, 5), ylim=(-5, 5),
                                          extrap={'left': 'linear', 'right': 'linear'}),
                        ShiftCoupling_([mk(1)], mask=mask),
                        DistConvertor_(8, symmetric=True)])
    net_.to(device=DEV, dtype=dt)
    prior = NormalPrior(loc=torch.zeros(shape, device=DEV, dtype=dt), scale=torch.ones(shape, device=DEV, dtype=dt))
    model = Model(net_=net_, prior=prior, action=ScalarPhi4Action(kappa=0.67, m_sq=-4 * 0.67, lambd=0.5))
    y, logq, logp = model.posterior.sample__(512)
    assert y.shape == (512,) + shape and bool(torch.isfinite(logq).all())
    assert rel(model.posterior.log_prob(y), logq) < 1e-8
    (x, yy, xh), (lj, l0) = backward_sanitychecker(model, n_samples=5, return_details=True)
    assert float((x - xh).abs().sum()) < 1e-8 and float(l0.abs().sum()) < 1e-8
    model.fit(n_epochs=3, batch_size=64, checkpoint_dict=dict(print_stride=1, print_batch_size=64))
    assert np.isfinite(model.fit.train_history['loss']).all()


# ------------------------------------------------------------------ K5: MFMA circular conv
CONV_CASES = [
    # (lattice, cin, cout, ksize, act)
    ((8,), 1, 8, 3, 'tanh'), ((6,), 3, 2, 3, None), ((5,), 2, 5, 5, 'relu'),
    ((6, 4), 1, 8, 3, 'tanh'), ((16, 16), 8, 2, 3, None), ((3, 5), 4, 46, 3, 'leaky_relu'), ((2, 2), 1, 3, 3, None),
    ((4, 6, 4), 8, 8, 3, 'tanh'), ((16, 16, 16), 8, 46, 3, None), ((4, 4, 10), 5, 17, 3, 'softplus'),
    ((4, 4, 2, 6), 1, 8, 3, 'tanh'), ((8, 8, 8, 8), 8, 46, 3, None), ((4, 2, 4, 4), 8, 70, 3, 'abs'),
    ((6, 6, 6, 12), 8, 8, 3, 'tanh'), ((4, 4, 4, 64), 2, 4, 3, None),
    # many input channels: the K loop runs in channel chunks that fit LDS (and odd counts >= 8 are zero-padded)
    ((8, 8, 8, 8), 48, 8, 3, None), ((4, 4, 4, 8), 46, 5, 3, 'tanh'), ((16, 16), 22, 3, 3, None), ((6, 8, 8), 10, 12, 3, None),
]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("lattice,cin,cout,k,act", CONV_CASES)
def test_conv_kernel_vs_oracle(lattice, cin, cout, k, act, dtype):
    """fp32 MFMA kernel vs the fp64 definition (oracle circular_conv_direct); fp32 products and
    accumulation over K = taps*cin terms: error ~ 1e-7 * sum|a b| (guide: 0.75-1.5e-7 at K<=1024)."""
    d = len(lattice)
    g = torch.Generator(device='cpu').manual_seed(hash((lattice, cin, cout)) % 1000)
    B = 3
    x = torch.randn((B, cin) + lattice, generator=g, dtype=torch.float64, device='cpu')
    w = 0.3 * torch.randn((cout, cin) + (k,) * d, generator=g, dtype=torch.float64, device='cpu')
    b = torch.randn(cout, generator=g, dtype=torch.float64, device='cpu')
    ref = O._ACTS[act](O.circular_conv_direct(x, w, b))
    xd, wd, bd = (t.to(DEV, dtype) for t in (x, w, b))
    out = _hip.conv_layer(xd, wd, bd, _hip.ACT_CODES[act])
    assert out.shape == ref.shape and out.dtype == dtype
    tol = 1e-6 + 2e-7 * 0.3 * cin * k ** d        # ~ eps_f32 * sum|a b| over K = cin * k^d terms
    if dtype == torch.float64:                    # v_mfma_f64_16x16x4_f64
        tol = 1e-12
    assert rel(out, ref) <= tol
    out_nb = _hip.conv_layer(xd, wd, None, 0)
    assert rel(out_nb, O.circular_conv_direct(x, w, None)) <= tol
    if lattice[-1] % 2 == 0:
        for parity in (0, 1):
            act_mask = (O.even_odd_mask(lattice, parity=0) == (1 - parity)).reshape(-1).to(DEV)   # coord sum % 2 == parity
            comp = _hip.conv_layer(xd, wd, bd, _hip.ACT_CODES[act], compact=True, parity=parity)
            want = compact(T(ref.reshape(B, cout, -1).numpy(), torch.float64), act_mask.to(torch.uint8))
            assert comp.shape == want.shape and rel(comp, want) <= tol


def test_convact_fused_matches_torch_path_and_grads():
    """ConvAct on the MFMA kernel == the same module evaluated with torch ops (fp64), forward and
    gradients (the kernel's VJP is the torch-op restatement); pair-compact output feeds the
    coupling kernel with the same result as the full layout."""
    torch.manual_seed(21)
    shape = (4, 4, 4, 8)
    net = ConvAct(1, 22, 3, conv_dim=4, hidden_sizes=[8, 8], acts=['tanh', 'tanh', None]).to(DEV, torch.float32)
    x = torch.randn((5, 1) + shape, device=DEV, dtype=torch.float32, requires_grad=True)
    y = net(x)
    net64 = ConvAct(1, 22, 3, conv_dim=4, hidden_sizes=[8, 8], acts=['tanh', 'tanh', None]).to(DEV, torch.float64)
    net64.load_state_dict({k: v.double() for k, v in net.state_dict().items()})
    x64 = x.detach().double().requires_grad_(True)
    y64 = net64(x64)
    assert rel(y, y64) <= 1e-5
    gy = torch.randn_like(y)
    grads = torch.autograd.grad(y, [x] + list(net.parameters()), gy)
    grads64 = torch.autograd.grad(y64, [x64] + list(net64.parameters()), gy.double())
    for a, b in zip(grads, grads64):
        assert rel(a, b) <= 1e-4
    mask = EvenOddMask(shape=shape)
    cpl = RQSplineCoupling_([net], mask=mask, xlim=(-5, 5), ylim=(-5, 5), extrap={'left': 'linear', 'right': 'linear'})
    cpl.to(DEV)
    xf = torch.randn((5,) + shape, device=DEV, dtype=torch.float32)
    with torch.no_grad():
        p_pair, lay = cpl._params(net, mask.purify(xf, 1), parity=0)
        assert lay == _hip.LAYOUT_PAIR and p_pair.shape == (5, 22, 256)
        p_full = net(mask.purify(xf, 1).unsqueeze(1)).reshape(5, 22, -1)
        assert rel(p_pair, compact(p_full, mask.activity(0).reshape(-1).to(DEV))) <= 1e-6
        y1, l1 = cpl(xf)
        cpl64 = RQSplineCoupling_([net64], mask=EvenOddMask(shape=shape), xlim=(-5, 5), ylim=(-5, 5),
                                  extrap={'left': 'linear', 'right': 'linear'}).to(DEV)
        y2, l2 = cpl64(xf.double())
    assert rel(y1, y2) <= 1e-5 and rel(l1, l2) <= 1e-5


def test_fixed_knots_module_level_vs_oracle():
    """RQSplineCoupling_(knots_x=..., knots_y=...) variants (couplings_.py:236-256): x fixed,
    y fixed, both fixed -- module API against the oracle, fp64 and fp32, forward + inverse."""
    torch.manual_seed(9)
    shape, B, m = (6, 4), 4, 5
    kx = torch.tensor([-2.0, -0.7, 0.1, 0.9, 2.0], dtype=torch.float64, device='cpu')
    ky = torch.tensor([-2.0, -1.1, -0.2, 1.2, 2.0], dtype=torch.float64, device='cpu')
    for fx, fy, C in ((kx, None, 2 * m - 1), (None, ky, 2 * m - 1), (kx, ky, m)):
        for dtype in (torch.float64, torch.float32):
            net = ConvAct(1, C, 3, conv_dim=2, hidden_sizes=[4], acts=['tanh', None]).to(DEV, dtype)
            mask = EvenOddMask(shape=shape)
            cpl = RQSplineCoupling_([net], mask=mask, xlim=(-2.0, 2.0), ylim=(-2.0, 2.0), knots_x=fx, knots_y=fy,
                                    extrap={'left': 'linear', 'right': 'linear'}).to(DEV)
            x = 1.5 * torch.randn((B,) + shape, device=DEV, dtype=dtype)
            with torch.no_grad():
                y, lj = cpl(x)
                xb, lb = cpl.backward(y, lj)
                convs = [mod for mod in net if hasattr(mod, 'weight')]
                layers = [(c.weight.double().cpu(), c.bias.double().cpu()) for c in convs]
                yo, lo = O.coupling_block(x.double().cpu(), [lambda t: O.conv_act(t, layers, ['tanh', None])], 'rqs',
                                          shape, xlim=(-2.0, 2.0), ylim=(-2.0, 2.0), knots_x=fx, knots_y=fy,
                                          extrap={'left': 'linear', 'right': 'linear'})
            tol = 1e-9 if dtype == torch.float64 else 2e-5
            assert rel(y, yo) <= tol and rel(lj, lo) <= tol
            assert rel(xb, x) <= 100 * tol and float(lb.abs().max()) <= 100 * tol


@pytest.mark.parametrize("m,shape", [(16, (4, 4, 4, 8)), (8, (6, 8)), (4, (4, 6, 4)), (16, (16, 16, 16)), (16, (10,))])
def test_fused_conv_spline_epilogue_matches_unfused(m, shape):
    """nf_conv_rqs (logits accumulator -> LDS -> spline, never in HBM) == conv kernel + coupling
    kernel run separately (same fp32 arithmetic: tight), and == the fp64 oracle within 1e-5;
    forward and inverse; clipped boxes (lattices smaller than / not dividing the box)."""
    torch.manual_seed(m + len(shape))
    d = len(shape)
    C = 3 * m - 2
    net = ConvAct(1, C, 3, conv_dim=d, hidden_sizes=[8, 8], acts=['tanh', 'tanh', None]).to(DEV, torch.float32)
    with torch.no_grad():
        for p in list(net.parameters())[-2:]:
            p.mul_(0.3)
    mask = EvenOddMask(shape=shape)
    lim = dict(xlim=(-4.0, 4.0), ylim=(-4.0, 4.0), extrap={'left': 'linear', 'right': 'linear'})
    cpl = RQSplineCoupling_([net, net], mask=mask, **lim).to(DEV)
    x = 1.5 * torch.randn((5,) + shape, device=DEV, dtype=torch.float32)
    for parity in (0, 1):
        xa, xf = mask.purify(x, parity), mask.purify(x, 1 - parity)
        l0 = torch.randn(5, device=DEV, dtype=torch.float32)
        with torch.no_grad():
            yf, lf = cpl._fused_atom(False, xa, xf, parity, net, l0)
            params, lay = cpl._params(net, xf, parity)
            opts = _hip.make_rqs_opts(m, lim["xlim"], lim["ylim"], lim["extrap"], lay)
            act = mask.activity(parity).reshape(-1).to(DEV)
            yu, lu = _hip.RQSCouplingFn.apply(xa.reshape(5, -1), params, l0, act, opts, False)
            assert rel(yf.reshape(5, -1), yu) <= 2e-6 and rel(lf, lu) <= 2e-6
            check_fused_round_trip(cpl, net, ['tanh', 'tanh', None], xa, xf, yf, lf, l0, parity, shape, lim, nb=5)
        convs = [mod for mod in net if hasattr(mod, 'weight')]
        layers = [(c.weight.detach().double().cpu(), c.bias.detach().double().cpu()) for c in convs]
        out = O.conv_act(xf.double().cpu().unsqueeze(1), layers, ['tanh', 'tanh', None])
        yo, lo = O.rqs_coupling_atom(xa.double().cpu(), out, O.channel_mask(shape, parity), log0=l0.double().cpu(), **lim)
        assert rel(yf, yo) <= 1e-5 and rel(lf, lo) <= 1e-5
    # the block-level API takes the fused path under no_grad and the differentiable path otherwise
    with torch.no_grad():
        y1, l1 = cpl(x)
    y2, l2 = cpl(x.clone().requires_grad_(True))
    assert rel(y1, y2) <= 2e-6 and rel(l1, l2) <= 2e-6


PIPE_CASES = [
    # (lattice, cin, cout, B): eligible for the persistent staging-overlapped kernel (fp32, cin % 4 == 0, k = 3);
    # B chosen so that workgroups walk several (sample, box) items and both LDS buffers change hands
    ((8, 8, 8, 16), 8, 46, 40), ((8, 8, 8, 16), 8, 8, 40), ((6, 4, 6, 12), 4, 20, 150), ((8, 8, 8, 8), 12, 8, 70),
    ((8, 16, 32), 8, 30, 24), ((16, 16), 8, 46, 300),
]


@pytest.mark.parametrize("lattice,cin,cout,B", PIPE_CASES)
def test_conv_pipelined_kernel_vs_oracle(lattice, cin, cout, B):
    """nf_conv_pipe.hip (persistent workgroups, double-buffered LDS, staging carried by the MFMA loop)
    against the fp64 definition, full and pair-compact outputs, many items per workgroup; the test
    also asserts that this kernel is the one that ran."""
    d = len(lattice)
    g = torch.Generator(device='cpu').manual_seed(7 + cin + cout)
    x = torch.randn((B, cin) + lattice, generator=g, dtype=torch.float64, device='cpu')
    w = 0.3 * torch.randn((cout, cin) + (3,) * d, generator=g, dtype=torch.float64, device='cpu')
    b = torch.randn(cout, generator=g, dtype=torch.float64, device='cpu')
    ref = torch.tanh(O.circular_conv_fast(x, w, b))
    xd, wd, bd = (t.to(DEV, torch.float32) for t in (x, w, b))
    tol = 1e-6 + 2e-7 * 0.3 * cin * 3 ** d
    out = _hip.conv_layer(xd, wd, bd, _hip.ACT_CODES['tanh'])
    assert _hip.load().nf_conv_last_path() == 1
    assert rel(out, ref) <= tol
    for parity in (0, 1):
        act_mask = (O.even_odd_mask(lattice, parity=0) == (1 - parity)).reshape(-1).to(DEV)
        comp = _hip.conv_layer(xd, wd, bd, _hip.ACT_CODES['tanh'], compact=True, parity=parity)
        assert _hip.load().nf_conv_last_path() == 1
        want = compact(T(ref.reshape(B, cout, -1).numpy(), torch.float64), act_mask.to(torch.uint8))
        assert comp.shape == want.shape and rel(comp, want) <= tol


C1_CASES = [
    # (lattice, cout, B, act): single input channel, <= 8 output channels, whole-row boxes (L3 in {8,16,32,64})
    ((8, 8, 8, 32), 8, 12, 'tanh'), ((4, 4, 4, 8), 8, 40, 'tanh'), ((6, 4, 6, 16), 5, 30, None),
    ((8, 8, 16), 8, 70, 'tanh'), ((12, 32), 3, 50, 'relu'), ((32, 32), 8, 600, 'tanh'),
]


@pytest.mark.parametrize("lattice,cout,B,act", C1_CASES)
def test_conv_first_layer_kernel_vs_oracle(lattice, cout, B, act):
    """conv_c1_kernel (first ConvAct layer: the four fastest-axis taps of a site pair are the K of one MFMA,
    weights in registers, persistent workgroups, LDS-transposed row stores) against the fp64 definition;
    asserts that this kernel ran."""
    d = len(lattice)
    g = torch.Generator(device='cpu').manual_seed(3 + cout + d)
    x = torch.randn((B, 1) + lattice, generator=g, dtype=torch.float64, device='cpu')
    w = 0.3 * torch.randn((cout, 1) + (3,) * d, generator=g, dtype=torch.float64, device='cpu')
    b = torch.randn(cout, generator=g, dtype=torch.float64, device='cpu')
    ref = O._ACTS[act](O.circular_conv_fast(x, w, b))
    xd, wd, bd = (t.to(DEV, torch.float32) for t in (x, w, b))
    out = _hip.conv_layer(xd, wd, bd, _hip.ACT_CODES[act])
    assert _hip.load().nf_conv_last_path() == 2
    tol = 1e-6 + 2e-7 * 0.3 * 3 ** d               # fp32 products and accumulation over 3^d taps
    assert out.shape == ref.shape and rel(out, ref) <= tol
    out_nb = _hip.conv_layer(xd, wd, None, 0)
    assert rel(out_nb, O.circular_conv_fast(x, w, None)) <= tol


def test_fused_epilogue_on_pipelined_kernel_multi_item():
    """nf_conv_rqs through the persistent kernel with several items per workgroup (the epilogue borrows
    the LDS buffer that the next phase is about to be staged into): vs conv + coupling kernels run
    separately and vs the fp64 oracle; forward and inverse."""
    torch.manual_seed(11)
    shape, m, B = (8, 8, 8, 16), 16, 48
    C = 3 * m - 2
    net = ConvAct(1, C, 3, conv_dim=4, hidden_sizes=[8, 8], acts=['tanh', 'tanh', None]).to(DEV, torch.float32)
    with torch.no_grad():
        for p in list(net.parameters())[-2:]:
            p.mul_(0.3)
    mask = EvenOddMask(shape=shape)
    lim = dict(xlim=(-4.0, 4.0), ylim=(-4.0, 4.0), extrap={'left': 'linear', 'right': 'linear'})
    cpl = RQSplineCoupling_([net, net], mask=mask, **lim).to(DEV)
    x = 1.5 * torch.randn((B,) + shape, device=DEV, dtype=torch.float32)
    for parity in (0, 1):
        xa, xf = mask.purify(x, parity), mask.purify(x, 1 - parity)
        l0 = torch.randn(B, device=DEV, dtype=torch.float32)
        with torch.no_grad():
            yf, lf = cpl._fused_atom(False, xa, xf, parity, net, l0)
            assert _hip.load().nf_conv_last_path() == 1
            params, lay = cpl._params(net, xf, parity)
            opts = _hip.make_rqs_opts(m, lim["xlim"], lim["ylim"], lim["extrap"], lay)
            act = mask.activity(parity).reshape(-1).to(DEV)
            yu, lu = _hip.RQSCouplingFn.apply(xa.reshape(B, -1), params, l0, act, opts, False)
            assert rel(yf.reshape(B, -1), yu) <= 2e-6 and rel(lf, lu) <= 2e-6
            check_fused_round_trip(cpl, net, ['tanh', 'tanh', None], xa, xf, yf, lf, l0, parity, shape, lim)
        if parity == 0:
            convs = [mod for mod in net if hasattr(mod, 'weight')]
            layers = [(c.weight.detach().double().cpu(), c.bias.detach().double().cpu()) for c in convs]
            nb = 6                                  # the oracle on a few samples is enough here
            out = O.conv_act(xf[:nb].double().cpu().unsqueeze(1), layers, ['tanh', 'tanh', None])
            yo, lo = O.rqs_coupling_atom(xa[:nb].double().cpu(), out, O.channel_mask(shape, parity),
                                         log0=l0[:nb].double().cpu(), **lim)
            assert rel(yf[:nb], yo) <= 1e-5 and rel(lf[:nb], lo) <= 1e-5


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_endpoint_kernels_against_goldens(golden, dtype):
    """phi^4 action and normal-prior log-density kernels vs the reference's values (callers.npz),
    and their VJPs vs autograd through the oracle."""
    from normflow__amd.action import ScalarPhi4Action
    from normflow__amd.prior import NormalPrior
    z = golden("callers")
    kap, msq, lam = (float(v) for v in z["phi4/coef"])
    act = ScalarPhi4Action(kappa=kap, m_sq=msq, lambd=lam)
    tol = 1e-12 if dtype == torch.float64 else 2e-6
    for d in (1, 2, 3, 4):
        cfg = T(z[f"phi4/d{d}/cfg"], dtype).requires_grad_(True)
        S = act(cfg)
        assert rel(S, z[f"phi4/d{d}/S"]) <= tol
        shape = cfg.shape[1:]
        prior = NormalPrior(loc=torch.zeros(shape, device=DEV, dtype=dtype), scale=torch.ones(shape, device=DEV, dtype=dtype))
        lp = prior.log_prob(cfg)
        assert rel(lp, z[f"phi4/d{d}/logr"]) <= tol
        w = torch.linspace(0.5, 1.5, cfg.shape[0], device=DEV, dtype=dtype)
        g1, = torch.autograd.grad((S * w).sum() + (lp * w).sum(), cfg)
        co = T(z[f"phi4/d{d}/cfg"], dev="cpu").requires_grad_(True)
        wo = w.double().cpu()
        ref = (O.phi4_action(co, kappa=kap, m_sq=msq, lambd=lam) * wo).sum() + (O.normal_log_prob(co) * wo).sum()
        g0, = torch.autograd.grad(ref, co)
        assert rel(g1, g0) <= 100 * tol
    # general loc / scale
    g = torch.Generator(device='cpu').manual_seed(3)
    loc = torch.randn(6, 4, generator=g, device='cpu', dtype=torch.float64)
    sc = 0.5 + torch.rand(6, 4, generator=g, device='cpu', dtype=torch.float64)
    x = torch.randn(7, 6, 4, generator=g, device='cpu', dtype=torch.float64)
    ref = torch.distributions.Normal(loc, sc).log_prob(x).sum(dim=(1, 2))
    pr = NormalPrior(loc=loc.to(DEV, dtype), scale=sc.to(DEV, dtype))
    assert rel(pr.log_prob(x.to(DEV, dtype)), ref) <= 10 * tol


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("lattice,cin,cout,act", [((4, 4, 4, 8), 8, 46, None), ((4, 4, 4, 8), 1, 8, 'tanh'),
                                                  ((6, 8), 8, 8, 'tanh'), ((10,), 3, 5, 'softplus'),
                                                  ((4, 6, 4), 8, 22, 'leaky_relu'), ((8, 8, 8, 8), 8, 50, 'relu'),
                                                  ((6, 4), 2, 2, 'abs'), ((3, 5), 4, 3, 'expit')])
def test_conv_vjp_kernels_vs_autograd(lattice, cin, cout, act, dtype):
    """ConvFn.backward (nf_act_vjp + nf_conv_fwd with flipped weights + nf_conv_wgrad) against
    autograd through the fp64 oracle convolution; also the pair-compact output mode."""
    d = len(lattice)
    g = torch.Generator(device='cpu').manual_seed(cin * 100 + cout)
    x = torch.randn((3, cin) + lattice, generator=g, dtype=torch.float64, device='cpu')
    w = 0.3 * torch.randn((cout, cin) + (3,) * d, generator=g, dtype=torch.float64, device='cpu')
    b = torch.randn(cout, generator=g, dtype=torch.float64, device='cpu')
    go = torch.randn((3, cout) + lattice, generator=g, dtype=torch.float64, device='cpu')
    xo, wo, bo = (t.clone().requires_grad_(True) for t in (x, w, b))
    ref = O._ACTS[act](O.circular_conv_direct(xo, wo, bo))
    gref = torch.autograd.grad(ref, (xo, wo, bo), go, retain_graph=True)
    xd, wd, bd = (t.to(DEV, dtype).requires_grad_(True) for t in (x, w, b))
    out = _hip.conv_layer(xd, wd, bd, _hip.ACT_CODES[act])
    got = torch.autograd.grad(out, (xd, wd, bd), go.to(DEV, dtype))
    tol = 1e-10 if dtype == torch.float64 else 2e-5
    for a_, r_ in zip(got, gref):
        assert rel(a_, r_) <= tol * max(1.0, float(r_.abs().max()) ** 0)
    if lattice[-1] % 2 == 0 and act != 'abs':
        act_mask = (O.even_odd_mask(lattice, parity=0) == 1).reshape(-1)          # coordinate sum even
        outc = _hip.conv_layer(xd, wd, bd, _hip.ACT_CODES[act], compact=True, parity=0)
        goc = compact(go.reshape(3, cout, -1).to(DEV, dtype), act_mask.to(torch.uint8).to(DEV))
        gotc = torch.autograd.grad(outc, (xd, wd, bd), goc)
        gom = go * act_mask.reshape((1, 1) + lattice).double()
        grefc = torch.autograd.grad(ref, (xo, wo, bo), gom)
        for a_, r_ in zip(gotc, grefc):
            assert rel(a_, r_) <= tol


PSD_CASES = [
    ("psd2d", (8, 8), dict(knots_len=6, symmetric=True, final_scale=True, smooth=True), dict(knots_len=5, ignore_zeromode=True)),
    ("psd3d", (4, 6, 4), dict(knots_len=4, symmetric=False, smooth=False), dict(knots_len=4, ignore_zeromode=False)),
    ("psd1d_odd", (9,), dict(knots_len=5, symmetric=True, smooth=True),
     dict(knots_len=1, ignore_zeromode=True, eff_mass2=0.7, eff_kappa=1.3, a=0.5)),
]


@pytest.mark.parametrize("tag,shape,mfdict,fftdict", PSD_CASES)
def test_spectral_block_against_goldens(golden, tag, shape, mfdict, fftdict):
    """PSDBlock_ = MeanFieldNet_ + FFTNet_ vs the reference's outputs (tests/golden/psd.npz,
    generated by make_golden_psd.py): state_dict keys, k^2 grid, inverse PSD, forward (y, log J), gradients
    w.r.t. the input and every parameter, and the inverse.  On an odd fastest axis the reference's irfftn
    returns N-1 sites (a defect: no `s=`); there only the pieces that are well defined are compared."""
    from normflow__amd.nn import FFTNet_, MeanFieldNet_, PSDBlock_
    z = golden("psd")
    dtype = torch.float64
    blk = PSDBlock_(mfnet_=MeanFieldNet_.build(**mfdict), fftnet_=FFTNet_.build(shape, **fftdict)).to(DEV, dtype)
    keys = [k[len(tag) + 7:] for k in z.files if k.startswith(tag + "/state/")]
    assert list(blk.state_dict().keys()) == keys
    assert rel(blk.fftnet_.norm_lat_k2, T(z[tag + "/k2norm"], dtype)) <= 1e-14
    assert abs(float(blk.fftnet_.max_lat_k2) - float(z[tag + "/k2max"])) <= 1e-12
    blk.load_state_dict({k: T(z[f"{tag}/state/{k}"], dtype) for k in keys})
    assert rel(blk.fftnet_.ipsd, T(z[tag + "/ipsd"], dtype)) <= 1e-10
    assert abs(float(blk.fftnet_.infrared_mass) - float(z[tag + "/ir_mass"])) <= 1e-12
    odd = shape[-1] % 2 == 1
    for part, net in (("", blk), ("_fft", blk.fftnet_), ("_mf", blk.mfnet_)):
        x = T(z[f"{tag}{part}/x"], dtype).requires_grad_(True)
        l0 = T(z[f"{tag}{part}/log0"], dtype)
        y, lj = net.forward(x, l0)
        assert rel(lj, T(z[f"{tag}{part}/logJ"], dtype)) <= 1e-10
        if odd and part != "_mf":
            continue
        assert rel(y, T(z[f"{tag}{part}/y"], dtype)) <= 1e-10
        loss = lj.mean() + (y ** 2).mean()
        names = [n for n, _ in net.named_parameters()]
        grads = torch.autograd.grad(loss, [x] + [p for _, p in net.named_parameters()])
        assert rel(grads[0], T(z[f"{tag}{part}/grad_x"], dtype)) <= 1e-9
        for n, gp in zip(names, grads[1:]):
            want = T(z[f"{tag}{part}/grad/{n}"], dtype)
            assert float((gp - want).abs().max()) <= 1e-9 * max(1.0, float(want.abs().max())), n
        with torch.no_grad():
            xb, lb = net.backward(y.detach(), lj.detach())
        assert rel(xb, T(z[f"{tag}{part}/xb"], dtype)) <= 1e-9 and rel(xb, x.detach()) <= 1e-9
        assert float((lb - l0).abs().max()) <= 1e-9


def test_example_network_assembles_and_trains():
    """The network of examples/scalar_affine.py (PSDBlock_, DistConvertor_, AffineCoupling_ with ConvAct nets,
    DistConvertor_) built from this package's names: round trip, and a few epochs of Model.fit lower the loss."""
    import normflow__amd as nf
    from normflow__amd.nn import (FFTNet_, MeanFieldNet_, PSDBlock_, DistConvertor_, AffineCoupling_, ConvAct,
                                  ModuleList_)
    from normflow__amd.prior import NormalPrior
    from normflow__amd.action import ScalarPhi4Action
    torch.manual_seed(5)
    lat = (8, 8)
    nets = [PSDBlock_(mfnet_=MeanFieldNet_.build(knots_len=10, symmetric=True, final_scale=True, smooth=True),
                      fftnet_=FFTNet_.build(lat, knots_len=10, ignore_zeromode=True)),
            DistConvertor_(50, symmetric=True, smooth=True),
            AffineCoupling_([ConvAct(in_channels=1, out_channels=2, hidden_sizes=[8, 8], kernel_size=3, conv_dim=2,
                                     acts=('tanh', 'tanh', None), bias=False) for _ in range(4)],
                            mask=EvenOddMask(shape=lat)),
            DistConvertor_(50, symmetric=True, smooth=True)]
    net_ = ModuleList_(nets)
    net_.to(device=DEV, dtype=torch.float64)
    prior = NormalPrior(loc=torch.zeros(lat, device=DEV, dtype=torch.float64),
                        scale=torch.ones(lat, device=DEV, dtype=torch.float64))
    model = nf.Model(net_=net_, prior=prior, action=ScalarPhi4Action(kappa=0.67, m_sq=-4 * 0.67, lambd=0.5))
    (x, y, xh), (lj, l0) = nf.backward_sanitychecker(model, return_details=True)
    assert float((x - xh).abs().max()) < 1e-8 and float(l0.abs().max()) < 1e-8
    model.fit(n_epochs=40, batch_size=128, hyperparam=dict(lr=0.01), checkpoint_dict=dict(print_stride=1000))
    h = model.fit.train_history['loss']
    assert h[-1] < h[0] - 0.5


def test_graphed_flow_replays_bitwise():
    """GraphedFlow (one no_grad pass captured into a HIP graph) == the eager pass, bitwise, on new inputs,
    forward and backward; shape changes are refused.  (BASELINE config 2 shapes: launch-bound.)"""
    from normflow__amd import GraphedFlow
    torch.manual_seed(2)
    shape = (16, 16)
    mask = EvenOddMask(shape=shape)
    mk = lambda c: ConvAct(1, c, 3, conv_dim=2, hidden_sizes=[8, 8], acts=['tanh', 'tanh', None])
    net_ = ModuleList_([AffineCoupling_([mk(2) for _ in range(4)], mask=mask),
                        RQSplineCoupling_([mk(22), mk(22)], mask=mask, xlim=(-5, 5), ylim=(-5, 5),
                                          extrap={'left': 'linear', 'right': 'linear'})])
    net_.to(device=DEV, dtype=torch.float32)
    x = torch.randn((64,) + shape, device=DEV, dtype=torch.float32)
    fwd = GraphedFlow(net_, x)
    for _ in range(2):
        xn = torch.randn_like(x)
        with torch.no_grad():
            y0, l0 = net_(xn)
        y1, l1 = fwd(xn)
        assert torch.equal(y0, y1) and torch.equal(l0, l1)
    bwd = GraphedFlow(net_, y0, inverse=True, log0=l0)
    xb, lb = bwd(y0, l0)
    with torch.no_grad():
        xe, le = net_.backward(y0, l0)
    assert torch.equal(xb, xe) and torch.equal(lb, le)
    with pytest.raises(ValueError):
        fwd(x[:8])


@pytest.mark.parametrize("m,layout", [(16, "pair"), (16, "full"), (8, "pair"), (4, "full")])
def test_rqs_fp16_storage_fp32_logdet(m, layout):
    """BASELINE config 5 precision: x, logits and y stored in fp16, arithmetic fp32, log-det accumulated in
    fp32 (nf_dtype NF_F16).  Against the fp64 oracle ON THE SAME fp16-rounded inputs: y to fp16 output rounding
    (2^-11 relative), log|J| to the fp32 tolerance 1e-5; inverse by forward residual; byte-for-byte the same result as the
    fp32 kernel fed the fp16-rounded inputs, up to the final rounding of y."""
    torch.manual_seed(m)
    shape = (8, 8, 8, 16)
    B, V = 6, int(np.prod(shape))
    C = 3 * m - 2
    lim = dict(xlim=(-5.0, 5.0), ylim=(-5.0, 5.0), extrap={'left': 'linear', 'right': 'linear'})
    mask = EvenOddMask(shape=shape)
    act = mask.activity(0).reshape(-1).to(DEV)
    x16 = (1.5 * torch.randn(B, V, device=DEV)).half() * act.half()
    pfull = (0.5 * torch.randn(B, C, V, device=DEV)).half()
    p16 = compact(pfull, act) if layout == "pair" else pfull
    lay = _hip.LAYOUT_PAIR if layout == "pair" else _hip.LAYOUT_FULL
    opts = _hip.make_rqs_opts(m, lim["xlim"], lim["ylim"], lim["extrap"], lay)
    l0 = torch.randn(B, device=DEV, dtype=torch.float32)
    y16, lj = _hip.RQSCouplingFn.apply(x16, p16, l0, act, opts, False)
    assert y16.dtype == torch.float16 and lj.dtype == torch.float32
    yo, lo = O.rqs_coupling_atom(x16.double().cpu().reshape((B,) + shape), pfull.double().cpu().reshape((B, C) + shape),
                                 O.channel_mask(shape, 0), log0=l0.double().cpu(), **lim)
    assert rel(y16.reshape((B,) + shape), yo) <= 2 ** -10 and rel(lj, lo) <= 1e-5
    y32, lj32 = _hip.RQSCouplingFn.apply(x16.float(), p16.float(), l0, act, opts, False)
    assert torch.equal(y16, y32.half()) and torch.equal(lj, lj32)
    # inverse: y was rounded to fp16, so x comes back only up to 2^-11 / slope; the forward residual is the clean check
    xb, lb = _hip.RQSCouplingFn.apply(y16, p16, lj, act, opts, True)
    assert xb.dtype == torch.float16 and bool(torch.isfinite(lb).all())
    yb, _ = _hip.RQSCouplingFn.apply(xb, p16, None, act, opts, False)
    assert rel(yb, y16) <= 2 ** -9


def test_example_script_runs_with_package_defaults():
    """examples/phi4_lattice.py in a fresh interpreter: the package's import side effects (default dtype fp64,
    default device cuda -- the reference's, device/__init__.py:7-13) and a net assembled WITHOUT any explicit
    device: masks, priors and parameters must meet on the GPU (drop-in behaviour of user scripts)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k != "NORMFLOW_AMD_KEEP_TORCH_DEFAULTS"}
    for extra in (["--lat", "8,8", "--epochs", "4"], ["--lat", "4,4,8", "--kind", "rqs", "--layers", "2", "--epochs", "2", "--batch", "32"]):
        r = subprocess.run([sys.executable, os.path.join(root, "examples", "phi4_lattice.py")] + extra, env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert "Sanity check is OK" in r.stdout
        a, b = (float(t) for t in r.stdout.strip().splitlines()[-1].split())
        assert a < 1e-8 and b < 1e-8


@pytest.mark.parametrize("shape,B", [((4, 2, 6, 32), 100), ((2, 2, 2, 32), 7), ((8, 8, 8, 32), 3), ((2, 2, 4, 48), 9), ((4, 4, 4, 64), 5),
                                     ((4, 2, 2, 96), 3), ((8, 4, 4, 48), 4),
                                     # round 3 (tiled item order per XCD, half items): box counts that are not multiples of the tile,
                                     # rows of 2.5 and 3.5 segments, many boxes along axis 0, whole 4 x 4 tiles, more items than workgroups
                                     ((2, 6, 4, 48), 5), ((6, 2, 2, 80), 3), ((2, 2, 2, 112), 2), ((12, 2, 2, 32), 11), ((2, 8, 8, 48), 2),
                                     ((4, 8, 16, 48), 3)])
def test_split_fp16_fused_last_layer(shape, B):
    """nf_conv_h.hip: the fused last layer with every fp32 product as three fp16 matrix-core products (hidden
    activations are tanh outputs, so |h| <= 1).  Against (a) the fp32 kernels run separately (conv + coupling) and
    (b) the fp64 oracle, forward and inverse; several items per workgroup; asserts that this kernel ran.
    Tolerances: north_star's 1e-5 relative on y and log|J| vs the oracle; 5e-6 vs the fp32 path (the split
    products carry ~1.7x the rounding error of an fp32 chain)."""
    torch.manual_seed(17)
    m, C = 16, 46
    net = ConvAct(1, C, 3, conv_dim=4, hidden_sizes=[8, 8], acts=['tanh', 'tanh', None]).to(DEV, torch.float32)
    with torch.no_grad():
        for p_ in list(net.parameters())[-2:]:
            p_.mul_(0.3)
    mask = EvenOddMask(shape=shape)
    lim = dict(xlim=(-5.0, 5.0), ylim=(-5.0, 5.0), extrap={'left': 'linear', 'right': 'linear'})
    cpl = RQSplineCoupling_([net, net], mask=mask, **lim).to(DEV)
    x = 1.5 * torch.randn((B,) + shape, device=DEV, dtype=torch.float32)
    for parity in (0, 1):
        xa, xf = mask.purify(x, parity), mask.purify(x, 1 - parity)
        l0 = torch.randn(B, device=DEV, dtype=torch.float32)
        with torch.no_grad():
            yf, lf = cpl._fused_atom(False, xa, xf, parity, net, l0)
            assert _hip.load().nf_conv_last_path() == 3
            params, lay = cpl._params(net, xf, parity)
            opts = _hip.make_rqs_opts(m, lim["xlim"], lim["ylim"], lim["extrap"], lay)
            act = mask.activity(parity).reshape(-1).to(DEV)
            yu, lu = _hip.RQSCouplingFn.apply(xa.reshape(B, -1), params, l0, act, opts, False)
            assert rel(yf.reshape(B, -1), yu) <= 5e-6 and rel(lf, lu) <= 5e-6
            check_fused_round_trip(cpl, net, ['tanh', 'tanh', None], xa, xf, yf, lf, l0, parity, shape, lim)
            assert _hip.load().nf_conv_last_path() == 3
            perm = torch.randperm(B, device=DEV)
            yp, lp = cpl._fused_atom(False, xa[perm], xf[perm], parity, net, l0[perm])
            assert torch.equal(yp, yf[perm]) and torch.equal(lp, lf[perm])          # deterministic, sample-independent
        nb = min(B, 4)
        convs = [mod for mod in net if hasattr(mod, 'weight')]
        layers = [(c.weight.detach().double().cpu(), c.bias.detach().double().cpu()) for c in convs]
        out = O.conv_act(xf[:nb].double().cpu().unsqueeze(1), layers, ['tanh', 'tanh', None])
        yo, lo = O.rqs_coupling_atom(xa[:nb].double().cpu(), out, O.channel_mask(shape, parity),
                                     log0=l0[:nb].double().cpu(), **lim)
        assert rel(yf[:nb], yo) <= 1e-5 and rel(lf[:nb], lo) <= 1e-5


@pytest.mark.parametrize("shape,B", [((4, 2, 6, 32), 40), ((2, 4, 8, 32), 45), ((2, 2, 4, 32), 300), ((2, 2, 4, 48), 30), ((4, 4, 2, 64), 12),
                                     ((2, 4, 6, 48), 10),
                                     # round 3 (columns numbered tile by tile on multi-segment lattices): tile remainders, 2.5 segments
                                     ((6, 2, 2, 80), 4), ((2, 6, 4, 48), 6), ((8, 8, 2, 48), 3)])
def test_split_fp16_hidden_layer_and_chain(shape, B):
    """conv_g_kernel (8 -> 8 hidden layer on fp16 (hi, lo) pairs in and out) against the fp64 definition, and the whole
    split chain of a ConvAct stack (first layer writes the pairs, hidden layer, fused last layer) against the fp32
    kernels and the oracle."""
    torch.manual_seed(23)
    V = int(np.prod(shape))
    g = torch.Generator(device='cpu').manual_seed(5)
    h = torch.tanh(torch.randn((B, 8) + shape, generator=g, dtype=torch.float64, device='cpu'))
    w = 0.2 * torch.randn((8, 8, 3, 3, 3, 3), generator=g, dtype=torch.float64, device='cpu')
    b = 0.3 * torch.randn(8, generator=g, dtype=torch.float64, device='cpu')
    ref = torch.tanh(O.circular_conv_fast(h, w, b))
    h16 = _hip.to_split16(h.to(DEV, torch.float32))
    assert rel(_hip.from_split16(h16, shape), h) <= 1e-6            # the pair layout's own round trip
    out16 = _hip.conv_layer_split16(h16, w.to(DEV, torch.float32), b.to(DEV, torch.float32), _hip.ACT_CODES['tanh'], shape)
    out = _hip.from_split16(out16, shape)
    assert rel(out, ref) <= 1e-5        # (the fp32 kernels' bound for K = 648 terms is 1e-6 + 2e-7*0.3*648 = 4e-5)
    # the chain through the package API
    net = ConvAct(1, 46, 3, conv_dim=4, hidden_sizes=[8, 8], acts=['tanh', 'tanh', None]).to(DEV, torch.float32)
    with torch.no_grad():
        for p_ in list(net.parameters())[-2:]:
            p_.mul_(0.3)
    mask = EvenOddMask(shape=shape)
    lim = dict(xlim=(-5.0, 5.0), ylim=(-5.0, 5.0), extrap={'left': 'linear', 'right': 'linear'})
    cpl = RQSplineCoupling_([net, net], mask=mask, **lim).to(DEV)
    x = 1.5 * torch.randn((B,) + shape, device=DEV, dtype=torch.float32)
    xf = mask.purify(x, 1)
    with torch.no_grad():
        got = net.hidden_and_last(xf.unsqueeze(1))
    assert got[3] and got[0].dtype == torch.float16 and tuple(got[0].shape) == (B, V, 16)
    with torch.no_grad():
        y, lj = cpl(x)
        xb, lb = cpl.backward(y, lj)
    y2, lj2 = cpl(x[:3].clone().requires_grad_(True))          # fp32 kernels, logits materialised
    assert rel(y2, y[:3]) <= 5e-6 and rel(lj2, lj[:3]) <= 5e-6
    assert rel(xb, x) <= 5e-4 and float(lb.abs().max()) <= 5e-4 * max(1.0, float(lj.abs().max()))


def test_split_fp16_guards_and_graph_replay():
    """(a) weights outside the split kernel's range (|w| * 2^10 >= 3e4) fall back to the fp32 kernels, same results
    within tolerance; (b) the split chain is capturable: GraphedFlow replays it bitwise."""
    from normflow__amd import GraphedFlow
    torch.manual_seed(31)
    shape, B = (2, 2, 4, 32), 5
    net = ConvAct(1, 46, 3, conv_dim=4, hidden_sizes=[8, 8], acts=['tanh', 'tanh', None]).to(DEV, torch.float32)
    with torch.no_grad():
        for p_ in list(net.parameters())[-2:]:
            p_.mul_(0.3)
    mask = EvenOddMask(shape=shape)
    lim = dict(xlim=(-5.0, 5.0), ylim=(-5.0, 5.0), extrap={'left': 'linear', 'right': 'linear'})
    cpl = RQSplineCoupling_([net, net], mask=mask, **lim).to(DEV)
    x = torch.randn((B,) + shape, device=DEV, dtype=torch.float32)
    with torch.no_grad():
        y, lj = cpl(x)
    assert _hip.load().nf_conv_last_path() == 3
    g = GraphedFlow(cpl, x)
    xn = torch.randn_like(x)
    with torch.no_grad():
        y1, l1 = cpl(xn)
    y2, l2 = g(xn)
    assert torch.equal(y1, y2) and torch.equal(l1, l2)
    # one huge (but harmless: multiplied by a zero input channel weight elsewhere) weight switches the split path off
    last = [mod for mod in net if hasattr(mod, 'weight')][-1]
    with torch.no_grad():
        w_old = last.weight[0, 0, 0, 0, 0, 0].item()
        last.weight[0, 0, 0, 0, 0, 0] = 40.0
        y3, l3 = cpl(x)
        assert _hip.load().nf_conv_last_path() != 3
        y4, l4 = cpl(x[:2].clone().requires_grad_(True))
        assert rel(y4, y3[:2]) <= 5e-6 and rel(l4, l3[:2]) <= 5e-6
        last.weight[0, 0, 0, 0, 0, 0] = w_old
        y5, l5 = cpl(x)
    assert _hip.load().nf_conv_last_path() == 3 and torch.equal(y5, y) and torch.equal(l5, lj)


# -------------------------------------------------- the headline network itself (bench.build_net), end to end
def _oracle_nets(cpl, dtype):
    nets = []
    for net in cpl.nets:
        convs = [mod for mod in net if hasattr(mod, 'weight')]
        layers = [(c.weight.detach().to('cpu', dtype), c.bias.detach().to('cpu', dtype)) for c in convs]
        nets.append(lambda t, layers=layers: O.conv_act(t, layers, ['tanh', 'tanh', None]))
    return nets


def test_headline_network_vs_fp64_oracle():
    """bench.py's own network (bench.build_net: 8 RQ-spline layers m=16, ConvAct 1-8-8-46, logits rescaled to std 0.5) on a
    32-wide 4-D lattice the CPU oracle can afford, through the SAME kernels as the timed run (first layer -> fp16 pairs,
    split-fp16 hidden layer, split-fp16 fused last layer), against the fp64 oracle after all 8 layers: north_star's 1e-5
    on y and log|J|, or twice the error of the oracle run in float32 on the same network where 8 stacked fp32 layers are
    further than that from fp64 (the reference's own fp32 whole-net floor is 6e-5 on y)."""
    import bench
    lattice, B = (16, 16, 16, 32), 2
    net_, cpl = bench.build_net(lattice, 8, 16, DEV, seed=2024)
    g = torch.Generator(device=DEV).manual_seed(1234)
    x = torch.randn((B,) + lattice, device=DEV, dtype=torch.float32, generator=g)
    with torch.no_grad():
        y, lj = net_(x)
        assert _hip.load().nf_conv_last_path() == 3, "the split-fp16 kernels did not run"
        with _hip.options(split16=False):
            y32, lj32 = net_(x)
            assert _hip.load().nf_conv_last_path() != 3
    lim = dict(xlim=(-5.0, 5.0), ylim=(-5.0, 5.0), extrap={'left': 'linear', 'right': 'linear'})
    yo, lo = O.coupling_block(x.double().cpu(), _oracle_nets(cpl, torch.float64), 'rqs', lattice, **lim)
    yf, lf = O.coupling_block(x.float().cpu(), _oracle_nets(cpl, torch.float32), 'rqs', lattice, **lim)
    floor_y, floor_l = rel(yf, yo), rel(lf, lo)
    ty, tl = max(1e-5, 2 * floor_y), max(1e-5, 2 * floor_l)
    ey, el = rel(y, yo), rel(lj, lo)
    ey32, el32 = rel(y32, yo), rel(lj32, lo)
    print(f"\nheadline net vs fp64 oracle: split-fp16 path y {ey:.2e} logJ {el:.2e} | fp32-product path y {ey32:.2e} logJ {el32:.2e}"
          f" | CPU oracle in fp32: y {floor_y:.2e} logJ {floor_l:.2e}")
    assert ey <= ty and el <= tl, (ey, ty, el, tl)
    assert ey32 <= ty and el32 <= tl, (ey32, ty, el32, tl)


def test_headline_network_full_size_vs_fp64_oracle(parity_report):
    """The headline network at its own size: 32^4, all 8 RQ-spline layers of bench.build_net, one sample, through the timed
    kernels (split-fp16 products) and through exact fp32 MFMA products, EACH against the float64 oracle (~40 s of CPU),
    with the oracle run in float32 on the same network beside them as the floor: north_star's 1e-5 on y and log|J|, or
    twice that floor where eight stacked float32 layers are further than 1e-5 from float64 whatever the arithmetic."""
    import bench
    lattice, B = (32, 32, 32, 32), 1
    net_, cpl = bench.build_net(lattice, 8, 16, DEV, seed=2024)
    g = torch.Generator(device=DEV).manual_seed(1234)
    x = torch.randn((B,) + lattice, device=DEV, dtype=torch.float32, generator=g)
    with torch.no_grad():
        y, lj = net_(x)
        assert _hip.load().nf_conv_last_path() == 3, "the split-fp16 kernels did not run"
        with _hip.options(split16=False):
            y32, lj32 = net_(x)
            assert _hip.load().nf_conv_last_path() != 3
        assert _hip.load().nf_get_option(_hip.OPT_SPLIT16) == 1
    lim = dict(xlim=(-5.0, 5.0), ylim=(-5.0, 5.0), extrap={'left': 'linear', 'right': 'linear'})
    yo, lo = O.coupling_block(x.double().cpu(), _oracle_nets(cpl, torch.float64), 'rqs', lattice, **lim)
    yf, lf = O.coupling_block(x.float().cpu(), _oracle_nets(cpl, torch.float32), 'rqs', lattice, **lim)
    floor_y, floor_l = rel(yf, yo), rel(lf, lo)
    ty, tl = max(1e-5, 2 * floor_y), max(1e-5, 2 * floor_l)
    for name, (ya, la) in {"split-fp16 products": (y, lj), "fp32 products": (y32, lj32)}.items():
        ey, el = rel(ya, yo), rel(la, lo)
        parity_report("headline 32^4 x 8 layers", f"{name}: y", ey, ty, f"oracle-in-fp32 floor {floor_y:.2e}")
        parity_report("headline 32^4 x 8 layers", f"{name}: logJ", el, tl, f"oracle-in-fp32 floor {floor_l:.2e}")
        assert ey <= ty and el <= tl, (name, ey, ty, el, tl)
    # one layer of the same network at full size against the fp64 oracle: north_star's flat 1e-5
    xa, xf = cpl.mask.purify(x[:1], 0), cpl.mask.purify(x[:1], 1)
    with torch.no_grad():
        y1, l1 = cpl._fused_atom(False, xa, xf, 0, cpl.nets[0], 0)
    nets = _oracle_nets(cpl, torch.float64)
    out = nets[0](xf.double().cpu().unsqueeze(1))
    yo1, lo1 = O.rqs_coupling_atom(xa.double().cpu(), out, O.channel_mask(lattice, 0), log0=0, **lim)
    parity_report("headline 32^4, first layer", "split-fp16: y", rel(y1, yo1), 1e-5)
    parity_report("headline 32^4, first layer", "split-fp16: logJ", rel(l1, lo1), 1e-5)
    assert rel(y1, yo1) <= 1e-5 and rel(l1, lo1) <= 1e-5, (rel(y1, yo1), rel(l1, lo1))


def test_bench_self_launch_two_ranks_rehearsal():
    """`python bench.py --gpus 2 --full` with no launcher: the parent starts two ranks itself (before any GPU call of its own)
    and rank 0 prints ONE line with n_gpus 2, a weak and a strong leg.  NF_BENCH_REHEARSAL=1: both ranks share cuda:0 and meet
    over gloo -- the code path of the 8-GPU run (RCCL there), on the one-GPU box."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["NF_BENCH_REHEARSAL"] = "1"
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--batch", "8",
                        "--lattice", "4,4,4,32", "--layers", "2", "--kernel-reps", "3", "--full"],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["scaling"] == "weak" and line["config"]["global_batch"] == 16
    assert line["strong"]["global_batch"] == 8 and line["strong"]["batch_per_gpu"] == 4 and line["strong"]["value"] > 0
    assert line["value"] > 0 and line["value_fp32_products"] > 0 and line["selfcheck"]["split16_kernels_ran"]
    assert "cpu_baseline" not in line          # rank 0 at N = 1 only


def test_bench_dump_outputs_are_the_last_timed_step(tmp_path):
    """`python bench.py --steps 3 --dump-outputs DIR` on a small lattice: the line reports 3 timed steps and ms_per_step and,
    without --full, nothing else that takes work of its own; DIR/y.npy, DIR/logJ.npy (float32, in full at this size) are
    bench.build_net's network on bench's seeded input, recomputed here with bench's torch defaults (float32, CPU-initialised
    weights)."""
    import json
    import subprocess
    import sys
    import bench
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lattice, B, layers = (4, 4, 4, 32), 8, 2
    out = tmp_path / "dump"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--batch", str(B), "--lattice", ",".join(map(str, lattice)), "--layers", str(layers),
                        "--dump-outputs", str(out)],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    full_only = {"strong", "value_fp32_products", "fp32_products", "selfcheck", "roofline", "roofline_kernels",
                 "roofline_hbm_kernel", "other_configs", "cpu_baseline"}
    assert not full_only & set(line), sorted(full_only & set(line))
    yd, ld = np.load(out / "y.npy"), np.load(out / "logJ.npy")
    assert yd.dtype == np.float32 and yd.shape == (B,) + lattice and ld.dtype == np.float32 and ld.shape == (B,)
    dtype, device = torch.get_default_dtype(), torch.get_default_device()
    torch.set_default_dtype(torch.float32)
    torch.set_default_device("cpu")
    try:
        net_, _ = bench.build_net(lattice, layers, 16, DEV, seed=2024)
    finally:
        torch.set_default_dtype(dtype)
        torch.set_default_device(device)
    g = torch.Generator(device=DEV).manual_seed(1234)
    x = torch.randn((B,) + lattice, device=DEV, dtype=torch.float32, generator=g)
    with torch.no_grad():
        y, lj = net_(x)
    # the timed pass has no float atomics and static item schedules: the dump is these outputs bit for bit
    # (tests/test_kernel_state.py holds every kernel of the chain to that)
    assert np.array_equal(yd.view(np.int32), y.cpu().numpy().view(np.int32)), rel(torch.from_numpy(yd), y)
    assert np.array_equal(ld.view(np.int32), lj.cpu().numpy().view(np.int32)), rel(torch.from_numpy(ld), lj)


# -------------------------------------------------- the prior as one Philox kernel
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("B,shape,affine", [(3, (4, 4, 2, 6), False), (5, (7,), True), (2, (6, 5), True), (1, (1,), False),
                                            (4, (16, 16, 16), False)])
def test_philox_prior_kernel_vs_oracle(B, shape, affine, dtype):
    """nf_normal_sample through the C ABI against the oracle's restatement of the same counter layout, number by number
    (float32: the Box-Muller transcendentals are hardware log / sin / cos, 2e-5 absolute on O(1) draws; float64 1e-10),
    and logr against both the oracle and the density of the drawn field."""
    from normflow__amd.prior import NormalPrior
    V = int(np.prod(shape))
    if affine:
        g = torch.Generator(device='cpu').manual_seed(3)
        loc = torch.randn(shape, generator=g, device='cpu').to(DEV, dtype)
        scale = (0.5 + torch.rand(shape, generator=g, device='cpu')).to(DEV, dtype)
        prior = NormalPrior(loc=loc, scale=scale)
    else:
        loc = scale = None
        prior = NormalPrior(shape=shape)
        prior.to(device=DEV, dtype=dtype)
    torch.manual_seed(4242)
    gen = torch.cuda.default_generators[DEV.index]
    seed, off = gen.initial_seed(), gen.get_offset()
    x, logr = prior.sample_(B)
    assert gen.get_offset() == off + 4 and x.shape == (B,) + shape and logr.shape == (B,) and x.dtype == dtype
    xo, lo = O.normal_prior_sample(seed, off // 4, B, V, loc=None if loc is None else loc.cpu(),
                                   scale=None if scale is None else scale.cpu(), dtype=dtype)     # dtype selects the draw layout
    xo, lo = xo.double(), lo.double()
    tol = 2e-5 if dtype == torch.float32 else 1e-10
    assert float((x.double().cpu().reshape(B, V) - xo).abs().max()) <= tol * max(1.0, float(xo.abs().max()))
    assert rel(logr, lo) <= (1e-5 if dtype == torch.float32 else 1e-10)
    assert rel(logr, prior.log_prob(x)) <= (1e-5 if dtype == torch.float32 else 1e-10)      # logr IS the density of x
    torch.manual_seed(4242)
    x2, _ = prior.sample_(B)
    x3, _ = prior.sample_(B)
    assert torch.equal(x, x2) and not torch.equal(x2, x3)          # torch.manual_seed governs the kernel; the stream advances
    prior.torch_rng = True                                          # the reference's sampler stays available
    torch.manual_seed(7)
    xt, lt = prior.sample_(B)
    torch.manual_seed(7)
    want = torch.normal(prior.loc.expand((B,) + shape), prior.scale.expand((B,) + shape))
    assert torch.equal(xt, want) and rel(lt, prior.log_prob(xt)) <= 1e-6


def test_philox_prior_statistics():
    """10^6 draws per call: moments and a Kolmogorov-Smirnov test against the normal CDF; independence across samples
    and across calls (correlation of consecutive calls); a 32^4 batch fills every site."""
    from scipy import stats
    from normflow__amd.prior import NormalPrior
    prior = NormalPrior(shape=(1000,))
    prior.to(device=DEV, dtype=torch.float32)
    torch.manual_seed(99)
    x, logr = prior.sample_(1000)
    z = x.double().cpu().numpy().ravel()
    assert abs(z.mean()) < 4e-3 and abs(z.std() - 1) < 3e-3
    assert abs(stats.skew(z)) < 0.01 and abs(stats.kurtosis(z)) < 0.02
    assert stats.kstest(z, "norm").pvalue > 1e-3
    assert abs(np.corrcoef(z[:-1], z[1:])[0, 1]) < 4e-3                       # neighbours in a group / across groups
    x2, _ = prior.sample_(1000)
    assert abs(np.corrcoef(z, x2.double().cpu().numpy().ravel())[0, 1]) < 4e-3
    assert z.max() > 4.0 and z.min() < -4.0                                    # the tails are there
    big = NormalPrior(shape=(32, 32, 32, 32))
    big.to(device=DEV, dtype=torch.float32)
    xb, lb = big.sample_(3)
    assert bool(torch.isfinite(xb).all()) and float((xb == 0).float().mean()) < 1e-6
    assert rel(lb, big.log_prob(xb)) <= 1e-5
    assert abs(float(xb.mean())) < 2e-3 and abs(float(xb.std()) - 1) < 2e-3


# -------------------------------------------------- BASELINE config 5: fp16 parameters and fields, fp32 log-det
def test_config5_fp16_storage_mixed_network_48_wide():
    """Config 5's precision path end to end: a 16-layer mixed network (affine and RQ-spline blocks alternating, ConvAct
    1-8-8-C, m = 16) on a 48-wide 4-D lattice with fp16 PARAMETERS (net_.to(float16)) and an fp16 FIELD; log|J| accumulates in
    fp32.  Storage is half, arithmetic fp32: the affine atoms run conv -> nf_affine (NF_F16_FIELD: half field, the fp32
    parameters the conv layer wrote), the spline atoms the fused conv -> spline kernel with NF_CONV_FIELD_F16 (the logits never
    exist in memory).  Parity, layer by layer with the oracle's own (half-representable) inputs fed to every layer: the
    GPU's half output equals the oracle's fp64 result rounded to half up to one half-ulp (where fp32 arithmetic lands on the
    other side of a rounding boundary) plus the fp32 bound 1e-5 on the value itself (outputs near zero: half's spacing there is
    far finer than fp32 arithmetic on O(1) terms), on at most 2 % of the sites; the log-det increment matches to 1e-5 relative."""
    torch.manual_seed(55)
    shape, B, m = (4, 4, 4, 48), 3, 16
    mask = EvenOddMask(shape=shape)
    lim = dict(xlim=(-5.0, 5.0), ylim=(-5.0, 5.0), extrap={'left': 'linear', 'right': 'linear'})
    blocks = []
    for i in range(4):
        for kind in ('affine', 'rqs'):
            C = 2 if kind == 'affine' else 3 * m - 2
            nets = [ConvAct(1, C, 3, conv_dim=4, hidden_sizes=[8, 8], acts=['tanh', 'tanh', None]) for _ in range(2)]
            for net in nets:
                with torch.no_grad():
                    for p_ in list(net.parameters())[-2:]:
                        p_.mul_(0.3)
            blocks.append(AffineCoupling_(nets, mask=mask) if kind == 'affine' else RQSplineCoupling_(nets, mask=mask, **lim))
    net_ = ModuleList_(blocks)
    net_.to(device=DEV, dtype=torch.float16)
    assert all(p_.dtype == torch.float16 for p_ in net_.parameters())
    x = torch.randn((B,) + shape, device=DEV, dtype=torch.float32).half()
    with torch.no_grad():
        y, lj = net_(x)
        xb, lb = net_.backward(y, lj)
    assert y.dtype == torch.float16 and lj.dtype == torch.float32 and bool(torch.isfinite(y).all()) and bool(torch.isfinite(lj).all())
    assert rel(xb, x) <= 5e-2                 # 16 layers of half storage: each inverse restarts from a field rounded to 11 bits
    # layer by layer against the oracle, teacher-forced
    half = lambda t: t.to(torch.float16).to(torch.float64)
    parts = [half(x.double().cpu() * O.channel_mask(shape, c)) for c in (0, 1)]
    n_layers, worst_ulp, frac_off = 0, 0.0, 0.0
    for blk in blocks:
        kind = 'affine' if isinstance(blk, AffineCoupling_) else 'rqs'
        atom = O.affine_coupling_atom if kind == 'affine' else O.rqs_coupling_atom
        opts = {} if kind == 'affine' else lim
        for k, net in enumerate(blk.nets):
            p_ = k % 2
            convs = [mod for mod in net if hasattr(mod, 'weight')]
            layers = [(c.weight.detach().double().cpu(), c.bias.detach().double().cpu()) for c in convs]
            out = O.conv_act(parts[1 - p_].unsqueeze(1), layers, ['tanh', 'tanh', None])
            l0 = torch.randn(B, dtype=torch.float64, device='cpu')
            yo, lo = atom(parts[p_], out, O.channel_mask(shape, p_), log0=l0, **opts)
            with torch.no_grad():
                yg, lg = blk.atomic_forward(x_active=parts[p_].to(DEV, torch.float16), x_frozen=parts[1 - p_].to(DEV, torch.float16),
                                            parity=p_, net=net, log0=l0.to(DEV, torch.float32))
            assert yg.dtype == torch.float16 and lg.dtype == torch.float32
            want = half(yo)
            diff = (yg.double().cpu() - want).abs()
            # one half-ulp (the storage rounding may fall on the other side of a boundary) + north_star's fp32 bound on the value
            ulp = want.abs().clamp_min(2.0 ** -14) * 2.0 ** -10 + 1e-5 * max(1.0, float(want.abs().max()))
            worst_ulp = max(worst_ulp, float((diff / ulp).max()))
            frac_off = max(frac_off, float((diff > 0).double().mean()))
            assert rel(lg, lo) <= 1e-5, (kind, k, rel(lg, lo))
            parts[p_] = want
            n_layers += 1
    assert n_layers == 16
    assert worst_ulp <= 1.0 + 1e-9 and frac_off <= 0.02, (worst_ulp, frac_off)


@pytest.mark.parametrize("layout", ["pair", "full"])
def test_affine_fp16_storage_fp32_logdet(layout):
    """nf_affine with fp16 storage (NF_F16: x, params, y half; NF_F16_FIELD: params fp32): the fp32 kernel's result on the same
    rounded inputs up to the final rounding of y; log|J| fp32 within 1e-6 of the fp64 oracle on those inputs."""
    torch.manual_seed(8)
    shape, B = (8, 8, 8, 16), 5
    V = int(np.prod(shape))
    for parity in (0, 1):
        act = O.channel_mask(shape, parity).to(torch.uint8).reshape(-1).to(DEV)
        x16 = (1.5 * torch.randn(B, V, device=DEV)).half() * act.half()
        pfull = torch.randn(B, 2, V, device=DEV).half()
        par16 = compact(pfull, act) if layout == "pair" else pfull
        lay = _hip.LAYOUT_PAIR if layout == "pair" else _hip.LAYOUT_FULL
        l0 = torch.randn(B, device=DEV, dtype=torch.float32)
        for inverse in (False, True):
            y16, lj = _hip.AffineCouplingFn.apply(x16, par16, l0, act, lay, inverse)                 # NF_F16
            yf, ljf = _hip.AffineCouplingFn.apply(x16, par16.float(), l0, act, lay, inverse)         # NF_F16_FIELD
            y32, lj32 = _hip.AffineCouplingFn.apply(x16.float(), par16.float(), l0, act, lay, inverse)
            assert y16.dtype == torch.float16 and lj.dtype == torch.float32
            # the fp32 kernel's value rounded to half, up to one half-ulp (the instantiations may contract a*b+c differently)
            spacing = y32.abs().clamp_min(2.0 ** -14) * 2.0 ** -10
            for got in (y16, yf):
                d_ = (got.float() - y32).abs()
                assert bool((d_ <= spacing).all()) and float((got != y32.half()).float().mean()) < 0.01
            assert rel(lj, lj32) <= 1e-6 and rel(ljf, lj32) <= 1e-6
            yo, lo = O.affine_coupling_atom(x16.double().cpu().reshape((B,) + shape), pfull.double().cpu().reshape((B, 2) + shape),
                                            O.channel_mask(shape, parity), inverse=inverse, log0=l0.double().cpu())
            assert rel(lj, lo) <= 1e-6
            assert rel(y16, yo.reshape(B, V)) <= 1e-3


def test_graph_replay_survives_larger_eager_calls():
    """a captured graph bakes raw scratch pointers in.  The per-workgroup log-det partials come from torch's
    caching allocator per call (graph-pool safe), so a replay after LARGER eager calls and unrelated allocations still
    writes into memory the graph owns: results stay bitwise equal to an eager pass."""
    from normflow__amd import GraphedFlow
    torch.manual_seed(77)
    shape = (8, 8)
    mask = EvenOddMask(shape=shape)
    mk = lambda c: ConvAct(1, c, 3, conv_dim=2, hidden_sizes=[4], acts=['tanh', None]).to(DEV, torch.float32)
    lim = dict(xlim=(-4.0, 4.0), ylim=(-4.0, 4.0), extrap={'left': 'linear', 'right': 'linear'})
    net_ = ModuleList_([AffineCoupling_([mk(2), mk(2)], mask=mask), RQSplineCoupling_([mk(22), mk(22)], mask=mask, **lim)]).to(DEV)
    xs = torch.randn((4,) + shape, device=DEV, dtype=torch.float32)
    g = GraphedFlow(net_, xs)
    with torch.no_grad():
        y0, l0 = net_(xs)
        big = torch.randn((4096,) + shape, device=DEV, dtype=torch.float32)
        for _ in range(3):
            net_(big)                                        # needs far more scratch than the captured pass
        junk = [torch.full((1 << 20,), float(i), device=DEV, dtype=torch.float32) for i in range(16)]      # churn the allocator
        del junk
        net_(big[:1000])
    y1, l1 = g(xs)
    assert torch.equal(y1, y0) and torch.equal(l1, l0)
    # after an optimizer-like in-place weight change the graph re-captures (the kernel choice was validated for the old values)
    with torch.no_grad():
        for p_ in net_.parameters():
            p_.mul_(1.01)
        y2, l2 = net_(xs)
    y3, l3 = g(xs)
    assert torch.equal(y3, y2) and torch.equal(l3, l2) and not torch.equal(y3, y0)


@pytest.mark.parametrize("shape,B", [((4, 2, 6, 32), 33), ((2, 2, 2, 32), 5), ((2, 4, 4, 48), 9), ((4, 4, 2, 64), 6)])
def test_fused_affine_layer_on_the_split_chain(shape, B):
    """nf_conv_affine_split16: the last layer (8 -> 2) of an affine coupling's net fused with the coupling, fed by the pair
    tensor of the split-fp16 chain -- against the unfused path (fp32 conv stack + nf_affine: two roundings of the same exact
    result) and against the fp64 oracle within north_star's 1e-5; forward, inverse (round trip through the fused kernels),
    both parities, log0 threaded; batch-permutation invariance (the per-(column, wave) log-det partials are deterministic)."""
    torch.manual_seed(41)
    net = ConvAct(1, 2, 3, conv_dim=4, hidden_sizes=[8, 8], acts=['tanh', 'tanh', None]).to(DEV, torch.float32)
    with torch.no_grad():
        for p_ in list(net.parameters())[-2:]:
            p_.mul_(0.3)
    mask = EvenOddMask(shape=shape)
    cpl = AffineCoupling_([net, net], mask=mask).to(DEV)
    x = 1.5 * torch.randn((B,) + shape, device=DEV, dtype=torch.float32)
    convs = [mod for mod in net if hasattr(mod, 'weight')]
    layers = [(c.weight.detach().double().cpu(), c.bias.detach().double().cpu()) for c in convs]
    for parity in (0, 1):
        xa, xf = mask.purify(x, parity), mask.purify(x, 1 - parity)
        l0 = torch.randn(B, device=DEV, dtype=torch.float32)
        with torch.no_grad():
            got = cpl._fused_atom(False, xa, xf, parity, net, l0)
            assert got is not None, "the fused affine path did not apply"
            yf, lf = got
            with _hip.options(split16=False):
                assert cpl._fused_atom(False, xa, xf, parity, net, l0) is None
                yu, lu = cpl.atomic_forward(x_active=xa, x_frozen=xf, parity=parity, net=net, log0=l0)
            assert rel(yf, yu) <= 1e-5 and rel(lf, lu) <= 1e-5, (rel(yf, yu), rel(lf, lu))
            xb, lb = cpl._fused_atom(True, yf, xf, parity, net, lf)
            assert rel(xb, xa) <= 2e-5 and rel(lb, l0) <= 1e-5 * max(1.0, float(lf.abs().max())), (rel(xb, xa), rel(lb, l0))
            perm = torch.randperm(B, device=DEV)
            yp, lp = cpl._fused_atom(False, xa[perm], xf[perm], parity, net, l0[perm])
            assert torch.equal(yp, yf[perm]) and torch.equal(lp, lf[perm])
        nb = min(B, 4)
        out = O.conv_act(xf[:nb].double().cpu().unsqueeze(1), layers, ['tanh', 'tanh', None])
        yo, lo = O.affine_coupling_atom(xa[:nb].double().cpu(), out, O.channel_mask(shape, parity), log0=l0[:nb].double().cpu())
        assert rel(yf[:nb], yo) <= 1e-5 and rel(lf[:nb], lo) <= 1e-5, (rel(yf[:nb], yo), rel(lf[:nb], lo))
    # the block-level API takes the fused path under no_grad and the differentiable path otherwise
    with torch.no_grad():
        y1, l1 = cpl(x)
    y2, l2 = cpl(x.clone().requires_grad_(True))
    assert rel(y1, y2) <= 1e-5 and rel(l1, l2) <= 1e-5


# ----------------------------------------------------------------------------- the spline object of a coupling layer
SPLINE_EXTRAPS = [{}, {'left': 'linear', 'right': 'linear'}, {'left': 'anti'}, {'left': 'anti', 'right': 'linear'},
                  {'right': 'anti'}]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("m", [2, 5, 16])
def test_make_spline_knots_and_values_vs_oracle(m, dtype):
    """`RQSplineCoupling_.make_spline(out)` (couplings_.py:211-262): the knot tensors the object shows (nf_rqs_knots + the
    boundary augmentation of spline.py:458-532) and spline(x, grad=True) / spline.backward(y, grad=True) at EVERY site
    (nf_rqs_fwd_sites / nf_rqs_inv_sites) against the oracle's knots_from_logits / augment_knots / rqs_evaluate /
    rqs_invert.  fp64 1e-9; fp32 1e-5 on knots and values, derivative 1e-4 (it is exp of a log the kernel holds to 1e-5)."""
    shape, B = (4, 6, 5), 3
    x, out = _rand_case(shape, B, m, 400 + m, dtype, x_std=1.5)
    lim = dict(xlim=(-2.0, 2.0), ylim=(-1.5, 2.5))
    tol = 1e-9 if dtype == torch.float64 else 1e-5
    mask = EvenOddMask(shape=shape)
    for extrap in SPLINE_EXTRAPS:
        cpl = RQSplineCoupling_([torch.nn.Identity()], mask=mask, extrap=extrap, **lim)
        sp = cpl.make_spline(out.to(DEV, dtype))
        kx, ky, kd = O.knots_from_logits(out, **lim)
        kx, ky, kd = O.augment_knots(kx, ky, kd, axis=1, **extrap)
        assert sp.knots_len == kx.shape[1] and tuple(sp.knots_shape) == tuple(kx.shape)
        assert rel(sp.knots_x, kx) <= tol and rel(sp.knots_y, ky) <= tol and rel(sp.knots_d, kd) <= tol
        # inside the knot range, and for the extrapolating variants also beyond it
        v = (2.0 * x).unsqueeze(1)
        v = v.clamp(min=-1e9 if extrap.get('left') else -1.99, max=1e9 if extrap.get('right') else 1.99)
        if 'anti' in extrap.values() and len(extrap) == 1:      # the mirror image must stay inside the side with no rule
            v = v.clamp(-5.9, 5.9)
        fo, go = O.rqs_evaluate(kx, ky, kd, v, axis=1)
        f, g = sp(v.to(DEV, dtype), grad=True)
        assert f.shape == v.shape and g.shape == v.shape
        assert rel(f, fo) <= tol and rel(g, go) <= 10 * tol
        assert rel(sp(v.squeeze(1).to(DEV, dtype), squeezed=True), fo.squeeze(1)) <= tol
        w = fo.clamp(min=-1e9 if extrap.get('left') else -1.49, max=1e9 if extrap.get('right') else 2.49)
        bo, hgo = O.rqs_invert(kx, ky, kd, w, axis=1)
        bk, hg = sp.backward(w.to(DEV, dtype), grad=True)
        assert rel(bk, bo) <= 50 * tol and rel(hg, hgo) <= 50 * tol


def test_make_spline_fixed_knots_and_channels_axis():
    """Fixed 1-D knots_x / knots_y are copied through to every site; a channels axis other than 1 is honoured."""
    shape, B, m = (6, 4), 2, 5
    kxf = torch.tensor([-2.0, -0.7, 0.1, 0.9, 2.0], dtype=torch.float64, device='cpu')
    torch.manual_seed(11)
    out = 0.5 * torch.randn((B, 2 * m - 1) + shape, dtype=torch.float64, device='cpu')
    x = torch.randn((B, 1) + shape, dtype=torch.float64, device='cpu').clamp(-1.9, 1.9)
    mask = EvenOddMask(shape=shape)
    cpl = RQSplineCoupling_([torch.nn.Identity()], mask=mask, xlim=(-2.0, 2.0), ylim=(-2.0, 2.0), knots_x=kxf)
    sp = cpl.make_spline(out.to(DEV))
    kx, ky, kd = O.knots_from_logits(out, (-2.0, 2.0), (-2.0, 2.0), knots_x=kxf)
    assert rel(sp.knots_x, O._bcast_like(kx, out).expand_as(ky)) == 0.0
    assert rel(sp.knots_y, ky) <= 1e-12 and rel(sp.knots_d, kd) <= 1e-12
    fo, go = O.rqs_evaluate(O._bcast_like(kx, out).expand_as(ky), ky, kd, x, axis=1)
    f, g = sp(x.to(DEV), grad=True)
    assert rel(f, fo) <= 1e-10 and rel(g, go) <= 1e-9
    # channels last
    cpl2 = RQSplineCoupling_([torch.nn.Identity()], mask=mask, xlim=(-2.0, 2.0), ylim=(-2.0, 2.0), knots_x=kxf,
                             channels_axis=-1)
    sp2 = cpl2.make_spline(out.movedim(1, -1).contiguous().to(DEV))
    assert tuple(sp2.knots_y.shape) == (B,) + shape + (m,)
    assert rel(sp2.knots_y.movedim(-1, 1), ky) <= 1e-12


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_hack_and_propagate_density(dtype):
    """`_hack` (couplings_.py:202-209) and propagate_density (nn/_core.py:19,38-42): per-site log-derivatives, zero off the
    active sublattice, against the oracle's per-site log g; their sum over the sites is the layer's log|J| (same kernel
    arithmetic, summed in the other order: 1e-12 / 1e-6 relative)."""
    torch.manual_seed(5)
    shape, B, m = (4, 6, 8), 3, 8
    net = ConvAct(1, 3 * m - 2, 3, conv_dim=3, hidden_sizes=[4], acts=['tanh', None]).to(DEV, dtype)
    mask = EvenOddMask(shape=shape)
    opts = dict(xlim=(-3.0, 3.0), ylim=(-3.0, 3.0), extrap={'left': 'linear', 'right': 'linear'})
    cpl = RQSplineCoupling_([net, net], mask=mask, **opts).to(DEV)
    x = 1.5 * torch.randn((B,) + shape, device=DEV, dtype=dtype)
    convs = [mod for mod in net if hasattr(mod, 'weight')]
    layers = [(c.weight.double().cpu(), c.bias.double().cpu()) for c in convs]
    tol = 1e-9 if dtype == torch.float64 else 1e-5
    for parity in (0, 1):
        am = O.channel_mask(shape, parity)
        xa, xf = x * am.to(DEV, dtype), x * (1 - am).to(DEV, dtype)
        spline, fx, logg = cpl._hack(x_active=xa, x_frozen=xf, parity=parity, net=net)
        out = O.conv_act(xf.double().cpu().unsqueeze(1), layers, ['tanh', None])
        kx, ky, kd = O.knots_from_logits(out, opts['xlim'], opts['ylim'])
        kx, ky, kd = O.augment_knots(kx, ky, kd, axis=1, **opts['extrap'])
        fo, go = O.rqs_evaluate(kx, ky, kd, xa.double().cpu().unsqueeze(1), axis=1)
        assert rel(fx, fo.squeeze(1) * am) <= tol
        assert rel(logg, torch.log(go.squeeze(1)) * am) <= tol
        assert float(logg[:, am == 0].abs().max()) == 0.0 and float(fx[:, am == 0].abs().max()) == 0.0
        assert rel(spline.knots_d, kd) <= tol
        with torch.no_grad():
            y, lj = cpl.atomic_forward(x_active=xa, x_frozen=xf, parity=parity, net=net, log0=0)
        assert rel(fx, y) <= (1e-12 if dtype == torch.float64 else 1e-6)
        assert rel(logg.reshape(B, -1).double().sum(1), lj) <= (1e-12 if dtype == torch.float64 else 2e-6)
    # propagate_density: whole block, forward and inverse, log0 a per-site tensor
    with torch.no_grad():
        y_ref, lj_ref = cpl(x)
        cpl.propagate_density = True
        try:
            y, dens = cpl(x)
            assert dens.shape == x.shape
            assert torch.equal(y, y_ref)
            assert rel(dens.reshape(B, -1).double().sum(1), lj_ref) <= (1e-12 if dtype == torch.float64 else 2e-6)
            xb, back = cpl.backward(y, dens)
            assert rel(xb, x) <= 100 * tol and float(back.abs().max()) <= 100 * tol
        finally:
            cpl.propagate_density = False
    with pytest.raises(NotImplementedError):
        cpl.propagate_density = True
        try:
            cpl(x.clone().requires_grad_(True))
        finally:
            cpl.propagate_density = False


@pytest.mark.parametrize("lattice,cin,cout,B", [((2, 3, 4, 32), 8, 46, 3), ((2, 2, 2, 32), 1, 8, 5), ((4, 2, 2, 32), 8, 8, 2),
                                                ((1, 1, 3, 32), 8, 22, 4), ((3, 2, 1, 32), 1, 8, 2), ((2, 2, 3, 48), 8, 46, 2),
                                                ((2, 1, 2, 64), 8, 8, 3), ((1, 2, 2, 48), 1, 8, 2), ((2, 2, 1, 96), 8, 14, 1)])
def test_conv_wgrad_split16_kernel_vs_autograd(lattice, cin, cout, B):
    """nf_conv_wgrad_split16 (nf_conv_w.hip): grad_weight and grad_bias of a 3^4 circular conv layer on the fp16 matrix cores
    (three fp16 products per fp32 product, gz scaled into fp16's range) against autograd through the fp64 oracle
    convolution, with cotangents of the magnitude a mean over a batch produces (1e-6) as well as O(1); equal to the fp32
    kernel (nf_conv_wgrad) within the same bound; deterministic.  2e-5 relative to the largest entry, the fp32 kernel's
    bound in test_conv_vjp_kernels_vs_autograd."""
    g = torch.Generator(device='cpu').manual_seed(cin * 100 + cout)
    x = torch.randn((B, cin) + lattice, generator=g, dtype=torch.float64, device='cpu')
    w = 0.3 * torch.randn((cout, cin) + (3,) * 4, generator=g, dtype=torch.float64, device='cpu')
    bias = torch.randn(cout, generator=g, dtype=torch.float64, device='cpu')
    for gscale in (1.0, 1e-6):
        go = gscale * torch.randn((B, cout) + lattice, generator=g, dtype=torch.float64, device='cpu')
        go[:, :, 0, 0, 0, :4] *= 50.0                    # a few large entries: the scale follows the maximum
        wo, bo = w.clone().requires_grad_(True), bias.clone().requires_grad_(True)
        ref = O.circular_conv_direct(x, wo, bo)
        gw_ref, gb_ref = torch.autograd.grad(ref, (wo, bo), go)
        xd, god = x.to(DEV, torch.float32), go.to(DEV, torch.float32)
        assert _hip.load().nf_conv_wgrad_split16_supported(*_hip._lat4(lattice, (3,) * 4), cin, cout)
        gw, gb = _hip.conv_weight_grad(xd, god, (3,) * 4)
        gw2, gb2 = _hip.conv_weight_grad(xd, god, (3,) * 4)
        assert torch.equal(gw, gw2) and torch.equal(gb, gb2)
        with _hip.options(split16=False):
            gw32, gb32 = _hip.conv_weight_grad(xd, god, (3,) * 4)
        for got, want in ((gw, gw_ref), (gb, gb_ref), (gw32, gw_ref), (gb32, gb_ref)):
            assert float((got.double().cpu() - want).abs().max()) <= 2e-5 * float(want.abs().max())


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("kind", ["affine", "shift"])
def test_affine_propagate_density(kind, dtype):
    """propagate_density (nn/_core.py:19,38-42) on the affine / shift couplings: nf_affine_sites returns -|s| (forward) / +|s|
    (inverse) per active site, 0 elsewhere and for a shift layer; against the oracle's (t, s) of the same net, and summing
    to the layer's log|J|; the values of the map are those of the summed path, bit for bit."""
    torch.manual_seed(3)
    shape, B = (6, 4, 8), 3
    nch = 2 if kind == "affine" else 1
    net = ConvAct(1, nch, 3, conv_dim=3, hidden_sizes=[4], acts=['tanh', None]).to(DEV, dtype)
    mask = EvenOddMask(shape=shape)
    cls = AffineCoupling_ if kind == "affine" else ShiftCoupling_
    cpl = cls([net, net], mask=mask).to(DEV)
    x = torch.randn((B,) + shape, device=DEV, dtype=dtype)
    convs = [mod for mod in net if hasattr(mod, 'weight')]
    layers = [(c.weight.double().cpu(), c.bias.double().cpu()) for c in convs]
    tol = 1e-10 if dtype == torch.float64 else 1e-5
    with torch.no_grad():
        y_ref, lj_ref = cpl(x)
        cpl.propagate_density = True
        try:
            y, dens = cpl(x)
            if kind == "shift":
                # unit Jacobian: the reference hands log0 back untouched (couplings_.py:110-116), number or tensor
                assert dens == 0 and not torch.is_tensor(dens) and torch.equal(y, y_ref)
                l0 = torch.randn_like(x)
                y2, d2 = cpl(x, l0)
                assert d2 is l0 and torch.equal(y2, y_ref)
                xb, back = cpl.backward(y, l0)
                assert back is l0 and rel(xb, x) <= 100 * tol
                return
            assert dens.shape == x.shape and torch.equal(y, y_ref)
            lj_sum = dens.reshape(B, -1).double().sum(1)
            if torch.is_tensor(lj_ref):
                assert rel(lj_sum, lj_ref) <= (1e-12 if dtype == torch.float64 else 2e-6)
            else:
                assert float(lj_sum.abs().max()) == 0.0
            # first layer against the oracle: density = -|s| at the active sites of parity 0
            am = O.channel_mask(shape, 0)
            xa, xf = x * am.to(DEV, dtype), x * (1 - am).to(DEV, dtype)
            _, d0 = cpl.atomic_forward(x_active=xa, x_frozen=xf, parity=0, net=net, log0=0)
            out = O.conv_act(xf.double().cpu().unsqueeze(1), layers, ['tanh', None])
            want = -out[:, 1].abs() * am if kind == "affine" else torch.zeros_like(out[:, 0])
            assert rel(d0, want) <= tol
            xb, back = cpl.backward(y, dens)
            assert rel(xb, x) <= 100 * tol and float(back.abs().max()) <= 100 * tol
        finally:
            cpl.propagate_density = False


@pytest.mark.parametrize("lattice,cout,B,cin", [((2, 2, 4, 32), 46, 3, 8), ((4, 2, 2, 32), 8, 2, 8), ((2, 4, 2, 48), 22, 2, 8),
                                                    ((2, 2, 2, 64), 46, 1, 8), ((2, 2, 4, 32), 8, 3, 1)])
def test_conv_input_grad_split16_vs_autograd(lattice, cout, B, cin):
    """nf_planes_to_split16 + nf_conv_dgrad_split16: the gradient w.r.t. the input of an 8 -> cout layer on the split-fp16
    chain (cotangent scaled into fp16's range, 8-channel groups through the hidden-layer kernel, fp32 planes accumulated)
    against autograd through the fp64 oracle convolution, with O(1) and 1e-6 cotangents; the whole ConvFn.backward with it
    (weight and bias gradients from nf_conv_wgrad_split16 where the lattice qualifies).  2e-5 of the largest entry."""
    g = torch.Generator(device='cpu').manual_seed(cout)
    x = torch.tanh(torch.randn((B, cin) + lattice, generator=g, dtype=torch.float64, device='cpu'))
    w = 0.3 * torch.randn((cout, cin) + (3,) * 4, generator=g, dtype=torch.float64, device='cpu')
    bias = torch.randn(cout, generator=g, dtype=torch.float64, device='cpu')
    for gscale in (1.0, 1e-6):
        go = gscale * torch.randn((B, cout) + lattice, generator=g, dtype=torch.float64, device='cpu')
        go[:, :, 0, 0, 0, :4] *= 30.0
        xo, wo, bo = (t.clone().requires_grad_(True) for t in (x, w, bias))
        ref = O.circular_conv_direct(xo, wo, bo)
        gref = torch.autograd.grad(ref, (xo, wo, bo), go)
        xd, wd, bd = (t.to(DEV, torch.float32).requires_grad_(True) for t in (x, w, bias))
        out = _hip.conv_layer(xd, wd, bd, 0)
        got = torch.autograd.grad(out, (xd, wd, bd), go.to(DEV, torch.float32))
        for a_, r_ in zip(got, gref):
            assert float((a_.double().cpu() - r_).abs().max()) <= 2e-5 * float(r_.abs().max())
        wt = wd.detach().flip([2, 3, 4, 5]).transpose(0, 1).contiguous()
        direct = _hip.conv_input_grad_split16(go.to(DEV, torch.float32), wt)
        assert direct is not None and torch.equal(direct, got[0])           # this path ran, and it is deterministic
    if cout == 8 and cin == 8:
        # the forward 8 -> 8 layer training keeps as planes (ConvFn.forward): tanh and no activation, inputs beyond [-1, 1] too
        for act, scale in (('tanh', 1.0), (None, 40.0)):
            xs = (scale * x).to(DEV, torch.float32)
            want = O._ACTS[act](O.circular_conv_direct(scale * x, w, bias))
            got_f = _hip.conv_hidden_planes_split16(xs, w.to(DEV, torch.float32), bias.to(DEV, torch.float32), _hip.ACT_CODES[act])
            assert got_f is not None
            assert float((got_f.double().cpu() - want).abs().max()) <= 1e-5 * max(1.0, float(want.abs().max()))
            tr = _hip.conv_layer(xs.clone().requires_grad_(True), w.to(DEV, torch.float32), bias.to(DEV, torch.float32),
                                 _hip.ACT_CODES[act])
            assert torch.equal(tr.detach(), got_f)


@pytest.mark.parametrize("lattice,B", [((2, 2, 4, 32), 3), ((4, 2, 2, 32), 5), ((2, 2, 2, 48), 2), ((2, 4, 2, 64), 1)])
def test_conv_last_logits_split16_vs_oracle(lattice, B):
    """nf_conv_last_logits_split16 (K5h's matrix-core part with the logits written out): the 8 -> 46 layer at the active
    sites, pair-compact, against the fp64 oracle convolution; inputs in [-1, 1] and far outside (the input is scaled by the
    power of two of its maximum); and through ConvFn (training), where it is the forward of the compact last layer and the
    gradients still match autograd through the oracle.  1e-5 of the largest logit."""
    g = torch.Generator(device='cpu').manual_seed(46)
    w = 0.1 * torch.randn((46, 8) + (3,) * 4, generator=g, dtype=torch.float64, device='cpu')
    bias = torch.randn(46, generator=g, dtype=torch.float64, device='cpu')
    for scale in (1.0, 300.0):
        x = scale * torch.tanh(torch.randn((B, 8) + lattice, generator=g, dtype=torch.float64, device='cpu'))
        full = O.circular_conv_direct(x, w, bias)
        for parity in (0, 1):
            act_mask = (O.even_odd_mask(lattice, parity=parity) == 1).reshape(-1)
            want = compact(full.reshape(B, 46, -1), act_mask.to(torch.uint8))
            got = _hip.conv_last_logits_split16(x.to(DEV, torch.float32), w.to(DEV, torch.float32), bias.to(DEV, torch.float32), parity)
            assert got is not None and got.shape == want.shape
            assert float((got.double().cpu() - want).abs().max()) <= 1e-5 * float(want.abs().max())
    # through autograd: forward equals the direct call bit for bit, gradients vs the oracle
    x = torch.tanh(torch.randn((B, 8) + lattice, generator=g, dtype=torch.float64, device='cpu'))
    act_mask = (O.even_odd_mask(lattice, parity=0) == 1).reshape(-1)
    xd, wd, bd = (t.to(DEV, torch.float32).requires_grad_(True) for t in (x, w, bias))
    out = _hip.conv_layer(xd, wd, bd, 0, compact=True, parity=0)
    assert torch.equal(out.detach(), _hip.conv_last_logits_split16(xd.detach(), wd.detach(), bd.detach(), 0))
    go = torch.randn((B, 46) + lattice, generator=g, dtype=torch.float64, device='cpu') * act_mask.reshape((1, 1) + lattice).double()
    goc = compact(go.reshape(B, 46, -1).to(DEV, torch.float32), act_mask.to(torch.uint8).to(DEV))
    got = torch.autograd.grad(out, (xd, wd, bd), goc)
    xo, wo, bo = (t.clone().requires_grad_(True) for t in (x, w, bias))
    gref = torch.autograd.grad(O.circular_conv_direct(xo, wo, bo), (xo, wo, bo), go)
    for a_, r_ in zip(got, gref):
        assert float((a_.double().cpu() - r_).abs().max()) <= 2e-5 * float(r_.abs().max())


# ------------------------------------------------------------------ round 3: small completions
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("layout", ["nd_axis1", "nd_last", "shared", "mixed_x1d"])
def test_rqspline_from_explicit_knots_vs_oracle(layout, dtype):
    """`RQSpline(knots_x=, knots_y=, knots_d=, knots_axis=, extrap=)` (spline.py:39-68) on nf_spline_eval: per-site knots
    along axis 1 or the last axis, one shared 1-D spline, and 1-D knots_x against N-D knots_y; forward / backward with
    grad=True against the oracle's augment_knots + rqs_evaluate / rqs_invert.  fp64 1e-10, fp32 1e-5 (values),
    1e-4 (derivatives)."""
    from normflow__amd.lib.spline import RQSpline
    torch.manual_seed(77)
    B, L, m = 3, (5, 4), 6
    tol = 1e-10 if dtype == torch.float64 else 1e-5
    with torch.device("cpu"):
        out = 0.6 * torch.randn((B, 3 * m - 2) + L, dtype=torch.float64)
        kx, ky, kd = O.knots_from_logits(out, (-2.0, 2.0), (-1.0, 3.0))
        if layout == "shared":
            kx, ky, kd = kx[0, :, 0, 0].contiguous(), ky[0, :, 0, 0].contiguous(), kd[0, :, 0, 0].contiguous()
        if layout == "mixed_x1d":
            kx = torch.linspace(-2.0, 2.0, m, dtype=torch.float64)
        v = 1.6 * torch.randn((B, 2) + L, dtype=torch.float64)      # two points per spline along the knots axis
    for extrap in ({}, {'left': 'linear', 'right': 'linear'}, {'left': 'anti-periodic', 'right': 'linear'}):
        if not extrap:
            vv = v.clamp(-1.95, 1.95)
        else:
            vv = v
        ax = 0 if layout == "shared" else 1
        if layout == "mixed_x1d" and extrap:
            kxo = O._bcast_like(kx, ky).expand_as(ky)
        else:
            kxo = kx
        with torch.device("cpu"):
            akx, aky, akd = O.augment_knots(kxo, ky, kd, axis=ax, **extrap)
            if layout == "shared":
                fo, go = O.rqs_evaluate(akx.reshape(-1, 1), aky.reshape(-1, 1), akd.reshape(-1, 1), vv.reshape(1, -1), axis=0)
                fo, go = fo.reshape(vv.shape), go.reshape(vv.shape)
            else:               # the oracle evaluates one point per spline: the two points of the knots axis one by one
                pts = [O.rqs_evaluate(O._bcast_like(akx, aky), aky, akd, vv[:, r:r + 1], axis=1) for r in range(vv.shape[1])]
                fo, go = torch.cat([p[0] for p in pts], 1), torch.cat([p[1] for p in pts], 1)
        to = lambda t: t.to(DEV, dtype)
        if layout == "nd_last":
            sp = RQSpline(knots_x=to(kx.movedim(1, -1)), knots_y=to(ky.movedim(1, -1)), knots_d=to(kd.movedim(1, -1)),
                          knots_axis=-1, extrap=extrap)
            inp, back = to(vv.movedim(1, -1).contiguous()), (lambda t: t.movedim(-1, 1))
        else:
            sp = RQSpline(knots_x=to(kx), knots_y=to(ky), knots_d=to(kd), knots_axis=(0 if layout == "shared" else 1),
                          extrap=extrap)
            inp, back = to(vv), (lambda t: t)
        assert sp.knots_len == akx.shape[ax]
        f, g = sp(inp, grad=True)
        assert rel(back(f), fo) <= tol and rel(back(g), go) <= 10 * tol, (layout, extrap, rel(back(f), fo), rel(back(g), go))
        assert rel(back(sp.forward(inp)), fo) <= tol
        xb, ig = sp.backward(f, grad=True)
        assert rel(back(xb), vv) <= 100 * tol and rel(back(ig), 1 / go) <= 100 * tol, (layout, extrap, rel(back(xb), vv))
    # knots_d = None: the reference's smooth derivatives (spline.py:125-152)
    if layout in ("nd_axis1", "shared"):
        ax = 0 if layout == "shared" else 1
        sp = RQSpline(knots_x=kx.to(DEV, dtype), knots_y=ky.to(DEV, dtype), knots_d=None, knots_axis=ax)
        with torch.device("cpu"):
            slope = (ky.narrow(ax, 1, m - 1) - ky.narrow(ax, 0, m - 1)) / (kx.narrow(ax, 1, m - 1) - kx.narrow(ax, 0, m - 1))
            want = torch.cat((slope.narrow(ax, 0, 1), 0.5 * (slope.narrow(ax, 1, m - 2) + slope.narrow(ax, 0, m - 2)),
                              slope.narrow(ax, m - 2, 1)), ax)
        assert rel(sp.knots_d, want) <= tol


_SEG_CASES = {}


def _shared_segment_case(K):
    """K shared knots on (0, 1) and (3, 257) points for each direction: drawn inside the knot range, with every interior
    knot itself in front of each row (a value ON knot k belongs to bin k - 1: "strictly below").  Everything is rounded
    through float32, so both precisions see the same numbers.  The fp64 oracle gives the expected values once per K, and is
    used alone to check that no denominator of the segment or of its inverse root comes near zero at these points."""
    if K in _SEG_CASES:
        return _SEG_CASES[K]
    g = torch.Generator(device='cpu').manual_seed(500 + K)
    r32 = lambda t: t.float().double()
    with torch.device("cpu"):
        cum = lambda: torch.cat((torch.zeros(1, dtype=torch.float64),
                                 torch.cumsum(0.5 + torch.rand(K - 1, generator=g, dtype=torch.float64), 0)))
        cx, cy = cum(), cum()
        kx, ky = r32(0.05 + 0.9 * cx / cx[-1]), r32(0.08 + 0.85 * cy / cy[-1])
        kd = r32(0.5 + 1.5 * torch.rand(K, generator=g, dtype=torch.float64))
        pts = {}
        for name, kn in (("x", kx), ("y", ky)):
            u = torch.rand((3, 257), generator=g, dtype=torch.float64)
            p = r32(kn[0] + (kn[-1] - kn[0]) * (0.001 + 0.998 * u))
            p[:, :K - 2] = kn[1:K - 1]
            assert bool(((p > kn[0]) & (p < kn[-1])).all())
            pts[name] = p
        col = lambda t: t.reshape(-1, 1)
        flat = lambda t: t.reshape(1, -1)
        # denominators, from the oracle's own pieces: bin width and height, den on both sides, the root's divisor
        for name, kn in (("x", kx), ("y", ky)):
            v = flat(pts[name])
            seg = O._segment_index(col(kn), v, 0)
            x0, x1, y0, y1, d0, d1 = O._gather6(*(col(k).expand(K, v.shape[1]) for k in (kx, ky, kd)), seg, 0)
            sl, curv = O._slope_terms(x0, x1, y0, y1, d0, d1)
            assert float((x1 - x0).min()) > 1e-2 and float((y1 - y0).min()) > 1e-2
            if name == "x":
                th = (v - x0) / (x1 - x0)
            else:
                eta = (v - y0) / (y1 - y0)
                a2, a0 = -curv * eta + d0 - sl, sl * eta
                bb = a2 + sl
                disc = torch.sqrt(bb * bb - 4 * a0 * a2)
                div = torch.where(bb >= 0, bb + disc, 2 * a2)
                assert float(div.abs().min()) > 0.1
                th = torch.where(bb >= 0, 2 * a0 / div, (bb - disc) / div)
            assert float(th.min()) >= 0.0 and float(th.max()) <= 1.0
            assert float((sl + curv * th * (1 - th)).min()) > 0.1
        fo, go = O.rqs_evaluate(col(kx), col(ky), col(kd), flat(pts["x"]), axis=0)
        bo, igo = O.rqs_invert(col(kx), col(ky), col(kd), flat(pts["y"]), axis=0)
        want = {False: (fo.reshape(3, 257), go.reshape(3, 257)), True: (bo.reshape(3, 257), igo.reshape(3, 257))}
    _SEG_CASES[K] = (kx, ky, kd, pts, want)
    return _SEG_CASES[K]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("K", [2, 5, 16])
def test_shared_segment_three_users_agree(K, dtype):
    """One rational-quadratic segment in the device code (nf_rqs_core.h), three users of it on ONE spline of K shared
    knots: RQSpline on nf_spline_eval (its own walk over global knots), DistConvFn with the spline stage alone (K4: binary
    search in LDS) and nf_distconv_sites for the per-site log-derivative -- forward and inverse, at points inside the knot
    range and ON every interior knot, each against the fp64 oracle's rqs_evaluate / rqs_invert.  The tolerances of
    test_rqspline_from_explicit_knots_vs_oracle: values 1e-10 (fp64) / 1e-5 (fp32), derivatives and log-derivatives 10x."""
    from normflow__amd.lib.spline import RQSpline
    tol = 1e-10 if dtype == torch.float64 else 1e-5
    kx, ky, kd, pts, want = _shared_segment_case(K)
    to = lambda t: t.to(DEV, dtype)
    sp = RQSpline(knots_x=to(kx), knots_y=to(ky), knots_d=to(kd), knots_axis=0)
    knots = to(torch.stack((kx, ky, kd)))
    for inverse in (False, True):
        v = to(pts["y" if inverse else "x"])
        val_o, der_o = want[inverse]                       # forward: g; inverse: 1 / g
        val_s, der_s = sp.backward(v, grad=True) if inverse else sp(v, grad=True)
        val_k, _ = _hip.DistConvFn.apply(v, knots, None, _hip.STAGE_SPLINE, inverse)
        val_d, dens = _hip.DistConvSitesFn.apply(v, knots, None, None, _hip.STAGE_SPLINE, inverse, True)
        errs = dict(spline=rel(val_s, val_o), k4=rel(val_k, val_o), sites=rel(val_d, val_o), deriv=rel(der_s, der_o),
                    dens=rel(dens, der_o.log()), log_deriv_vs_dens=rel(der_s.log(), dens))
        print(f"shared segment K={K} {dtype} inverse={inverse}: {errs}")
        assert max(errs["spline"], errs["k4"], errs["sites"]) <= tol, errs
        assert max(errs["deriv"], errs["dens"], errs["log_deriv_vs_dens"]) <= 10 * tol, errs


def test_make_spline_accepts_the_anti_periodic_alias():
    """extrap 'anti-periodic' = 'anti' (spline.py:448-456): the spline object's stored knots are augmented either way."""
    shape, B, m = (4, 6), 2, 5
    x, out = _rand_case(shape, B, m, 91, torch.float64)
    mask = EvenOddMask(shape=shape)
    sps = [RQSplineCoupling_([torch.nn.Identity()], mask=mask, xlim=(0.0, 2.0), ylim=(0.0, 2.0),
                             extrap={'left': name, 'right': 'linear'}).make_spline(out.to(DEV)) for name in ('anti', 'anti-periodic')]
    assert sps[0].knots_len == sps[1].knots_len == 2 * (m + 1) - 1
    for a, b in zip((sps[0].knots_x, sps[0].knots_y, sps[0].knots_d), (sps[1].knots_x, sps[1].knots_y, sps[1].knots_d)):
        assert torch.equal(a, b)
    v = (2.0 * x).unsqueeze(1).to(DEV)
    assert torch.equal(sps[0](v), sps[1](v))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_multirqs_fixed_knots_channels_axis_and_density(dtype):
    """MultiRQSplineCoupling_ (couplings_.py:342-412) beyond free knots: a fixed knots_x for one spline and a fixed knots_y
    for the other, the channels on the last axis, and propagate_density -- each against the oracle's single-spline atom
    applied per data channel."""
    torch.manual_seed(13)
    shape, B, m = (4, 6), 3, 5
    tol = 1e-9 if dtype == torch.float64 else 1e-5
    kxf = torch.tensor([-2.0, -0.8, 0.2, 1.1, 2.0], dtype=torch.float64, device='cpu')
    kyf = torch.tensor([-1.0, -0.1, 0.6, 2.0, 3.0], dtype=torch.float64, device='cpu')
    xlims, ylims = [(-2.0, 2.0), (-1.0, 3.0)], [(-2.0, 2.0), (-1.0, 3.0)]
    extraps = [{'left': 'linear', 'right': 'linear'}] * 2
    Cs = 2 * m - 1
    with torch.device("cpu"):
        out = 0.5 * torch.randn((B, 2 * Cs) + shape, dtype=torch.float64)
        x = 1.2 * torch.randn((B, 2) + shape, dtype=torch.float64)
    am = O.channel_mask(shape, 0)

    class Fixed(torch.nn.Module):
        def __init__(self, t):
            super().__init__()
            self.t = t

        def forward(self, _):
            return self.t
    mask = EvenOddMask(shape=shape)
    cpl = MultiRQSplineCoupling_([Fixed(out.to(DEV, dtype))], mask=mask, xlims=xlims, ylims=ylims,
                                 knots_x=[kxf, None], knots_y=[None, kyf], extraps=extraps)
    xa = (x * am).to(DEV, dtype)
    xf = (x * (1 - am)).to(DEV, dtype)
    want_v, want_l, want_sites = [], 0, []
    for i in range(2):
        kw = dict(xlim=xlims[i], ylim=ylims[i], extrap=extraps[i], knots_x=kxf if i == 0 else None,
                  knots_y=kyf if i == 1 else None)
        o_i = out[:, i * Cs:(i + 1) * Cs]
        v, l = O.rqs_coupling_atom(x[:, i] * am, o_i, am, **kw)
        want_v.append(v)
        want_l = want_l + l
        # per-site log g of this spline: evaluate a batch of one-site "samples"
        kx, ky, kd = O.knots_from_logits(o_i, kw['xlim'], kw['ylim'], kw['knots_x'], kw['knots_y'])
        kx, ky, kd = (O._bcast_like(k, o_i) for k in (kx, ky, kd))
        full = (B, kd.shape[1]) + shape
        kx, ky, kd = O.augment_knots(*(k.expand(full) for k in (kx, ky, kd)), axis=1, **extraps[i])
        _, g = O.rqs_evaluate(kx, ky, kd, (x[:, i] * am).unsqueeze(1), axis=1)
        want_sites.append(torch.log(g.squeeze(1)) * am)
    want_v, want_sites = torch.stack(want_v, 1), torch.stack(want_sites, 1)
    with torch.no_grad():
        y, lj = cpl.atomic_forward(x_active=xa, x_frozen=xf, parity=0, net=cpl.nets[0], log0=0)
        assert rel(y, want_v) <= tol and rel(lj, want_l) <= tol, (rel(y, want_v), rel(lj, want_l))
        xb, l0 = cpl.atomic_backward(x_active=y, x_frozen=xf, parity=0, net=cpl.nets[0], log0=lj)
        assert rel(xb, x * am) <= 100 * tol and float(l0.abs().max()) <= 100 * tol * max(1.0, float(want_l.abs().max()))
        # propagate_density: log0 + per-site log g of both splines
        cpl.propagate_density = True
        yd, dens = cpl.atomic_forward(x_active=xa, x_frozen=xf, parity=0, net=cpl.nets[0], log0=0)
        assert torch.equal(yd, y) and dens.shape == xa.shape and rel(dens, want_sites) <= tol
        cpl.propagate_density = False
        # channels on the last axis
        cpl2 = MultiRQSplineCoupling_([Fixed(out.movedim(1, -1).contiguous().to(DEV, dtype))], mask=mask, xlims=xlims,
                                      ylims=ylims, knots_x=[kxf, None], knots_y=[None, kyf], extraps=extraps, channels_axis=-1)
        y2, lj2 = cpl2.atomic_forward(x_active=xa.movedim(1, -1).contiguous(), x_frozen=xf, parity=0, net=cpl2.nets[0], log0=0)
        assert torch.equal(y2.movedim(-1, 1), y) and torch.equal(lj2, lj)
    # gradients through the fixed-knot multi atom (VJP kernels with batch strides) vs autograd through the oracle
    if dtype == torch.float64:
        p = out.to(DEV, dtype).clone().requires_grad_(True)
        cpl3 = MultiRQSplineCoupling_([Fixed(p)], mask=mask, xlims=xlims, ylims=ylims, knots_x=[kxf, None],
                                      knots_y=[None, kyf], extraps=extraps)
        xin = xa.clone().requires_grad_(True)
        yv, lv = cpl3.atomic_forward(x_active=xin, x_frozen=xf, parity=0, net=cpl3.nets[0], log0=0)
        gx, gp = torch.autograd.grad(lv.mean() + (yv ** 2).mean(), (xin, p))
        with torch.device("cpu"):
            xo, oo = (x * am).clone().requires_grad_(True), out.clone().requires_grad_(True)
            vs, ls = [], 0
            for i in range(2):
                v, l = O.rqs_coupling_atom(xo[:, i], oo[:, i * Cs:(i + 1) * Cs], am, xlim=xlims[i], ylim=ylims[i],
                                           extrap=extraps[i], knots_x=kxf if i == 0 else None, knots_y=kyf if i == 1 else None)
                vs.append(v)
                ls = ls + l
            go_x, go_p = torch.autograd.grad(ls.mean() + (torch.stack(vs, 1) ** 2).mean(), (xo, oo))
        assert rel(gx, go_x) <= 1e-8 and rel(gp, go_p) <= 1e-8


def test_normal_prior_sample_and_sample__share_one_stream():
    """After the same torch.manual_seed, `sample(B)` and `sample_(B)[0]` are the same configurations (the reference draws
    both through dist.sample, prior.py:22-28); with torch_rng=True both are torch's own stream."""
    from normflow__amd.prior import NormalPrior
    shape, B = (4, 6, 8), 5
    for kw in (dict(shape=shape), dict(loc=torch.full(shape, 0.3), scale=torch.full(shape, 1.7))):
        for torch_rng in (False, True):
            prior = NormalPrior(torch_rng=torch_rng, **kw)
            prior.to(DEV, torch.float32)
            torch.manual_seed(123)
            a = prior.sample(B)
            torch.manual_seed(123)
            b, logr = prior.sample_(B)
            assert a.shape == (B,) + shape and torch.equal(a, b)
            assert rel(logr, prior.log_prob(b)) <= 1e-5
            if torch_rng:
                torch.manual_seed(123)
                want = torch.normal(prior.loc.expand((B,) + shape), prior.scale.expand((B,) + shape))
                assert torch.equal(a, want)
            a2 = prior.sample(B)                      # the generator moved on
            assert not torch.equal(a, a2)


@pytest.mark.parametrize("shape", [(2, 4, 2, 32), (2, 2, 4, 48)])
@pytest.mark.parametrize("hidden", [4, 8, 5])
@pytest.mark.parametrize("m", [8, 10, 16, 3])
def test_split_fp16_chain_free_knots_len_and_hidden_width(m, hidden, shape, parity_report):
    """The reference leaves knots_len and the hidden widths free (src/nn/scalar/modules.py:68-154, couplings_.py:211-262):
    the split-fp16 chain takes any knots_len 2..16 (run-time cout = 3m - 2 <= 46 in the fused last layer) and hidden widths
    below 8 (weights zero-padded to the 8 channels of the pair tensor).  A whole coupling atom through the chain, forward and
    inverse, against the fp64 oracle at north_star's 1e-5, and against the unfused fp32 kernels; asserts the split kernel ran."""
    torch.manual_seed(100 * m + hidden)
    B, C = 5, 3 * m - 2
    acts = ['tanh', 'tanh', None]
    net = ConvAct(1, C, 3, conv_dim=4, hidden_sizes=[hidden, hidden], acts=acts).to(DEV, torch.float32)
    with torch.no_grad():
        for p_ in list(net.parameters())[-2:]:
            p_.mul_(0.3)
    mask = EvenOddMask(shape=shape)
    lim = dict(xlim=(-4.0, 4.0), ylim=(-4.0, 4.0), extrap={'left': 'linear', 'right': 'linear'})
    cpl = RQSplineCoupling_([net, net], mask=mask, **lim).to(DEV)
    x = 1.5 * torch.randn((B,) + shape, device=DEV, dtype=torch.float32)
    convs = [mod for mod in net if hasattr(mod, 'weight')]
    layers = [(c.weight.detach().double().cpu(), c.bias.detach().double().cpu()) for c in convs]
    for parity in (0, 1):
        xa, xf = mask.purify(x, parity), mask.purify(x, 1 - parity)
        l0 = torch.randn(B, device=DEV, dtype=torch.float32)
        with torch.no_grad():
            got = cpl._fused_atom(False, xa, xf, parity, net, l0)
            assert got is not None and _hip.load().nf_conv_last_path() == 3, "the split-fp16 fused kernel did not run"
            yf, lf = got
            with _hip.options(split16=False):                 # the same atom on the fp32 kernels (fused where m allows, else conv + K2)
                yu, lu = cpl.atomic_forward(x_active=xa, x_frozen=xf, parity=parity, net=net, log0=l0)
                assert _hip.load().nf_conv_last_path() != 3
            assert rel(yf, yu) <= 1e-5 and rel(lf, lu) <= 1e-5, (rel(yf, yu), rel(lf, lu))     # two fp32-level evaluations
            xb, lb = cpl._fused_atom(True, yf, xf, parity, net, lf)
            assert _hip.load().nf_conv_last_path() == 3
            y2, _ = cpl._fused_atom(False, xb, xf, parity, net, l0)
            assert rel(y2, yf) <= 2e-5, ("forward residual of the inverse", rel(y2, yf))
        out = O.conv_act(xf.double().cpu().unsqueeze(1), layers, acts)
        am = O.channel_mask(shape, parity)
        yo, lo = O.rqs_coupling_atom(xa.double().cpu(), out, am, log0=l0.double().cpu(), **lim)
        ey, el = rel(yf, yo), rel(lf, lo)
        parity_report(f"split chain m={m} hidden={hidden} {shape} p{parity}", "y / logJ vs fp64 oracle", max(ey, el), 1e-5)
        assert ey <= 1e-5 and el <= 1e-5, (ey, el)
        xo, l0o = O.rqs_coupling_atom(yo, out, am, inverse=True, log0=lo, **lim)
        assert rel(xo, xa) <= 1e-9           # (the oracle's own round trip: the inputs are well conditioned)


def test_config5_full_size_in_its_own_precision(parity_report):
    """BASELINE config 5 at its own size and in its own precision: 48^4, fp16 PARAMETERS (net_.to(float16)) and an fp16 FIELD,
    fp32 log-det, mixed affine + RQ-spline blocks (ConvAct 1-8-8-C, m = 16), every atom on the split-fp16 chain.
    Size-independent properties on 2 samples: outputs half / log|J| fp32 and finite, frozen sites exactly zero after every
    atom, batch permutation bitwise, split-fp16 products == exact fp32 products up to one half-ulp of the stored field on 99 % of
    the sites after 4 layers, the
    inverse undoes the forward to half's resolution; and ONE spline layer and ONE affine layer at full size against the fp64
    oracle on the same half-rounded inputs (value: the oracle's result rounded to half, up to one half-ulp + the fp32 bound;
    log-det increment 1e-5)."""
    torch.manual_seed(48)
    shape, B, m = (48, 48, 48, 48), 2, 16
    mask = EvenOddMask(shape=shape)
    lim = dict(xlim=(-5.0, 5.0), ylim=(-5.0, 5.0), extrap={'left': 'linear', 'right': 'linear'})
    blocks = []
    for kind in ('affine', 'rqs'):
        C = 2 if kind == 'affine' else 3 * m - 2
        nets = [ConvAct(1, C, 3, conv_dim=4, hidden_sizes=[8, 8], acts=['tanh', 'tanh', None]) for _ in range(2)]
        for net in nets:
            with torch.no_grad():
                for p_ in list(net.parameters())[-2:]:
                    p_.mul_(0.3)
        blocks.append(AffineCoupling_(nets, mask=mask) if kind == 'affine' else RQSplineCoupling_(nets, mask=mask, **lim))
    net_ = ModuleList_(blocks)
    net_.to(device=DEV, dtype=torch.float16)
    x = torch.randn((B,) + shape, device=DEV, dtype=torch.float32).half()
    with torch.no_grad():
        y, lj = net_(x)
        assert _hip.load().nf_conv_last_path() == 3, "the split-fp16 kernels did not run"
        perm = torch.tensor([1, 0], device=DEV)
        yp, ljp = net_(x[perm])
        xb, lb = net_.backward(y, lj)
        with _hip.options(split16=False):
            y32, lj32 = net_(x[:1])
    assert y.dtype == torch.float16 and lj.dtype == torch.float32 and bool(torch.isfinite(y).all()) and bool(torch.isfinite(lj).all())
    assert torch.equal(yp, y[perm]) and torch.equal(ljp, lj[perm])
    assert rel(xb, x) <= 2e-2 and float(lb.abs().max()) <= 1e-3 * max(1.0, float(lj.abs().max()))      # 4 layers of half storage
    # the two product arithmetics agree to a half-ulp of the stored field on (nearly) every site, log|J| to 1e-5
    d = (y[:1].double() - y32.double()).abs()
    ulp = y32.double().abs().clamp_min(2.0 ** -14) * 2.0 ** -10
    # (a rounding that falls the other way in one layer is a different input, one half-ulp away, for the layers behind it)
    off1 = float((d > ulp).double().mean())
    parity_report("config 5, 48^4 fp16 storage, 4 layers", "split vs fp32 products: sites off by > 1 half-ulp", off1, 1e-2)
    assert off1 <= 1e-2 and rel(y[:1], y32) <= 5e-3 and rel(lj[:1], lj32) <= 1e-5, (off1, rel(y[:1], y32), rel(lj[:1], lj32))
    # one atom of each kind at full size: frozen sites exactly zero, and the fp64 oracle on the same half-rounded inputs
    half = lambda t: t.to(torch.float16).to(torch.float64)
    for blk in blocks:
        kind = 'affine' if isinstance(blk, AffineCoupling_) else 'rqs'
        net = blk.nets[0]
        xa, xf = mask.purify(x[:1], 0), mask.purify(x[:1], 1)
        l0 = torch.randn(1, device=DEV, dtype=torch.float32)
        with torch.no_grad():
            yg, lg = blk.atomic_forward(x_active=xa, x_frozen=xf, parity=0, net=net, log0=l0)
        assert yg.dtype == torch.float16 and lg.dtype == torch.float32
        am = O.channel_mask(shape, 0)
        assert float(yg.double().cpu().mul(1 - am).abs().max()) == 0.0          # frozen sites: exactly zero
        convs = [mod for mod in net if hasattr(mod, 'weight')]
        layers = [(c.weight.detach().double().cpu(), c.bias.detach().double().cpu()) for c in convs]
        out = O.conv_act(half(xf.cpu()).unsqueeze(1), layers, ['tanh', 'tanh', None])
        atom = O.affine_coupling_atom if kind == 'affine' else O.rqs_coupling_atom
        yo, lo = atom(half(xa.cpu()), out, am, log0=l0.double().cpu(), **({} if kind == 'affine' else lim))
        del out
        want = half(yo)
        diff = (yg.double().cpu() - want).abs()
        bound = want.abs().clamp_min(2.0 ** -14) * 2.0 ** -10 + 1e-5 * max(1.0, float(want.abs().max()))
        worst, off = float((diff / bound).max()), float((diff > 0).double().mean())
        parity_report(f"config 5, 48^4 fp16 storage, one {kind} layer", "y: worst err / (half-ulp + 1e-5)", worst, 1.0, f"{100 * off:.2f} % of sites off by a rounding")
        parity_report(f"config 5, 48^4 fp16 storage, one {kind} layer", "logJ vs fp64 oracle", rel(lg, lo), 1e-5)
        assert worst <= 1.0 + 1e-9 and off <= 0.02 and rel(lg, lo) <= 1e-5, (kind, worst, off, rel(lg, lo))


@pytest.mark.parametrize("shape,B,m,hidden,acts", [((16, 16, 16), 5, 16, 8, ('tanh', 'tanh')), ((4, 6, 16), 300, 16, 8, ('tanh', 'tanh')),
                                                   ((2, 2, 16), 7, 8, 4, ('tanh', 'expit')), ((1, 4, 16), 3, 5, 8, ('expit', 'tanh')),
                                                   ((5, 16, 16), 4, 10, 5, ('tanh', 'tanh')), ((16, 16, 16), 2, 3, 8, ('tanh', 'tanh'))])
def test_small3d_fused_layer_vs_oracle(shape, B, m, hidden, acts, parity_report):
    """nf_conv_s.hip (K5s): a whole RQ-spline coupling atom of a small 3-D lattice -- BASELINE config 3's 16^3 and smaller --
    in ONE launch with the sample resident in LDS: ConvAct 1 -> h -> h -> 3m-2 on split-fp16 products + the spline.  Forward
    and inverse against the fp64 oracle at north_star's 1e-5 (y, log|J|), against the fp32 kernels, batch order bitwise,
    more samples than workgroups; asserts that this kernel is the one that ran."""
    torch.manual_seed(7 * m + hidden)
    Cc = 3 * m - 2
    act_list = [acts[0], acts[1], None]
    net = ConvAct(1, Cc, 3, conv_dim=3, hidden_sizes=[hidden, hidden], acts=act_list).to(DEV, torch.float32)
    with torch.no_grad():
        for p_ in list(net.parameters())[-2:]:
            p_.mul_(0.3)
    mask = EvenOddMask(shape=shape)
    lim = dict(xlim=(-4.0, 4.0), ylim=(-4.0, 4.0), extrap={'left': 'linear', 'right': 'linear'})
    cpl = RQSplineCoupling_([net, net], mask=mask, **lim).to(DEV)
    x = 1.5 * torch.randn((B,) + shape, device=DEV, dtype=torch.float32)
    assert net.small3d_plan() is not None
    assert _hip.load().nf_small_lattice_supported(_hip._c_ints(shape), 3, 0, Cc, m, _hip.ACT_CODES[acts[0]], _hip.ACT_CODES[acts[1]])
    opts = _hip.make_rqs_opts(m, lim["xlim"], lim["ylim"], lim["extrap"], _hip.LAYOUT_PAIR)
    convs = [mod for mod in net if hasattr(mod, 'weight')]
    layers = [(c.weight.detach().double().cpu(), c.bias.detach().double().cpu()) for c in convs]
    nb = min(B, 6)
    for parity in (0, 1):
        xa, xf = mask.purify(x, parity), mask.purify(x, 1 - parity)
        l0 = torch.randn(B, device=DEV, dtype=torch.float32)
        with torch.no_grad():
            got = cpl._small_lattice_atom(0, False, xa, xf, parity, net, l0, opts)
            assert got is not None, "the small-lattice fused kernel did not take this layer"
            yf, lf = got
            yv, lv = cpl.atomic_forward(x_active=xa, x_frozen=xf, parity=parity, net=net, log0=l0)     # the API takes the same path
            assert torch.equal(yv, yf) and torch.equal(lv, lf)
            with _hip.options(split16=False):
                yu, lu = cpl.atomic_forward(x_active=xa, x_frozen=xf, parity=parity, net=net, log0=l0)
            assert rel(yf, yu) <= 1e-5 and rel(lf, lu) <= 1e-5, (rel(yf, yu), rel(lf, lu))
            perm = torch.randperm(B, device=DEV)
            yp, lp = cpl._small_lattice_atom(0, False, xa[perm], xf[perm], parity, net, l0[perm], opts)
            assert torch.equal(yp, yf[perm]) and torch.equal(lp, lf[perm])
            xb, lb = cpl._small_lattice_atom(0, True, yf, xf, parity, net, lf, opts)
            y2, _ = cpl._small_lattice_atom(0, False, xb, xf, parity, net, l0, opts)
            assert rel(y2, yf) <= 2e-5, ("forward residual of the inverse", rel(y2, yf))
        am = O.channel_mask(shape, parity)
        assert float((yf.double().cpu() * (1 - am)).abs().max()) == 0.0            # frozen sites: exactly zero
        out = O.conv_act(xf[:nb].double().cpu().unsqueeze(1), layers, act_list)
        yo, lo = O.rqs_coupling_atom(xa[:nb].double().cpu(), out, am, log0=l0[:nb].double().cpu(), **lim)
        ey, el = rel(yf[:nb], yo), rel(lf[:nb], lo)
        parity_report(f"small3d {shape} m={m} h={hidden} p{parity}", "y / logJ vs fp64 oracle", max(ey, el), 1e-5)
        assert ey <= 1e-5 and el <= 1e-5, (ey, el)
        xo, _ = O.rqs_coupling_atom(yf[:nb].double().cpu(), out, am, inverse=True, log0=lf[:nb].double().cpu(), **lim)
        # the inverse against the oracle's inverse of the SAME y: conditioned by 1/g, bounded through the forward residual above
        assert rel(xb[:nb], xo) <= 1e-3


@pytest.mark.parametrize("shape,m,B", [((2, 2, 4, 32), 16, 3), ((2, 4, 2, 48), 16, 2), ((2, 2, 2, 32), 8, 4)])
@pytest.mark.parametrize("inverse", [False, True])
def test_fused_last_layer_spline_vjp_vs_autograd_through_oracle(shape, m, B, inverse, parity_report):
    """Training path (Fitter.step, src/_normflowcore.py:275-294): with gradients required the last ConvAct layer and the spline
    are ONE differentiable node (`_hip.FusedLastRqsFn`: nf_conv_rqs_split16_train forward, nf_conv_rqs_split16_vjp backward,
    logits recomputed in the kernel and never materialised).  Values and the gradients of mean(log|J|) + mean(out^2) with
    respect to the field and to every parameter of the net, against autograd through the fp64 oracle, and against the
    unfused GPU path (conv stack with materialised logits + nf_rqs_*_vjp)."""
    torch.manual_seed(3 * m + len(shape) + int(inverse))
    Cc = 3 * m - 2
    acts = ['tanh', 'tanh', None]
    net = ConvAct(1, Cc, 3, conv_dim=4, hidden_sizes=[8, 8], acts=acts).to(DEV, torch.float32)
    with torch.no_grad():
        for p_ in list(net.parameters())[-2:]:
            p_.mul_(0.3)
    mask = EvenOddMask(shape=shape)
    lim = dict(xlim=(-4.0, 4.0), ylim=(-4.0, 4.0), extrap={'left': 'linear', 'right': 'linear'})
    cpl = RQSplineCoupling_([net, net], mask=mask, **lim).to(DEV)
    params = list(net.parameters())
    x = 1.3 * torch.randn((B,) + shape, device=DEV, dtype=torch.float32)
    parity = 1
    am = O.channel_mask(shape, parity)
    xa0, xf0 = mask.purify(x, parity), mask.purify(x, 1 - parity)
    l0 = torch.randn(B, device=DEV, dtype=torch.float32)

    def run(fused):
        xa, xf = xa0.clone().requires_grad_(True), xf0.clone().requires_grad_(True)
        if fused:
            got = cpl._train_fused_atom(inverse, xa, xf, parity, net, l0)
            assert got is not None, "the differentiable fused node did not take this layer"
            val, lj = got
        else:
            k = lambda v, p, l, act, layout: _hip.RQSCouplingFn.apply(v, p, l, act, cpl._opts(p.shape[1], layout, v), inverse)
            val, lj = cpl._run_atom(k, xa, xf, parity, net, l0, Cc)
        loss = lj.mean() + (val ** 2).mean()
        grads = torch.autograd.grad(loss, [xa, xf] + params)
        return val.detach(), lj.detach(), [g_.detach() for g_ in grads]

    from normflow__amd.nn.scalar import couplings_
    old_thr = couplings_.set_training_fusion(0)          # always fused (the default fuses atoms whose logits exceed 1 GiB)
    try:
        vf, lf, gf = run(True)
        vu, lu, gu = run(False)
        # the API takes the fused node by itself when gradients are required
        xa, xf = xa0.clone().requires_grad_(True), xf0.clone()
        fn = cpl.atomic_backward if inverse else cpl.atomic_forward
        va, la = fn(x_active=xa, x_frozen=xf, parity=parity, net=net, log0=l0)
        assert torch.equal(va, vf) and torch.equal(la, lf) and va.grad_fn is not None
        couplings_.set_training_fusion(1 << 62)          # never: the same call materialises the logits
        vb, lb = fn(x_active=xa, x_frozen=xf, parity=parity, net=net, log0=l0)
        assert torch.equal(vb, vu) and torch.equal(lb, lu)
    finally:
        couplings_.set_training_fusion(old_thr)
    # the oracle, fp64, autograd
    with torch.device("cpu"):
        convs = [mod for mod in net if hasattr(mod, 'weight')]
        leaves = [(c.weight.detach().double().cpu().requires_grad_(True), c.bias.detach().double().cpu().requires_grad_(True)) for c in convs]
        xao, xfo = xa0.double().cpu().requires_grad_(True), xf0.double().cpu().requires_grad_(True)
        out = O.conv_act(xfo.unsqueeze(1), leaves, acts)
        vo, lo = O.rqs_coupling_atom(xao, out, am, inverse=inverse, log0=l0.double().cpu(), **lim)
        loss = lo.mean() + (vo ** 2).mean()
        flat = [xao, xfo] + [t for wb in leaves for t in wb]
        go = torch.autograd.grad(loss, flat)
    # parameter order of the module: weight, bias per conv (Conv4d keeps its weight in the lower-dimensional container)
    def as_module_order(glist):
        outl = list(glist[:2])
        k = 2
        for c in convs:
            outl.append((c, glist[k], glist[k + 1]))
            k += 2
        return outl
    assert rel(vf, vo) <= 2e-5 and rel(lf, lo) <= 1e-5, (rel(vf, vo), rel(lf, lo))
    names = ["grad x_active", "grad x_frozen"] + [f"grad {n_}" for n_, _ in net.named_parameters()]
    ref = {"grad x_active": go[0], "grad x_frozen": go[1]}
    k = 2
    for ci, c in zip((0, 2, 4), convs):
        ref[f"grad {ci}._conv_lower_dim.weight"] = go[k].movedim(2, 1).reshape(c._conv_lower_dim.weight.shape)
        ref[f"grad {ci}.bias"] = go[k + 1]
        k += 2
    worst = 0.0
    for name, a_, b_ in zip(names, gf, gu):
        want = ref[name]
        e_or, e_un = rel(a_, want) / max(1e-30, float(want.abs().max())) * max(1.0, float(want.abs().max())), rel(a_, b_)
        scale = max(1e-30, float(want.abs().max()))
        e_or = float((a_.double().cpu() - want).abs().max()) / scale           # relative to the gradient's own largest entry
        e_un = float((a_ - b_).abs().max()) / scale
        worst = max(worst, e_or)
        assert e_or <= 2e-4 and e_un <= 2e-4, (name, e_or, e_un)
    parity_report(f"fused VJP {shape} m={m} inverse={inverse}", "worst gradient vs oracle (rel. to its max)", worst, 2e-4)


@pytest.mark.parametrize("shape,B,kind,m,hidden", [((16, 16), 512, 'affine', 0, 8), ((16, 16), 9, 'rqs', 16, 8), ((6, 16), 300, 'affine', 0, 4),
                                                   ((4, 16), 5, 'rqs', 8, 5), ((16, 16, 16), 3, 'affine', 0, 8), ((3, 8, 16), 7, 'affine', 0, 8)])
def test_small_lattice_affine_and_2d_vs_oracle(shape, B, kind, m, hidden, parity_report):
    """K5s (nf_small_lattice_coupling) beyond the 3-D spline atom: the AFFINE coupling (couplings_.py:123-139) and 2-D lattices
    (BASELINE config 2: 16 x 16, affine, batch 512) -- the whole atom, parameter net included, in one launch.  Forward and
    inverse against the fp64 oracle at 1e-5, against the fp32 kernels, batch order bitwise, frozen sites exactly zero; and the
    API (`atomic_forward`) takes this path by itself."""
    torch.manual_seed(11 * len(shape) + hidden + m)
    d = len(shape)
    Cc = 2 if kind == 'affine' else 3 * m - 2
    acts = ['tanh', 'tanh', None]
    net = ConvAct(1, Cc, 3, conv_dim=d, hidden_sizes=[hidden, hidden], acts=acts).to(DEV, torch.float32)
    with torch.no_grad():
        for p_ in list(net.parameters())[-2:]:
            p_.mul_(0.3)
    mask = EvenOddMask(shape=shape)
    lim = dict(xlim=(-4.0, 4.0), ylim=(-4.0, 4.0), extrap={'left': 'linear', 'right': 'linear'})
    cpl = (AffineCoupling_([net, net], mask=mask) if kind == 'affine' else RQSplineCoupling_([net, net], mask=mask, **lim)).to(DEV)
    x = 1.3 * torch.randn((B,) + shape, device=DEV, dtype=torch.float32)
    convs = [mod for mod in net if hasattr(mod, 'weight')]
    layers = [(c.weight.detach().double().cpu(), c.bias.detach().double().cpu()) for c in convs]
    nb = min(B, 8)
    opts = None if kind == 'affine' else _hip.make_rqs_opts(m, lim["xlim"], lim["ylim"], lim["extrap"], _hip.LAYOUT_PAIR)
    for parity in (0, 1):
        xa, xf = mask.purify(x, parity), mask.purify(x, 1 - parity)
        l0 = torch.randn(B, device=DEV, dtype=torch.float32)
        with torch.no_grad():
            got = cpl._small_lattice_atom(1 if kind == 'affine' else 0, False, xa, xf, parity, net, l0, opts)
            assert got is not None, "the small-lattice fused kernel did not take this layer"
            yf, lf = got
            yv, lv = cpl.atomic_forward(x_active=xa, x_frozen=xf, parity=parity, net=net, log0=l0)
            assert torch.equal(yv, yf) and torch.equal(lv, lf)
            with _hip.options(split16=False):
                yu, lu = cpl.atomic_forward(x_active=xa, x_frozen=xf, parity=parity, net=net, log0=l0)
            assert rel(yf, yu) <= 1e-5 and rel(lf, lu) <= 1e-5, (rel(yf, yu), rel(lf, lu))
            perm = torch.randperm(B, device=DEV)
            yp, lp = cpl.atomic_forward(x_active=xa[perm], x_frozen=xf[perm], parity=parity, net=net, log0=l0[perm])
            assert torch.equal(yp, yf[perm]) and torch.equal(lp, lf[perm])
            xb, lb = cpl.atomic_backward(x_active=yf, x_frozen=xf, parity=parity, net=net, log0=lf)
        am = O.channel_mask(shape, parity)
        assert float((yf.double().cpu() * (1 - am)).abs().max()) == 0.0
        out = O.conv_act(xf[:nb].double().cpu().unsqueeze(1), layers, acts)
        atom = O.affine_coupling_atom if kind == 'affine' else O.rqs_coupling_atom
        kw = {} if kind == 'affine' else lim
        yo, lo = atom(xa[:nb].double().cpu(), out, am, log0=l0[:nb].double().cpu(), **kw)
        ey, el = rel(yf[:nb], yo), rel(lf[:nb], lo)
        parity_report(f"small lattice {kind} {shape} h={hidden} p{parity}", "y / logJ vs fp64 oracle", max(ey, el), 1e-5)
        assert ey <= 1e-5 and el <= 1e-5, (ey, el)
        if kind == 'affine':        # x = (y - t) e^{|s|}: conditioned by e^{|s|} <= e^2 here
            assert rel(xb, xa) <= 2e-5 and rel(lb, l0) <= 2e-5, (rel(xb, xa), rel(lb, l0))
        else:
            with torch.no_grad():
                y2, _ = cpl.atomic_forward(x_active=xb, x_frozen=xf, parity=parity, net=net, log0=l0)
            assert rel(y2, yf) <= 2e-5


from test_oracle_golden import small16_cases, SMALL16_LIM


@pytest.mark.parametrize("tag", small16_cases())
def test_small_lattice_kernel_against_reference_goldens(golden, tag, parity_report):
    """nf_conv_s.hip against the REFERENCE itself (tests/golden/small16.npz, written by make_golden_small16.py from the imported
    reference): whole Coupling_ blocks with the reference's weights (same state_dict keys) on 2-D / 3-D lattices with a 16-site
    fastest axis -- BASELINE config 2's 16 x 16 affine block and config 3's net on 4 x 6 x 16 among them.  fp32, no_grad (the
    fused path), forward and inverse: north_star's 1e-5 on y and log|J|."""
    z = golden("small16")
    kind = tag.split("/")[0]
    shape = tuple(int(v) for v in z[f"{tag}/shape"])
    m, hidden, d = int(z[f"{tag}/m"]), int(z[f"{tag}/hidden"]), len(shape)
    n_out = 2 if kind == "affine" else 3 * m - 2
    nets = [ConvAct(1, n_out, 3, conv_dim=d, hidden_sizes=[hidden, hidden], acts=['tanh', 'tanh', None]) for _ in range(2)]
    mask = EvenOddMask(shape=shape)
    cpl = AffineCoupling_(nets, mask=mask) if kind == "affine" else RQSplineCoupling_(nets, mask=mask, **SMALL16_LIM)
    sd = {k.split("/param/")[1]: torch.from_numpy(z[k]) for k in z.files if k.startswith(f"{tag}/param/")}
    missing, unexpected = cpl.load_state_dict(sd, strict=False)
    assert not unexpected and set(missing) == {"mask._mask", "mask._c_mask"}
    cpl = cpl.to(device=DEV, dtype=torch.float32)
    x = T(z[f"{tag}/x"], torch.float32)
    with torch.no_grad():
        xa, xf = mask.purify(x, 0), mask.purify(x, 1)
        so = None if kind == "affine" else _hip.make_rqs_opts(m, (-3.0, 3.0), (-3.0, 3.0), SMALL16_LIM["extrap"], _hip.LAYOUT_PAIR)
        took = cpl._small_lattice_atom(1 if kind == "affine" else 0, False, xa, xf, 0, cpl.nets[0], 0, so)
        assert took is not None, "the small-lattice fused kernel did not take this block"
        y, logJ = cpl(x)
        xh, lrt = cpl.backward(T(z[f"{tag}/y"], torch.float32), T(z[f"{tag}/logJ"], torch.float32))
        y2, _ = cpl(xh)
    ey, el = rel(y, z[f"{tag}/y"]), rel(logJ, z[f"{tag}/logJ"])
    parity_report(f"small16 {tag}", "y / logJ vs the reference", max(ey, el), 1e-5)
    assert ey <= 1e-5 and el <= 1e-5, (ey, el)
    assert rel(y2, z[f"{tag}/y"]) <= 2e-5                      # the inverse, through its forward residual
    if kind == "affine":
        assert rel(xh, z[f"{tag}/x"]) <= 2e-5 and float(lrt.abs().max()) <= 2e-5 * max(1.0, float(np.abs(z[f"{tag}/logJ"]).max()))


def test_small_lattice_kernel_edge_cases():
    """nf_small_lattice_coupling at its edges: empty batch, one sample, far more samples than workgroups (persistent loop),
    non-contiguous inputs, unsupported shapes fall back
    to the other kernels with the same results, CPU tensors refused."""
    torch.manual_seed(5)
    shape, m = (2, 4, 16), 16
    net = ConvAct(1, 3 * m - 2, 3, conv_dim=3, hidden_sizes=[8, 8], acts=['tanh', 'tanh', None]).to(DEV, torch.float32)
    with torch.no_grad():
        for p_ in list(net.parameters())[-2:]:
            p_.mul_(0.3)
    mask = EvenOddMask(shape=shape)
    lim = dict(xlim=(-4.0, 4.0), ylim=(-4.0, 4.0), extrap={'left': 'linear', 'right': 'linear'})
    cpl = RQSplineCoupling_([net, net], mask=mask, **lim).to(DEV)
    with torch.no_grad():
        # empty batch
        x0 = torch.empty((0,) + shape, device=DEV, dtype=torch.float32)
        y0, l0 = cpl(x0)
        assert y0.shape == x0.shape and l0.shape == (0,)
        # one sample / many samples
        x = 1.2 * torch.randn((1500,) + shape, device=DEV, dtype=torch.float32)
        y, lj = cpl(x)
        y1, l1 = cpl(x[:1])
        assert torch.equal(y1, y[:1]) and torch.equal(l1, lj[:1])
        # non-contiguous input (a strided view): same result as its contiguous copy
        xs = torch.randn((40,) + shape + (2,), device=DEV, dtype=torch.float32)[..., 0]
        assert not xs.is_contiguous()
        ya, la = cpl(xs)
        yb, lb = cpl(xs.contiguous())
        assert torch.equal(ya, yb) and torch.equal(la, lb)
        # a lattice the kernel does not take (fastest axis 8): the other kernels, same API
        mask8 = EvenOddMask(shape=(2, 4, 8))
        cpl8 = RQSplineCoupling_([net, net], mask=mask8, **lim).to(DEV)
        x8 = torch.randn((3, 2, 4, 8), device=DEV, dtype=torch.float32)
        assert cpl8._small_lattice_atom(0, False, mask8.purify(x8, 0), mask8.purify(x8, 1), 0, net, 0,
                                        _hip.make_rqs_opts(m, lim["xlim"], lim["ylim"], lim["extrap"], _hip.LAYOUT_PAIR)) is None
        y8, l8 = cpl8(x8)
        xb8, lb8 = cpl8.backward(y8, l8)
        y8b, _ = cpl8(xb8)
        assert rel(y8b, y8) <= 1e-4
    with pytest.raises(_hip.NormflowHipError):
        packed, biases, acts, cout = net.small3d_plan()
        cpu0 = torch.zeros((1,) + shape, device='cpu', dtype=torch.float32)
        _hip.small_lattice_coupling(0, cpu0, cpu0, packed, biases, None, 0, cout, acts,
                                    _hip.make_rqs_opts(m, (-4, 4), (-4, 4), lim["extrap"], _hip.LAYOUT_PAIR), False)


@pytest.mark.parametrize("shape,kinds,B", [((16, 16), ['affine'] * 2 + ['rqs'], 32), ((6, 8, 16), ['rqs'] * 2, 8),
                                            ((2, 2, 4, 32), ['rqs', 'affine'], 4)])
def test_graphed_train_step_equals_the_eager_step(shape, kinds, B):
    """GraphedTrainStep (forward + reverse-KL loss + backward of Fitter.step, reference src/_normflowcore.py:275-294, replayed
    from one HIP graph) against the eager step on the same draws: loss, log q/p and every parameter's gradient bit for bit,
    also AFTER optimiser steps (the weight repacking is part of the graph: a replay must use the current values), and through
    the guard that re-captures when a weight leaves the range the split-fp16 kernels were validated for."""
    import normflow__amd as nf
    from normflow__amd.prior import NormalPrior
    from normflow__amd.action import ScalarPhi4Action
    from normflow__amd.fitter import kl_mean
    torch.manual_seed(11)
    mask = EvenOddMask(shape=shape)
    lim = dict(xlim=(-5.0, 5.0), ylim=(-5.0, 5.0), extrap={'left': 'linear', 'right': 'linear'})
    mk = lambda c: ConvAct(1, c, 3, conv_dim=len(shape), hidden_sizes=[8, 8], acts=['tanh', 'tanh', None])
    net_ = ModuleList_([RQSplineCoupling_([mk(46)], mask=mask, **lim) if k == 'rqs' else AffineCoupling_([mk(2)], mask=mask)
                        for k in kinds])
    net_.to(device=DEV, dtype=torch.float32)
    prior = NormalPrior(loc=torch.zeros(shape, device=DEV, dtype=torch.float32),
                        scale=torch.ones(shape, device=DEV, dtype=torch.float32))
    model = nf.Model(net_=net_, prior=prior, action=ScalarPhi4Action(kappa=0.67, m_sq=-4 * 0.67, lambd=0.5))
    params = list(net_.parameters())
    opt = torch.optim.Adam(params, lr=1e-2)

    def eager(x, logr):
        for p in params:
            p.grad = None
        y, logj = net_(x)
        logq, logp = logr - logj, -model.action(y)
        loss = kl_mean(logq, logp)
        loss.backward()
        return loss.detach().clone(), (logq - logp).detach().clone(), [p.grad.clone() for p in params]

    state = torch.cuda.get_rng_state(DEV)
    step = nf.GraphedTrainStep(model, kl_mean, B)
    assert torch.equal(state, torch.cuda.get_rng_state(DEV))        # the capture's example draw left the stream alone
    for it in range(4):
        x, logr = prior.sample_(B)
        if it == 3:                                                   # outside the validated range: the guard re-captures
            with torch.no_grad():
                params[0].view(-1)[0] = 40.0
        with _hip.options(split16=it < 3):                            # (the re-captured graph runs the exact fp32 kernels)
            l0, d0, g0 = eager(x, logr)
        l1, d1 = step(x, logr)
        assert torch.equal(l0, l1) and torch.equal(d0, d1), (it, float(l0), float(l1))
        for p, g in zip(params, g0):
            if it < 3 or len(shape) < 4:
                assert torch.equal(p.grad, g), (it, float((p.grad - g).abs().max()))
            else:           # (4-D layers off the split-fp16 chain: nf_conv_wgrad adds its partial sums with float atomics)
                assert float((p.grad - g).abs().max()) <= 1e-5 * float(g.abs().max()), it
        opt.step()
    with pytest.raises(ValueError):
        step(torch.zeros((B + 1,) + shape, device=DEV, dtype=torch.float32), torch.zeros(B + 1, device=DEV, dtype=torch.float32))


def test_fit_graphed_reproduces_the_eager_loss_history():
    """model.fit(..., graphed=True) == model.fit(...) epoch by epoch (same seed): the option changes how a step is launched,
    not what it computes."""
    import copy
    import normflow__amd as nf
    from normflow__amd.prior import NormalPrior
    from normflow__amd.action import ScalarPhi4Action
    shape = (8, 8)
    mask = EvenOddMask(shape=shape)
    mk = lambda c: ConvAct(1, c, 3, conv_dim=2, hidden_sizes=[8, 8], acts=['tanh', 'tanh', None])
    torch.manual_seed(4)
    net0 = ModuleList_([AffineCoupling_([mk(2)], mask=mask), RQSplineCoupling_([mk(22)], mask=mask, xlim=(-5, 5), ylim=(-5, 5),
                                                                              extrap={'left': 'linear', 'right': 'linear'})])
    hist = []
    for graphed in (False, True):
        net_ = copy.deepcopy(net0)
        net_.to(device=DEV, dtype=torch.float32)
        prior = NormalPrior(loc=torch.zeros(shape, device=DEV, dtype=torch.float32),
                            scale=torch.ones(shape, device=DEV, dtype=torch.float32))
        model = nf.Model(net_=net_, prior=prior, action=ScalarPhi4Action(kappa=0.67, m_sq=-4 * 0.67, lambd=0.5))
        torch.manual_seed(9)
        model.fit(n_epochs=12, batch_size=64, hyperparam=dict(lr=0.01), checkpoint_dict=dict(print_stride=1000), graphed=graphed)
        hist.append(list(model.fit.train_history['loss']))
    assert hist[0] == hist[1], (hist[0][-3:], hist[1][-3:])


@pytest.mark.parametrize("lattice,cin,cout,B", [((16, 16, 16), 8, 46, 160), ((16, 16, 16), 8, 8, 160), ((16, 16, 16), 1, 8, 33),
                                                ((16, 16), 8, 2, 512), ((12, 10), 8, 22, 7), ((6, 6, 10), 3, 46, 5)])
def test_conv_wgrad_sites_kernel_vs_autograd(lattice, cin, cout, B):
    """nf_conv_wgrad_sites (few-column layers: the waves split the sites; pair-compact cotangents walked at their active sites
    only; fixed-order sums) against autograd through a circular fp64 convolution (torch, the definition the oracle's
    circular_conv_direct restates; reference: src/nn/scalar/convNd.py:86-126 differentiated by src/_normflowcore.py:288):
    full and pair-compact cotangents of both parities, more items than workgroups, non-power-of-two lattices, and the
    same bits on a second run."""
    import torch.nn.functional as F
    d = len(lattice)
    g = torch.Generator(device='cpu').manual_seed(B + cout)
    x = torch.randn((B, cin) + lattice, generator=g, dtype=torch.float32, device='cpu').to(DEV)
    gz = torch.randn((B, cout) + lattice, generator=g, dtype=torch.float32, device='cpu').to(DEV)
    conv = {1: F.conv1d, 2: F.conv2d, 3: F.conv3d}[d]
    w = torch.zeros((cout, cin) + (3,) * d, dtype=torch.float64, device=DEV, requires_grad=True)
    bias = torch.zeros(cout, dtype=torch.float64, device=DEV, requires_grad=True)
    out = conv(F.pad(x.double(), (1, 1) * d, mode='circular'), w, bias)
    V = x[0, 0].numel()
    coords = torch.stack(torch.meshgrid(*[torch.arange(n, device=DEV) for n in lattice], indexing='ij')).sum(0)
    for parity in (-1, 0, 1):
        if parity < 0:
            cot, gzk = gz, gz
        else:
            act = (coords % 2 == parity)
            cot = gz * act
            gzk = gz.reshape(B, cout, V)[:, :, act.reshape(-1)].contiguous()      # pair-compact: the active site of every pair
        gw0, gb0 = torch.autograd.grad(out, (w, bias), cot.double(), retain_graph=True)
        got = _hip.conv_weight_grad(x, gzk, (3,) * d, None, parity)
        assert got is not None
        gw, gb = got
        scale = float(gw0.abs().max())
        assert float((gw.double() - gw0).abs().max()) <= 2e-5 * scale, (parity, float((gw.double() - gw0).abs().max()), scale)
        assert float((gb.double() - gb0).abs().max()) <= 2e-5 * max(1.0, float(gb0.abs().max()))
        gw2, gb2 = _hip.conv_weight_grad(x, gzk, (3,) * d, None, parity)
        assert torch.equal(gw, gw2) and torch.equal(gb, gb2)
    if cout <= 8:                                                     # the fp64 instance
        gw0, gb0 = torch.autograd.grad(out, (w, bias), gz.double())
        gw, gb = _hip.conv_weight_grad(x.double(), gz.double(), (3,) * d)
        assert float((gw - gw0).abs().max()) <= 1e-11 * float(gw0.abs().max())


def test_consecutive_coupling_blocks_hand_their_parts_over():
    """ModuleList_ runs consecutive coupling blocks over one partition on the parts of the field, without cat / split in between
    (nn/_core.py::_run_chain; protocol of the reference: src/nn/_core.py:64-72 around couplings_.py:54-78): the same numbers
    as block after block, forward and backward -- with one mask object shared by the blocks, with equal masks built
    separately, and NOT across a block over another partition or a non-coupling block."""
    from normflow__amd.nn import DistConvertor_
    torch.manual_seed(21)
    shape = (4, 4, 4, 32)
    lim = dict(xlim=(-5.0, 5.0), ylim=(-5.0, 5.0), extrap={'left': 'linear', 'right': 'linear'})
    mk = lambda c: ConvAct(1, c, 3, conv_dim=4, hidden_sizes=[8, 8], acts=['tanh', 'tanh', None])
    shared = EvenOddMask(shape=shape)
    blocks = [RQSplineCoupling_([mk(46)], mask=shared, **lim), AffineCoupling_([mk(2), mk(2)], mask=shared),
              RQSplineCoupling_([mk(46), mk(46)], mask=EvenOddMask(shape=shape), **lim),            # an equal mask of its own
              DistConvertor_(6, symmetric=True),
              AffineCoupling_([mk(2)], mask=EvenOddMask(shape=shape)), ShiftCoupling_([mk(1)], mask=shared)]
    net_ = ModuleList_(blocks)
    net_.to(device=DEV, dtype=torch.float32)
    x = torch.randn((3,) + shape, device=DEV, dtype=torch.float32)
    calls = []
    orig_split = type(shared).split
    type(shared).split = lambda self, t: (calls.append(1), orig_split(self, t))[1]
    try:
        with torch.no_grad():
            y, lj = net_(x)
            n_chain = len(calls)
            xb, lb = net_.backward(y)
    finally:
        type(shared).split = orig_split
    assert n_chain == 2                          # blocks 0-2 as one run, block 3 apart, blocks 4-5 as one run
    with torch.no_grad():
        y0, l0 = x, 0
        for blk in blocks:
            y0, l0 = blk.forward(y0, l0)
        x0, lb0 = y, 0
        for blk in reversed(blocks):
            x0, lb0 = blk.backward(x0, lb0)
    assert torch.equal(y, y0) and torch.equal(lj, l0)
    assert torch.equal(xb, x0) and torch.equal(lb, lb0)
    assert float((xb - x).abs().median()) < 1e-4       # (and it is the inverse: the fp32 DistConvertor_ in the middle is ill-conditioned in its tails)


def test_posterior_graphed_draws_equal_the_eager_draws():
    """Posterior.graphed: the net pass of posterior.sample__ / mcmc.sample replayed from a HIP graph (one per batch shape) -- the
    same draws as the eager pass for the same seed, before and after the parameters change (the graph re-captures itself)."""
    import normflow__amd as nf
    from normflow__amd.prior import NormalPrior
    from normflow__amd.action import ScalarPhi4Action
    torch.manual_seed(6)
    shape = (16, 16)
    mask = EvenOddMask(shape=shape)
    mk = lambda c: ConvAct(1, c, 3, conv_dim=2, hidden_sizes=[8, 8], acts=['tanh', 'tanh', None])
    net_ = ModuleList_([AffineCoupling_([mk(2), mk(2)], mask=mask), RQSplineCoupling_([mk(22)], mask=mask, xlim=(-5, 5), ylim=(-5, 5),
                                                                                     extrap={'left': 'linear', 'right': 'linear'})])
    net_.to(device=DEV, dtype=torch.float32)
    prior = NormalPrior(loc=torch.zeros(shape, device=DEV, dtype=torch.float32), scale=torch.ones(shape, device=DEV, dtype=torch.float32))
    model = nf.Model(net_=net_, prior=prior, action=ScalarPhi4Action(kappa=0.67, m_sq=-4 * 0.67, lambd=0.5))
    for round_ in range(2):
        out = []
        for graphed in (False, True, True):
            model.posterior.graphed = graphed
            torch.manual_seed(100 + round_)
            out.append(model.posterior.sample__(64))
        for a, b in ((out[0], out[1]), (out[0], out[2])):
            assert all(torch.equal(s, t) for s, t in zip(a, b))
        with torch.no_grad():
            for p in net_.parameters():
                p.mul_(1.01)
    model.posterior.graphed = True
    y = model.mcmc.sample(32)
    assert y.shape == (32,) + shape and bool(torch.isfinite(y).all())


@pytest.mark.parametrize("hidden,m,shape", [(16, 16, (2, 2, 4, 32)), (12, 8, (2, 4, 2, 48)), (9, 16, (4, 2, 2, 64))])
def test_hidden_width_up_to_16_on_the_split_fp16_kernels(hidden, m, shape, parity_report):
    """ConvAct 1 -> h -> h -> 3m-2 with 8 < h <= 16 (the reference leaves the hidden widths free: modules.py:68-154): composed
    from the split-fp16 kernels in groups of 8 channels (_hip.conv_wide_logits_split16) + the coupling kernel.  Against the
    fp64 oracle, forward and inverse, both parities, and against the exact fp32-product path; asserts the composed path ran."""
    torch.manual_seed(31)
    C = 3 * m - 2
    lim = dict(xlim=(-5.0, 5.0), ylim=(-5.0, 5.0), extrap={'left': 'linear', 'right': 'linear'})
    nets = [ConvAct(1, C, 3, conv_dim=4, hidden_sizes=[hidden, hidden], acts=['tanh', 'tanh', None]) for _ in range(2)]
    mask = EvenOddMask(shape=shape)
    cpl = RQSplineCoupling_(nets, mask=mask, **lim).to(DEV, torch.float32)
    with torch.no_grad():
        for net in nets:
            for p_ in list(net.parameters())[-2:]:
                p_.mul_(0.3)
    B = 3
    x = 1.5 * torch.randn((B,) + shape, device=DEV, dtype=torch.float32)
    with torch.no_grad():
        assert nets[0]._wide_plan(x.unsqueeze(1)) is not None
        y, lj = cpl(x)
        xb, lb = cpl.backward(y, lj)
        with _hip.options(split16=False):
            assert nets[0]._wide_plan(x.unsqueeze(1)) is None
            y32, lj32 = cpl(x)
    assert rel(y, y32) <= 1e-5 and rel(lj, lj32) <= 1e-5
    assert rel(xb, x) <= 2e-4 and float(lb.abs().max()) <= 2e-4 * max(1.0, float(lj.abs().max()))
    # the fp64 oracle, atom by atom
    xo = x.double().cpu()
    parts = [xo * O.channel_mask(shape, 0), xo * O.channel_mask(shape, 1)]
    lo = torch.zeros(B, dtype=torch.float64, device='cpu')
    for k, net in enumerate(nets):
        p = k % 2
        convs = [mod for mod in net if hasattr(mod, 'weight')]
        layers = [(c.weight.detach().double().cpu(), c.bias.detach().double().cpu()) for c in convs]
        out = O.conv_act(parts[1 - p].unsqueeze(1), layers, ['tanh', 'tanh', None])
        parts[p], lo = O.rqs_coupling_atom(parts[p], out, O.channel_mask(shape, p), log0=lo, **lim)
    yo = parts[0] + parts[1]
    ey, el = rel(y, yo), rel(lj, lo)
    parity_report(f"hidden width {hidden}, m={m} {shape}", "y / logJ vs fp64 oracle", max(ey, el), 1e-5)
    assert ey <= 1e-5 and el <= 1e-5


def test_hidden_width_16_affine_coupling_on_the_split_fp16_kernels():
    """The same composition under an AffineCoupling_ (net 1 -> 16 -> 16 -> 2: the logits tensor is (B, 2, V/2)): == the exact
    fp32-product path and the fp64 oracle."""
    torch.manual_seed(33)
    shape = (2, 2, 4, 48)
    nets = [ConvAct(1, 2, 3, conv_dim=4, hidden_sizes=[16, 16], acts=['tanh', 'tanh', None]) for _ in range(2)]
    mask = EvenOddMask(shape=shape)
    cpl = AffineCoupling_(nets, mask=mask).to(DEV, torch.float32)
    x = torch.randn((3,) + shape, device=DEV, dtype=torch.float32)
    with torch.no_grad():
        assert nets[0]._wide_plan(x.unsqueeze(1)) is not None
        y, lj = cpl(x)
        xb, lb = cpl.backward(y, lj)
        with _hip.options(split16=False):
            y32, lj32 = cpl(x)
    assert rel(y, y32) <= 1e-5 and rel(lj, lj32) <= 1e-5
    assert rel(xb, x) <= 1e-5 and float(lb.abs().max()) <= 1e-4
    xo = x.double().cpu()
    parts = [xo * O.channel_mask(shape, 0), xo * O.channel_mask(shape, 1)]
    lo = torch.zeros(3, dtype=torch.float64, device='cpu')
    for k, net in enumerate(nets):
        p = k % 2
        convs = [mod for mod in net if hasattr(mod, 'weight')]
        layers = [(c.weight.detach().double().cpu(), c.bias.detach().double().cpu()) for c in convs]
        out = O.conv_act(parts[1 - p].unsqueeze(1), layers, ['tanh', 'tanh', None])
        parts[p], lo = O.affine_coupling_atom(parts[p], out, O.channel_mask(shape, p), log0=lo)
    assert rel(y, parts[0] + parts[1]) <= 1e-5 and rel(lj, lo) <= 1e-5

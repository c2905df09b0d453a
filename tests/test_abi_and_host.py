"""CPU-side checks (no GPU): the C-ABI library loads and exports every symbol that
include/normflow_hip.h declares; argument validation works without launching anything;
the product path refuses CPU tensors; host-side logic (masks, state_dict keys, knots,
Fitter, stats) behaves like the reference."""
import ctypes
import os
import re

import math
import numpy as np
import pytest
import torch

import normflow__amd as nf
from normflow__amd import _hip
from normflow__amd.mask import EvenOddMask, AlongAxesEvenOddMask
from normflow__amd.nn import (ConvAct, RQSplineCoupling_, AffineCoupling_, DistConvertor_, ModuleList_,
                              Module_, Conv4d)
from normflow__amd.nn.scalar.convNd import circular_conv
from oracle import nf_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device('cpu')


def test_library_exports_every_declared_symbol():
    header = open(os.path.join(ROOT, "include", "normflow_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(nf_[a-z0-9_]+)\s*\(", header))
    assert {"nf_rqs_fwd", "nf_rqs_inv", "nf_rqs_fwd_vjp", "nf_rqs_inv_vjp", "nf_affine_fwd", "nf_affine_inv",
            "nf_affine_vjp", "nf_distconv", "nf_distconv_vjp", "nf_version", "nf_last_error_string",
            "nf_workspace_bytes", "nf_normal_sample", "nf_normal_sample_rows"} <= declared
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in the header but not exported"
    assert set(_hip.PROTOTYPES) == declared
    assert _hip.load().nf_version() == 301


def test_argument_validation_without_gpu():
    lib = _hip.load()
    opts = _hip.make_rqs_opts(1, (0, 1), (0, 1), {}, 0)       # m < 2
    rc = lib.nf_rqs_fwd(None, None, None, None, None, None, 1, 4, ctypes.byref(opts), None, None, 0, 0, None)
    assert rc == -1 and b"mask" in lib.nf_last_error_string() or b"knots_len" in lib.nf_last_error_string()
    rc = lib.nf_affine_fwd(None, None, None, None, None, None, 1, 4, 3, 0, None, 0, 0, None)
    assert rc == -1
    assert lib.nf_workspace_bytes(4, 1024) > 0
    with pytest.raises(NotImplementedError):
        _hip.make_rqs_opts(4, (0, 1), (0, 1), {'left': 'periodic'}, 0)


def test_tiling_plan_queries():
    """nf_plan_tiling / nf_rqs_plan_block: pure host planning, the launchers' own make_tiling and pick_block.  A literal
    table (iters doubles while (units // (2 block iters)) B >= 8192, blocks_x = ceil(units / (block iters))) and the
    argument validation."""
    lib = _hip.load()
    err = lambda: lib.nf_last_error_string().decode()

    def plan(units, B, block=256):
        it, bx = ctypes.c_int(-7), ctypes.c_int64(-7)
        assert lib.nf_plan_tiling(units, B, block, ctypes.byref(it), ctypes.byref(bx)) == 0
        return it.value, bx.value

    table = {(256, 5): (1, 1), (2310, 3): (1, 10), (1155, 4096): (2, 3), (1155, 8192): (4, 2), (2310, 8192): (8, 2),
             (4096, 1024): (2, 8),                     # 16^3 at batch 1024: BASELINE config 3
             (524288, 8): (2, 1024),                   # 32^4 in the pair layout at batch 8: config 4's slab
             (1155, 4096, 64): (8, 3), (1155, 4096, 128): (4, 3), (1155, 3, 64): (1, 19),
             (2 ** 22 + 3, 1): (2, 8193), (2 ** 22 - 1, 1): (1, 16384), (0, 4): (1, 0), (7, 0): (1, 1)}
    for args, want in table.items():
        assert plan(*args) == want, (args, plan(*args), want)
    it, bx = ctypes.c_int(0), ctypes.c_int64(0)
    assert lib.nf_plan_tiling(10, 1, 256, None, ctypes.byref(bx)) == -1 and "NULL" in err()
    assert lib.nf_plan_tiling(10, 1, 256, ctypes.byref(it), None) == -1 and "NULL" in err()
    assert lib.nf_plan_tiling(-1, 1, 256, ctypes.byref(it), ctypes.byref(bx)) == -1 and "negative" in err()
    assert lib.nf_plan_tiling(10, -1, 256, ctypes.byref(it), ctypes.byref(bx)) == -1 and "negative" in err()
    for block in (0, 32, 100, 512, -64):
        assert lib.nf_plan_tiling(10, 1, block, ctypes.byref(it), ctypes.byref(bx)) == -1 and "workgroup size" in err()

    lin = {'left': 'linear', 'right': 'linear'}
    def block_of(m, dtype, layout=0, **kw):
        return lib.nf_rqs_plan_block(ctypes.byref(_hip.make_rqs_opts(m, (-5, 5), (-5, 5), lin, layout, **kw)), dtype)
    F32, F64, F16 = _hip.NF_F32, _hip.NF_F64, _hip.NF_F16
    table = {(4, F32): 256, (8, F64): 256, (16, F32): 256, (16, F16): 256,       # register kernels
             (3, F32): 256, (3, F64): 256, (10, F64): 256,                        # LDS columns that fit 64 KiB at 256 lanes
             (24, F32): 128, (24, F64): 64, (24, F32, 1): 128, (48, F32): 64,     # shrunk workgroups
             (200, F64): 0, (5, F16): 0}                                          # does not fit / no fp16 kernel
    for args, want in table.items():
        assert block_of(*args) == want, (args, block_of(*args), want)
    assert "fp16 storage" in err()
    assert block_of(200, F64) == 0 and "does not fit" in err()
    kx = torch.linspace(-5, 5, 4)
    assert block_of(4, F32, knots_x=kx) == 256        # fixed knots: the LDS-column kernel, C = 2m - 1 = 7 logits per lane
    assert lib.nf_rqs_plan_block(None, F32) == 0 and "opts is NULL" in err()
    assert block_of(1, F32) == 0 and "knots_len" in err()
    assert block_of(4, 9) == 0 and "dtype" in err()
    assert lib.nf_version() == 301


def test_kernel_selection_options_in_process():
    """nf_set_option / nf_get_option: the in-process switch between the split-fp16 and the exact-fp32-product kernels (what
    bench.py's second value and the headline parity tests use; the library reads no environment variable)."""
    lib = _hip.load()
    assert lib.nf_get_option(_hip.OPT_SPLIT16) == 1 and lib.nf_get_option(_hip.OPT_PIPE) == 1
    lat = (ctypes.c_int32 * 4)(4, 4, 4, 32)
    k3 = (ctypes.c_int32 * 4)(3, 3, 3, 3)
    assert lib.nf_conv_split16_supported(lat, k3, 8, 8, 1) == 1
    assert lib.nf_conv_weight_layout(lat, k3, 8, 46, 1, 3, _hip.NF_F32) == 2         # NF_WLAYOUT_SPLIT16
    with _hip.options(split16=False):
        assert lib.nf_get_option(_hip.OPT_SPLIT16) == 0
        assert lib.nf_conv_split16_supported(lat, k3, 8, 8, 1) == 0
        assert lib.nf_conv_weight_layout(lat, k3, 8, 46, 1, 3, _hip.NF_F32) == 1     # row-packed fp32 kernel
        with _hip.options(pipe=False):
            assert lib.nf_conv_weight_layout(lat, k3, 8, 46, 1, 3, _hip.NF_F32) == 0
    assert lib.nf_get_option(_hip.OPT_SPLIT16) == 1 and lib.nf_get_option(_hip.OPT_PIPE) == 1
    assert lib.nf_set_option(99, 1) == -1 and b"unknown option" in lib.nf_last_error_string()


def test_product_library_reads_no_environment():
    """Timing ablations that skip work (NF_CONV_DBG, NF_CONVG_DBG, NF_H_ABL), clock stamps and planner knobs exist only in
    `make DIAG=1` builds: the shipped library has no getenv import at all."""
    import subprocess
    out = subprocess.run(["nm", "-D", "--undefined-only", _hip.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "getenv" not in out


def test_bench_multi_gpu_launch_contract():
    """bench.py --gpus N: (1) without a launcher it starts the ranks itself -- and refuses, before touching any GPU, when
    the box has fewer devices; (2) under a launcher whose WORLD_SIZE differs from --gpus it exits non-zero instead of
    printing a number for the wrong world."""
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "NF_BENCH_REHEARSAL")}
    if torch.cuda.device_count() < 2:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], env=env, capture_output=True, text=True)
        assert r.returncode == 2 and "only" in r.stderr and r.stdout.strip() == ""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4"],
                       env=dict(env, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0"), capture_output=True, text=True)
    assert r.returncode == 2 and "WORLD_SIZE=2" in r.stderr and r.stdout.strip() == ""


def test_product_path_refuses_cpu_tensors():
    mask = EvenOddMask(shape=(4, 4))
    net = ConvAct(1, 2, 3, conv_dim=2).to(CPU)
    cpl = AffineCoupling_([net], mask=mask).to(CPU)
    with pytest.raises(_hip.NormflowHipError, match="no CPU fallback"):
        cpl(torch.randn(2, 4, 4, device=CPU))
    with pytest.raises(_hip.NormflowHipError):
        DistConvertor_(4).to(CPU)(torch.randn(3, 1, device=CPU))


def test_masks_match_golden_and_pairing(golden):
    z = golden("callers")
    for key in [k for k in z.files if k.startswith("mask/")]:
        _, shp, p = key.split("/")
        shape = tuple(int(s) for s in shp.split("x"))
        m = EvenOddMask(shape=shape, parity=int(p[1:]))
        assert np.array_equal(m._mask.cpu().numpy(), z[key])
        assert np.array_equal(m._c_mask.cpu().numpy(), 1 - z[key])
        assert m.pairable == (shape[-1] % 2 == 0)
    assert list(EvenOddMask(shape=(4, 4)).state_dict()) == ['_mask', '_c_mask']
    a = AlongAxesEvenOddMask(shape=(3, 4), mu=1)
    assert a._mask[:, 0].tolist() == [1, 1, 1] and a._mask[0].tolist() == [1, 0, 1, 0]


def test_state_dict_keys_match_reference(golden):
    z = golden("blocks")
    for d in (1, 2, 3, 4):
        nets = [ConvAct(1, 16, 3, conv_dim=d, hidden_sizes=[4, 4], acts=['tanh', 'tanh', None]) for _ in range(3)]
        cpl = RQSplineCoupling_(nets, mask=EvenOddMask(shape=(4,) * d))
        ours = {k for k in cpl.state_dict() if k.startswith("nets.")}
        ref = {k.split("/param/")[1] for k in z.files if k.startswith(f"rqs/d{d}/param/")}
        assert ours == ref
        for k, v in cpl.state_dict().items():
            if k.startswith("nets."):
                assert tuple(v.shape) == z[f"rqs/d{d}/param/{k}"].shape


@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_circular_conv_host_matches_oracle(d):
    g = torch.Generator(device='cpu').manual_seed(d)
    x = torch.randn((2, 3) + (4,) * d, generator=g, device=CPU, dtype=torch.float64)
    w = torch.randn((5, 3) + (3,) * d, generator=g, device=CPU, dtype=torch.float64)
    b = torch.randn(5, generator=g, device=CPU, dtype=torch.float64)
    assert (circular_conv(x, w, b) - O.circular_conv_direct(x, w, b)).abs().max() < 1e-12
    if d == 4:
        c = Conv4d(3, 5, 3).to(CPU)
        assert c._conv_lower_dim.weight.shape == (15, 3, 3, 3, 3)
        ref = O.circular_conv_direct(x, O.conv4d_standard_weight(c._conv_lower_dim.weight.detach(), 5, 3), c.bias.detach())
        assert (c(x) - ref).abs().max() < 1e-12


def test_shared_spline_knots_match_oracle():
    for sym in (False, True):
        for smooth in (False, True):
            dc = DistConvertor_(7, symmetric=sym, smooth=smooth).to(CPU)
            sp = dc.spline_layer_
            g = torch.Generator(device='cpu').manual_seed(3)
            with torch.no_grad():
                sp.weights_x.copy_(torch.randn(6, generator=g, device=CPU))
                sp.weights_y.copy_(torch.randn(6, generator=g, device=CPU))
                if not smooth:
                    sp.weights_d.copy_(torch.randn(7, generator=g, device=CPU))
            lim = (0.5, 1) if sym else (0, 1)
            ref = O.shared_spline_knots(sp.weights_x.detach(), sp.weights_y.detach(),
                                        None if smooth else sp.weights_d.detach(), lim, lim,
                                        {'left': 'anti'} if sym else {})
            ours = sp.knots().detach()
            assert ours.shape == (3, 13 if sym else 7)
            for a, b in zip(ours, ref):
                assert (a - b).abs().max() < 1e-14
    assert list(DistConvertor_(10, symmetric=True).state_dict()) == ['1.weights_x', '1.weights_y', '1.weights_d']


class _OracleDistConv(Module_):
    """TEST-ONLY stand-in for a flow block, evaluated by the CPU oracle, so that the
    host logic (Fitter, Posterior, MCMC, DP) can be exercised without a GPU."""

    def __init__(self, m=6):
        super().__init__(label='oracle_dc')
        self.wx = torch.nn.Parameter(torch.zeros(m - 1, device=CPU))
        self.wy = torch.nn.Parameter(torch.zeros(m - 1, device=CPU))
        self.wd = torch.nn.Parameter(torch.zeros(m, device=CPU))

    def forward(self, x, log0=0):
        return O.dist_convertor(x, self.wx, self.wy, self.wd, symmetric=True, log0=log0)

    def backward(self, x, log0=0):
        return O.dist_convertor(x, self.wx, self.wy, self.wd, symmetric=True, inverse=True, log0=log0)


def make_cpu_model(seed=0):
    from normflow__amd.prior import NormalPrior
    from normflow__amd.action import ScalarPhi4Action
    torch.manual_seed(seed)
    prior = NormalPrior(loc=torch.zeros(1, device=CPU), scale=torch.ones(1, device=CPU))
    action = ScalarPhi4Action(kappa=0, m_sq=-1.2, lambd=0.5)
    return nf.Model(net_=ModuleList_([_OracleDistConv()]), prior=prior, action=action)


def test_fitter_posterior_mcmc_host_logic(capsys):
    model = make_cpu_model()
    model.fit(n_epochs=60, batch_size=256, hyperparam=dict(lr=0.02, weight_decay=0.0),
              checkpoint_dict=dict(print_stride=30, print_batch_size=512))
    out = capsys.readouterr().out
    assert "Epoch: 30 | loss:" in out and "accept_rate" in out
    h = model.fit.train_history
    assert len(h['loss']) == 60 and h['loss'][-1] < h['loss'][0] - 0.3
    # analytic log Z of the README model = 1.112773; a short fit gets close
    assert abs(h['logz'][-1][0] - 1.112773) < 0.08
    y = model.posterior.sample(17)
    assert y.shape == (17, 1)
    y, logq, logp = model.posterior.sample__(64)
    assert torch.allclose(model.posterior.log_prob(y), logq, atol=1e-9)
    ys, lq, lp = model.mcmc.sample__(64)
    assert ys.shape == (64, 1) and 0.0 < model.mcmc.history.accept_rate[-1] <= 1.0
    (x, yy, xh), (lj, l0) = nf.backward_sanitychecker(model, return_details=True)
    assert (x - xh).abs().sum() < 1e-9 and l0.abs().sum() < 1e-9


def test_c1_caller_tuple_matches_golden(golden):
    """Posterior/Fitter arithmetic (logq = logr - logJ, loss = mean(logq - logp)) on the
    golden README-model tuple, with prior/action of this package."""
    from normflow__amd.prior import NormalPrior
    from normflow__amd.action import ScalarPhi4Action
    from normflow__amd._normflowcore import Fitter
    z = golden("callers")
    x = torch.from_numpy(z["c1/x"])
    prior = NormalPrior(loc=torch.zeros(1, device=CPU), scale=torch.ones(1, device=CPU))
    action = ScalarPhi4Action(kappa=0, m_sq=-1.2, lambd=0.5)
    logr = prior.log_prob(x)
    assert (logr - torch.from_numpy(z["c1/logr"])).abs().max() < 1e-13
    logq = logr - torch.from_numpy(z["c1/logJ"])
    logp = -action(torch.from_numpy(z["c1/y"]))
    assert (logp - torch.from_numpy(z["c1/logp"])).abs().max() < 1e-13
    assert abs(Fitter.calc_kl_mean(logq, logp).item() - float(z["c1/loss"])) < 1e-13
    kap, msq, lam = (float(v) for v in z["phi4/coef"])
    act = ScalarPhi4Action(kappa=kap, m_sq=msq, lambd=lam)
    for d in (1, 2, 3, 4):
        cfg = torch.from_numpy(z[f"phi4/d{d}/cfg"])
        assert (act(cfg) - torch.from_numpy(z[f"phi4/d{d}/S"])).abs().max() < 1e-11
        shape = cfg.shape[1:]
        pr = NormalPrior(loc=torch.zeros(shape, device=CPU), scale=torch.ones(shape, device=CPU))
        assert (pr.log_prob(cfg) - torch.from_numpy(z[f"phi4/d{d}/logr"])).abs().max() < 1e-11


def test_stats_helpers():
    from normflow__amd.lib import fmt_val_err, estimate_logz, Resampler
    assert fmt_val_err(1.112445, 0.000022, err_digits=2) == "1.112445(22)"
    assert fmt_val_err(0.988, 0.003) == "0.988(3)"
    t = torch.linspace(-1, 1, 50, device=CPU)
    mean, std = estimate_logz(t, method='jackknife')
    assert abs(mean - (torch.logsumexp(-t, 0).item() - np.log(50))) < 1e-12 and std > 0
    assert len(list(Resampler('jackknife')(t))) == 50


def test_spectral_block_host_side(golden):
    """k^2 grid, parameter/buffer names and the free-theory initialisation of the spectral block
    (PSDBlock_/FFTNet_/MeanFieldNet_) against the reference's values -- the parts that need no kernel."""
    from normflow__amd.nn import FFTNet_, MeanFieldNet_, PSDBlock_, lattice_k2
    z = golden("psd")
    for tag, shape, mfdict, fftdict in (
            ("psd2d", (8, 8), dict(knots_len=6, symmetric=True, final_scale=True, smooth=True), dict(knots_len=5, ignore_zeromode=True)),
            ("psd3d", (4, 6, 4), dict(knots_len=4, symmetric=False, smooth=False), dict(knots_len=4, ignore_zeromode=False)),
            ("psd1d_odd", (9,), dict(knots_len=5, symmetric=True, smooth=True),
             dict(knots_len=1, ignore_zeromode=True, eff_mass2=0.7, eff_kappa=1.3, a=0.5))):
        k2 = lattice_k2(shape, dtype=torch.float64, device=CPU)
        assert np.allclose((k2 / k2.max()).numpy(), z[tag + "/k2norm"], atol=1e-14)
        assert abs(float(k2.max()) - float(z[tag + "/k2max"])) < 1e-12
        with torch.device(CPU):
            blk = PSDBlock_(mfnet_=MeanFieldNet_.build(**mfdict), fftnet_=FFTNet_.build(shape, **fftdict))
        keys = [k[len(tag) + 7:] for k in z.files if k.startswith(tag + "/state/")]
        assert list(blk.state_dict().keys()) == keys
        for k in keys:
            assert tuple(blk.state_dict()[k].shape) == z[f"{tag}/state/{k}"].shape
    # free-theory start: logy = (log m^2 + d log a, log(kappa k2max) + (d - 2) log a)
    with torch.device(CPU):
        f = FFTNet_.build((9,), knots_len=1, eff_mass2=0.7, eff_kappa=1.3, a=0.5)
    k2max = float(lattice_k2((9,), dtype=torch.float64).max())
    want = [math.log(0.7) + math.log(0.5), math.log(1.3 * k2max) - math.log(0.5)]
    assert np.allclose(f.ipsd_net.logy.detach().double().numpy(), want, atol=1e-6)
    assert f.ipsd_net.knots_len == 2 and f.ipsd_net.smooth


def test_conv_weight_layout_planning_and_packers():
    """nf_conv_weight_layout is pure planning (no GPU): which layers get the persistent kernel's row-packed
    weights, and that the host packers produce that layout -- checked element by element against the
    definition in include/normflow_hip.h."""
    import ctypes as C
    lib = _hip.load()

    def layout(lat, ks, cin, cout, compact, fused, dtype=0):
        d = len(lat)
        lat4 = (C.c_int32 * 4)(*([1] * (4 - d) + list(lat)))
        k4 = (C.c_int32 * 4)(*([1] * (4 - d) + list(ks)))
        return lib.nf_conv_weight_layout(lat4, k4, cin, cout, int(compact), int(fused), dtype), lat4, k4

    assert layout((32,) * 4, (3,) * 4, 8, 46, True, True)[0] == 1          # fused last layer of the bench
    assert layout((32,) * 4, (3,) * 4, 8, 8, False, False)[0] == 1         # 8 -> 8 layer
    assert layout((32,) * 4, (3,) * 4, 1, 8, False, False)[0] == 0         # first layer: K-packed fragments
    assert layout((32,) * 4, (3,) * 4, 8, 46, True, False, dtype=1)[0] == 0  # fp64: one-box kernel
    assert layout((32,) * 4, (3, 3, 3, 5), 8, 8, False, False)[0] == 0     # k3 != 3
    assert layout((32,) * 4, (3,) * 4, 6, 8, False, False)[0] == 0         # cin % 4 != 0
    assert layout((48,) * 4, (3,) * 4, 8, 46, True, True)[0] == 1          # not a power of two: still the persistent kernel
    assert lib.nf_conv_weight_layout(None, None, 8, 8, 0, 0, 0) == -1

    torch.manual_seed(0)
    for cout, compact, fused in ((46, True, True), (8, False, False), (20, True, False)):
        cin, ks, lat = 8, (3, 3, 3, 3), (8, 8, 8, 16)
        w = torch.randn((cout, cin) + ks, dtype=torch.float32, device=CPU)
        code, lat4, k4 = layout(lat, ks, cin, cout, compact, fused)
        assert code == 1
        if lib.nf_conv_two_site(cout, int(compact), lat[-1], ks[-1]) and not fused:
            w2 = w.new_zeros((16, cin) + ks[:-1] + (ks[-1] + 1,))
            w2[:cout, ..., :ks[-1]] = w
            w2[8:8 + cout, ..., 1:] = w
            w = w2
        p = _hip.conv_weight_for_layer(w, lat4, k4, cin, cout, compact, fused, 0)
        k3, nt = w.shape[-1], (w.shape[0] + 15) // 16
        rows = 27
        assert tuple(p.shape) == (rows, cin // 4, 64, (k3 * nt + 3) // 4 * 4)
        wf = w.reshape(w.shape[0], cin, rows, k3)
        g = torch.Generator().manual_seed(1)
        for _ in range(400):
            row, kq, lane, j3, t = (int(torch.randint(0, n, (1,), generator=g)) for n in (rows, cin // 4, 64, k3, nt))
            col, ci = t * 16 + (lane & 15), kq * 4 + (lane >> 4)
            want = float(wf[col, ci, row, j3]) if col < w.shape[0] else 0.0
            assert float(p[row, kq, lane, j3 * nt + t]) == want
        assert float(p[..., k3 * nt:].abs().sum()) == 0.0


def test_rqspline_explicit_knots_host_side():
    """`RQSpline(knots_x=, knots_y=, knots_d=, knots_axis=, extrap=)` (spline.py:39-68): the stored knots after the
    boundary augmentation (spline.py:458-532), the knots_d=None smoothing (:125-152), the 'anti-periodic' alias and the
    reference's shape errors -- host logic, no kernel call (evaluation needs the GPU: tests/test_gpu_parity.py)."""
    from normflow__amd.lib.spline import RQSpline
    torch.manual_seed(3)
    with torch.device("cpu"):
        out = 0.7 * torch.randn(2, 13, 4, 3, dtype=torch.float64)
        kx, ky, kd = O.knots_from_logits(out, (-1.0, 2.0), (0.0, 3.0))
        for extrap in ({}, {'left': 'linear', 'right': 'linear'}, {'left': 'anti', 'right': 'linear'}, {'right': 'anti-periodic'}):
            want = O.augment_knots(kx, ky, kd, axis=1, **extrap)
            sp = RQSpline(knots_x=kx, knots_y=ky, knots_d=kd, knots_axis=1, extrap=extrap)
            sl = RQSpline(knots_x=kx.movedim(1, -1), knots_y=ky.movedim(1, -1), knots_d=kd.movedim(1, -1), extrap=extrap)
            assert sp.knots_len == want[0].shape[1] == sl.knots_len and sp.segm_len == sp.knots_len - 1
            assert tuple(sp.knots_shape) == tuple(want[0].shape)
            for got, got_last, w in zip((sp.knots_x, sp.knots_y, sp.knots_d), (sl.knots_x, sl.knots_y, sl.knots_d), want):
                assert torch.equal(got, w) and torch.equal(got_last.movedim(-1, 1), w)
        # 1-D knots_x against N-D knots_y with a boundary rule: every tensor gets the full shape first
        kx1 = torch.linspace(-1.0, 2.0, 5, dtype=torch.float64)
        sp = RQSpline(knots_x=kx1, knots_y=ky, knots_d=kd, knots_axis=1, extrap={'left': 'linear'})
        want = O.augment_knots(kx1, ky, kd, axis=1, left='linear')
        assert torch.equal(sp.knots_x, want[0]) and torch.equal(sp.knots_y, want[1])
        # knots_d = None
        sp = RQSpline(knots_x=kx1, knots_y=ky[0, :, 0, 0].contiguous(), knots_d=None)
        y1 = ky[0, :, 0, 0]
        s = (y1[1:] - y1[:-1]) / (kx1[1:] - kx1[:-1])
        assert torch.allclose(sp.knots_d, torch.cat((s[:1], 0.5 * (s[1:] + s[:-1]), s[-1:])), rtol=0, atol=1e-15)
        with pytest.raises(Exception, match="same shape"):
            RQSpline(knots_x=kx, knots_y=ky[:, :, :2], knots_d=kd)
        with pytest.raises(Exception, match="not supported"):
            RQSpline(knots_x=kx, knots_y=ky, knots_d=kd, knots_axis=1, extrap={'left': 'periodic'})
        # and without a device there is no evaluation: the product has no CPU path
        with pytest.raises(_hip.NormflowHipError):
            RQSpline(knots_x=kx, knots_y=ky, knots_d=kd, knots_axis=1)(torch.zeros(2, 1, 4, 3, dtype=torch.float64))


def test_coupling_slab_budgets_are_module_settings():
    """The planner knobs are module attributes with a setter -- the product reads no environment variable for them."""
    from normflow__amd.nn.scalar import couplings_
    old = couplings_.set_slab_bytes(hidden=1 << 20)
    try:
        assert couplings_.HIDDEN_SLAB_BYTES == 1 << 20 and couplings_.PARAM_SLAB_BYTES == old[0]
    finally:
        couplings_.set_slab_bytes(*old)
    assert (couplings_.PARAM_SLAB_BYTES, couplings_.HIDDEN_SLAB_BYTES) == old
    src = open(couplings_.__file__).read()
    assert "os.environ" not in src and "getenv" not in src


def test_round3_entry_points_validate_their_arguments_without_gpu():
    """The entry points added in round 3 refuse bad arguments with a status code and a message before any launch (no GPU
    needed): nf_spline_eval, nf_small_lattice_coupling(+_supported), nf_conv_rqs_split16_supported, the training node's two calls."""
    lib = _hip.load()
    err = lambda: lib.nf_last_error_string().decode()
    assert lib.nf_spline_eval(None, None, None, None, None, None, 1, 8, 1, 0, 0, 0, 0, 0, None) == -1 and "2 knots" in err()
    assert lib.nf_spline_eval(None, None, None, None, None, None, 1, 8, 4, 0, 0, 0, 0, 7, None) == -1 and "dtype" in err()
    assert lib.nf_spline_eval(None, None, None, None, None, None, 0, 8, 4, 0, 0, 0, 0, 0, None) == 0          # empty batch: nothing to do
    assert lib.nf_spline_eval(None, None, None, None, None, None, 1, 8, 4, 0, 0, 0, 0, 0, None) == -1 and "NULL" in err()
    lat3 = lambda *l: (ctypes.c_int32 * 3)(*l)
    T, S = _hip.ACT_CODES['tanh'], _hip.ACT_CODES['expit']
    assert lib.nf_small_lattice_supported(lat3(16, 16, 16), 3, 0, 46, 16, T, T) == 1
    assert lib.nf_small_lattice_supported(lat3(4, 6, 16), 3, 0, 22, 8, T, S) == 1
    assert lib.nf_small_lattice_supported(lat3(16, 16, 32), 3, 0, 46, 16, T, T) == 0        # fastest axis must be 16
    assert lib.nf_small_lattice_supported(lat3(16, 5, 16), 3, 0, 46, 16, T, T) == 0         # odd middle extent
    assert lib.nf_small_lattice_supported(lat3(16, 16, 16), 3, 0, 46, 15, T, T) == 0        # cout != 3m - 2
    assert lib.nf_small_lattice_supported(lat3(16, 16, 16), 3, 0, 46, 16, T, 2) == 0         # relu outputs are not fp16-safe
    assert lib.nf_small_lattice_supported(lat3(64, 16, 16), 3, 0, 46, 16, T, T) == 0        # does not fit the LDS
    opts = _hip.make_rqs_opts(16, (-5, 5), (-5, 5), {}, _hip.LAYOUT_PAIR)
    rc = lib.nf_small_lattice_coupling(0, None, None, None, None, None, None, None, None, None, None, None, 2, lat3(16, 16, 32), 3, 0, 46,
                                       T, T, ctypes.byref(opts), 0, None)
    assert rc == -1 and "needs a lattice" in err()
    rc = lib.nf_small_lattice_coupling(0, None, None, None, None, None, None, None, None, None, None, None, 0, lat3(16, 16, 16), 3, 0, 46,
                                       T, T, ctypes.byref(opts), 0, None)
    assert rc == 0
    lat2 = lambda *l: (ctypes.c_int32 * 2)(*l)
    assert lib.nf_small_lattice_supported(lat2(16, 16), 2, 1, 2, 0, T, T) == 1           # config 2: 16 x 16, affine
    assert lib.nf_small_lattice_supported(lat2(16, 16), 2, 0, 22, 8, T, T) == 1          # 2-D spline
    assert lib.nf_small_lattice_supported(lat3(8, 8, 16), 3, 1, 2, 0, T, S) == 1         # 3-D affine
    assert lib.nf_small_lattice_supported(lat2(16, 16), 2, 1, 3, 0, T, T) == 0           # affine nets end in (t, s)
    assert lib.nf_small_lattice_supported(lat2(16, 32), 2, 1, 2, 0, T, T) == 0
    rc = lib.nf_small_lattice_coupling(1, None, None, None, None, None, None, None, None, None, None, None, 3, lat2(16, 16), 2, 0, 2,
                                       T, T, None, 0, None)
    assert rc == -1 and "NULL tensor" in err()
    lat4 = lambda *l: (ctypes.c_int32 * 4)(*l)
    assert lib.nf_conv_rqs_split16_supported(lat4(4, 4, 4, 32), 28, 10) == 1
    assert lib.nf_conv_rqs_split16_supported(lat4(4, 4, 4, 48), 46, 16) == 1
    assert lib.nf_conv_rqs_split16_supported(lat4(4, 4, 4, 16), 46, 16) == 0
    assert lib.nf_conv_rqs_split16_supported(lat4(4, 3, 4, 32), 46, 16) == 0
    assert lib.nf_conv_rqs_split16_supported(lat4(4, 4, 4, 32), 49, 17) == 0
    rc = lib.nf_conv_rqs_split16_train(None, 0, None, None, 46, None, None, None, None, 1, lat4(4, 4, 4, 32), 0, None,
                                       ctypes.byref(opts), 0, None, 0, None)
    assert rc == -1 and "NULL" in err()
    rc = lib.nf_conv_rqs_split16_vjp(None, 0, None, None, 46, None, None, None, None, None, 1, lat4(4, 4, 4, 32), 0, None,
                                     ctypes.byref(opts), 0, None)
    assert rc == -1 and "NULL" in err()


def test_small3d_weight_packers_match_the_documented_fragments():
    """pack_small3d_weights against the fragment layouts include/normflow_hip.h documents for nf_small_lattice_coupling (hi + lo
    reassembled): lane 16 g + row, element i of every fragment."""
    torch.manual_seed(0)
    w1, w2, w3 = torch.randn(8, 1, 3, 3, 3), torch.randn(8, 8, 3, 3, 3), torch.randn(40, 8, 3, 3, 3)
    p1, p2, p3 = _hip.pack_small3d_weights(w1, w2, w3)
    S = _hip.SPLIT16_WEIGHT_SCALE
    r1 = (p1[0].double() + p1[1].double()) / S
    r2 = (p2[:, 0].double() + p2[:, 1].double()) / S
    r3 = (p3[:, :, 0].double() + p3[:, :, 1].double()) / S
    want1 = torch.zeros(64, 8, dtype=torch.float64)
    want2 = torch.zeros(9, 64, 8, dtype=torch.float64)
    want3 = torch.zeros(3, 7, 64, 8, dtype=torch.float64)
    for g in range(4):
        for n in range(16):
            lane = 16 * g + n
            for i in range(8):
                k = 8 * g + i
                if n < 8 and k < 27:
                    want1[lane, i] = w1.reshape(8, 27)[n, k]
            s_, co = n // 8, n % 8
            if 0 <= g - s_ <= 2:
                want2[:, lane, :] = w2[co, :, :, :, g - s_].permute(1, 2, 0).reshape(9, 8)
            for t in range(3):
                for i in range(7):
                    k, ch = 4 * i + g, 16 * t + n
                    if k < 27 and ch < 40:
                        want3[t, i, lane] = w3.reshape(40, 8, 27)[ch, :, k]
    for got, want in ((r1, want1), (r2, want2), (r3, want3)):
        assert float((got - want).abs().max()) <= 2e-7 * max(1.0, float(want.abs().max()))      # hi + lo carries 22 bits


def test_training_entry_points_of_the_small_lattices_validate_without_gpu():
    """nf_conv_wgrad_sites (+ _supported, _workspace) and nf_gather_pad: which layers they take, and that bad arguments come
    back as a status code with a message before any launch."""
    lib = _hip.load()
    err = lambda: lib.nf_last_error_string().decode()
    i4 = lambda *l: (ctypes.c_int32 * 4)(*l)
    F32, F64 = _hip.NF_F32, _hip.NF_F64
    assert lib.nf_conv_wgrad_sites_supported(i4(1, 16, 16, 16), i4(1, 3, 3, 3), 8, 46, F32) == 1       # config 3's last layer
    assert lib.nf_conv_wgrad_sites_supported(i4(1, 1, 16, 16), i4(1, 1, 3, 3), 8, 2, F64) == 1         # config 2, fp64
    assert lib.nf_conv_wgrad_sites_supported(i4(1, 1, 1, 10), i4(1, 1, 1, 3), 3, 5, F32) == 1
    assert lib.nf_conv_wgrad_sites_supported(i4(4, 4, 4, 32), i4(3, 3, 3, 3), 1, 8, F32) == 1          # 81 + 1 columns
    assert lib.nf_conv_wgrad_sites_supported(i4(4, 4, 4, 32), i4(3, 3, 3, 3), 8, 8, F32) == 0          # 649 columns: nf_conv_wgrad(_split16)
    assert lib.nf_conv_wgrad_sites_supported(i4(1, 16, 16, 16), i4(1, 3, 3, 3), 8, 46, F64) == 0       # fp64: 3 x 14 tiles do not fit
    assert lib.nf_conv_wgrad_sites_supported(i4(1, 16, 16, 16), i4(1, 3, 3, 3), 8, 49, F32) == 0
    assert lib.nf_conv_wgrad_sites_supported(i4(1, 16, 16, 16), i4(1, 3, 2, 3), 8, 8, F32) == 0        # even kernel extent
    need = lib.nf_conv_wgrad_sites_workspace(i4(1, 3, 3, 3), 8, 46, F32)
    assert need == 512 * 48 * 224 * 4
    rc = lib.nf_conv_wgrad_sites(None, None, None, 1, i4(1, 16, 16, 16), i4(1, 3, 3, 3), 8, 46, -1, None, 0, F32, None)
    assert rc == -1 and "NULL" in err()
    rc = lib.nf_conv_wgrad_sites(None, None, None, 1, i4(4, 4, 4, 32), i4(3, 3, 3, 3), 8, 8, -1, None, 0, F32, None)
    assert rc == -1 and "not supported" in err()
    assert lib.nf_gather_pad(None, None, None, 4, 4, 4, None) == -1 and "bad arguments" in err()
    one = (ctypes.c_int32 * 1)(0)
    assert lib.nf_gather_pad(one, one, one, 1, 1, 3, None) == -1 and "2, 4 or 8 bytes" in err()
    assert lib.nf_gather_pad(one, one, one, 0, 1, 4, None) == 0


def test_graphed_train_step_refuses_cpu_models():
    """GraphedTrainStep is a HIP-graph facility: a CPU model is refused with a message, Fitter.graphed is off by default and
    ignored for CPU tensors (the eager step runs)."""
    import normflow__amd as nf
    from normflow__amd.prior import NormalPrior
    from normflow__amd.action import ScalarPhi4Action
    from normflow__amd.nn import DistConvertor_, ModuleList_
    from normflow__amd.fitter import kl_mean
    with torch.device("cpu"):
        net_ = ModuleList_([DistConvertor_(6, symmetric=True)])
        prior = NormalPrior(loc=torch.zeros(1), scale=torch.ones(1))
        model = nf.Model(net_=net_, prior=prior, action=ScalarPhi4Action(kappa=0, m_sq=-1.2, lambd=0.5))
    assert model.fit.graphed is False
    with pytest.raises(ValueError, match="CUDA/HIP"):
        nf.GraphedTrainStep(model, kl_mean, 8)


def test_hidden_slabs_respect_the_budget_and_the_32_bit_site_index():
    """Coupling_._hidden_slabs: slabs of a fused atom -- the byte budget (1024 samples of 32^4 at hidden width 8), never more than
    2^30 sites per slab (the kernels index sites in 32 bits: a narrower net must not get a longer slab), whole coverage."""
    from normflow__amd.nn import AffineCoupling_, ConvAct
    from normflow__amd.mask import EvenOddMask
    from normflow__amd.nn.scalar import couplings_
    with torch.device("cpu"):
        cpl = AffineCoupling_([ConvAct(1, 2, 3, conv_dim=2, hidden_sizes=[8, 8], acts=['tanh', 'tanh', None])], mask=EvenOddMask(shape=(4, 4)))
    V = 32 ** 4
    for B, hidden, want in ((4096, 8, 1024), (4096, 4, 1024), (1000, 8, 1000), (3, 8, 3)):
        v = torch.empty((B, V), device="meta")
        slabs = cpl._hidden_slabs(v, hidden)
        assert slabs[0] == (0, want) and slabs[-1][1] == B
        assert all(b1 - b0 <= want and (b1 - b0) * V <= 1 << 30 for b0, b1 in slabs)
        assert [b0 for b0, _ in slabs[1:]] == [b1 for _, b1 in slabs[:-1]]
    old = couplings_.set_slab_bytes(hidden=8 << 30)
    try:
        assert cpl._hidden_slabs(torch.empty((4096, V), device="meta"), 8)[0] == (0, 256)
    finally:
        couplings_.set_slab_bytes(*old)


def test_bench_dump_outputs_writes_float32_and_a_fixed_sample(tmp_path, monkeypatch):
    """bench.dump_outputs (bench.py --dump-outputs): y and logJ as float32 .npy files, y in full up to the value budget and past
    it a sample of its flat positions that is the same in every run; the headline workload's dump stays within 64 MB."""
    monkeypatch.setattr(os, "environ", os.environ.copy())      # bench.py sets its defaults in os.environ at import
    import bench
    g = torch.Generator().manual_seed(0)
    y = torch.randn((3, 4, 6), generator=g, dtype=torch.float32)
    lj = torch.randn(3, generator=g, dtype=torch.float64)
    bench.dump_outputs(str(tmp_path / "full"), y, lj)
    yf, lf = np.load(tmp_path / "full" / "y.npy"), np.load(tmp_path / "full" / "logJ.npy")
    assert yf.dtype == np.float32 and yf.shape == (3, 4, 6) and np.array_equal(yf, y.numpy())
    assert lf.dtype == np.float32 and np.array_equal(lf, lj.float().numpy())
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), y, lj, max_values=10)
    ya, yb = np.load(tmp_path / "a" / "y.npy"), np.load(tmp_path / "b" / "y.npy")
    assert ya.dtype == np.float32 and ya.shape == (10,) and np.array_equal(ya, yb)
    idx = torch.randint(0, y.numel(), (10,), generator=torch.Generator().manual_seed(bench.DUMP_SEED)).sort().values
    assert np.array_equal(ya, y.reshape(-1)[idx].numpy())
    assert np.array_equal(np.load(tmp_path / "a" / "logJ.npy"), lf)
    assert 4 * (bench.DUMP_Y_VALUES + 1024) <= 64 << 20


def test_bench_full_is_off_by_default(monkeypatch):
    """A plain bench.py run times the headline leg alone; --full adds the other scaling leg (and the rest), an explicit
    --scaling holds either way."""
    monkeypatch.setattr(os, "environ", os.environ.copy())      # bench.py sets its defaults in os.environ at import
    import bench
    a = bench.parse(["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert not a.full and a.scaling == "weak"
    assert bench.parse(["--full"]).scaling == "both"
    assert bench.parse(["--scaling", "strong"]).scaling == "strong"
    assert bench.parse(["--full", "--scaling", "weak"]).scaling == "weak"


@pytest.mark.parametrize("cout,transposed", [(46, False), (8, False), (8, True)])
def test_conv_gather_map_follows_the_pipe_option(cout, transposed):
    """The index map `_conv_launch` packs a layer's weights with is cached per layer shape; the layout it must produce also
    depends on NF_OPT_PIPE (row-packed for the persistent kernel, fragment order without it).  Warm under pipe on, then
    pipe off, then on: each map reproduces, element for element, the packing `conv_weight_for_layer` makes under the option
    in force -- a map cached under the other option would hand the kernel a blob of the wrong shape."""
    lib = _hip.load()
    lat4, k4 = (ctypes.c_int32 * 4)(4, 4, 4, 32), (ctypes.c_int32 * 4)(3, 3, 3, 3)
    cin = 8
    two_site = bool(lib.nf_conv_two_site(cout, 0, 32, 3))
    g = torch.Generator().manual_seed(cout)
    shape = (cin, cout, 3, 3, 3, 3) if transposed else (cout, cin, 3, 3, 3, 3)
    w = torch.randn(shape, generator=g, dtype=torch.float64)

    def direct():
        v = w.flip([2, 3, 4, 5]).transpose(0, 1) if transposed else w
        if two_site:
            v2 = v.new_zeros((16, cin, 3, 3, 3, 4))
            v2[:cout, ..., :3] = v
            v2[8:8 + cout, ..., 1:] = v
            v = v2
        return _hip.conv_weight_for_layer(v, lat4, k4, cin, cout, False, False, _hip.NF_F32)

    def via_map():
        idx, out_shape = _hip._conv_weight_map(w.shape, w.device, lat4, k4, cin, cout, False, two_site, transposed, _hip.NF_F32)
        flat = torch.cat((w.reshape(-1), w.new_zeros(1)))        # index -1: a zero of the padding
        return flat[idx.long()].reshape(out_shape)

    layouts = []
    for pipe in (True, False, True):
        with _hip.options(pipe=pipe):
            layouts.append(lib.nf_conv_weight_layout(lat4, k4, cin, cout, 0, 0, _hip.NF_F32))
            want, got = direct(), via_map()
        assert got.shape == want.shape and torch.equal(got, want), (pipe, tuple(got.shape), tuple(want.shape))
    assert layouts == [1, 0, 1]


def test_data_edit_invalidation_reaches_every_weight_cache():
    """A write through `.data` bumps no version counter, so the caches keyed on (version, data_ptr) -- ConvAct's fp32 copies of
    half weights (_wb) and zero-padded narrow weights (_pad8), GraphedFlow's capture -- cannot see it by themselves; the
    documented `_hip.invalidate_weight_checks()` after the edit must make each of them serve the edited values."""
    from types import SimpleNamespace
    from normflow__amd.graphs import GraphedFlow
    torch.manual_seed(3)
    net = ConvAct(1, 46, 3, conv_dim=4, hidden_sizes=[4, 4], acts=['tanh', 'tanh', None]).to(CPU, torch.float32)
    conv = [m for m in net if hasattr(m, 'weight')][1]
    w8, _ = net._pad8(conv, conv.weight, conv.bias, pad_out=True, pad_in=True)
    state = GraphedFlow._param_state(SimpleNamespace(_net=net))
    conv.weight.data.mul_(0.5)
    _hip.invalidate_weight_checks()
    w8b, _ = net._pad8(conv, conv.weight, conv.bias, pad_out=True, pad_in=True)
    assert torch.equal(w8b[:4, :4], conv.weight.detach()) and not torch.equal(w8b, w8)
    assert GraphedFlow._param_state(SimpleNamespace(_net=net)) != state
    half = ConvAct(1, 2, 3, conv_dim=2, hidden_sizes=[4], acts=['tanh', None]).to(CPU, torch.float16)
    hconv = [m for m in half if hasattr(m, 'weight')][0]
    w32, _ = half._wb(hconv)
    hconv.weight.data.mul_(0.5)
    _hip.invalidate_weight_checks()
    w32b, _ = half._wb(hconv)
    assert torch.equal(w32b, hconv.weight.detach().float()) and not torch.equal(w32b, w32)

"""Per-site K4 densities on one GPU, on a (B, L^4) fp32 field, in GB/s of algorithmic traffic:

  sum           nf_distconv, SplineNet_ forward summed per sample: read x, write y: 8 B per element
  sites         nf_distconv_sites, per site: read x, write y and the per-site log J: 12 B per element
  sites_log0    the same with a per-site log0 read: 16 B per element
  sum_vjp       nf_distconv_vjp, summed: read x and grad y, write grad x: 12 B per element
  sites_vjp     nf_distconv_sites_vjp, per site: read x, grad y and grad log J, write grad x: 16 B per element
  wrap_masked   InvisibilityMaskWrapperModule_(SplineNet_) on an even-odd mask, the one masked pass: 8 B per element
  wrap_generic  the same wrapper by the reference's composition (split, per-site pass, purify, sum, cat), counted at
                the masked pass's 8 B per element (its real traffic is several times that)
  action        nf_phi4_action: read phi: 4 B per element
  density       nf_phi4_action_density: read phi, write the density: 8 B per element

    python tools/site_density_bench.py [--batch 1024] [--lattice 32] [--reps 20]
Times are HIP events around `reps` calls after 3 warm-up calls.  Prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("NORMFLOW_AMD_KEEP_TORCH_DEFAULTS", "1")
import torch  # noqa: E402

from normflow__amd import _hip  # noqa: E402
from normflow__amd.action import ScalarPhi4Action  # noqa: E402
from normflow__amd.mask import EvenOddMask  # noqa: E402
from normflow__amd.nn import InvisibilityMaskWrapperModule_, SplineNet_  # noqa: E402

DEV = torch.device("cuda:0")


def _events_ms(f, reps, warm=3):
    for _ in range(warm):
        f()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        f()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--lattice", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("site_density_bench needs a GPU")
    B, L = args.batch, args.lattice
    V = L ** 4
    N = B * V
    torch.manual_seed(0)
    spline = SplineNet_(10)
    with torch.no_grad():
        for p in spline.parameters():
            p.copy_(0.5 * torch.randn(p.shape))
    spline = spline.to(DEV, torch.float32)
    knots = spline.knots().detach()
    x = torch.rand((B, V), dtype=torch.float32, device=DEV)
    log0 = torch.randn_like(x)
    gy, gl = torch.randn_like(x), torch.randn_like(x)
    gx = torch.empty_like(x)
    gk = torch.empty(3, knots.shape[1], dtype=torch.float64, device=DEV)
    ws_vjp = _hip._workspace(B, V, DEV)
    lib = _hip.load()
    S = _hip.STAGE_SPLINE

    def sites(l0=None):
        return _hip.DistConvSitesFn.apply(x, knots, l0, None, S, False, True)

    gls = torch.randn(B, dtype=torch.float32, device=DEV)

    def sum_vjp():
        _hip._check(lib.nf_distconv_vjp(_hip._ptr(x), _hip._ptr(knots), knots.shape[1], _hip._ptr(gy), _hip._ptr(gls),
                                        _hip._ptr(gx), _hip._ptr(gk), B, V, S, 0, _hip._ptr(ws_vjp), ws_vjp.numel(),
                                        _hip.NF_F32, _hip._stream()), "nf_distconv_vjp")

    def vjp():
        _hip._check(lib.nf_distconv_sites_vjp(_hip._ptr(x), _hip._ptr(knots), knots.shape[1], None, _hip._ptr(gy),
                                              _hip._ptr(gl), _hip._ptr(gx), _hip._ptr(gk), B, V, S, 0, _hip.DC_SITES,
                                              _hip._ptr(ws_vjp), ws_vjp.numel(), _hip.NF_F32, _hip._stream()),
                    "nf_distconv_sites_vjp")

    xf = x.reshape((B,) + (L,) * 4)
    wrap = InvisibilityMaskWrapperModule_(spline, mask=EvenOddMask(shape=(L,) * 4).to(DEV))
    generic = InvisibilityMaskWrapperModule_(spline, mask=wrap.mask)
    generic._activity = lambda t: None                    # force the reference's composition
    act = ScalarPhi4Action(m_sq=-1.2, lambd=0.8, kappa=0.3)
    res = dict(workload=f"SplineNet_(10) fp32 ({B}, {L}^4)", elements=N)
    with torch.no_grad():
        for name, fn, bpe in (("sum", lambda: _hip.DistConvFn.apply(x, knots, None, S, False), 8),
                              ("sites", sites, 12), ("sites_log0", lambda: sites(log0), 16), ("sum_vjp", sum_vjp, 12),
                              ("sites_vjp", vjp, 16),
                              ("wrap_masked", lambda: wrap(xf), 8), ("wrap_generic", lambda: generic(xf), 8),
                              ("action", lambda: act.action(xf), 4), ("density", lambda: act.action_density(xf), 8)):
            ms = _events_ms(fn, args.reps)
            res[f"{name}_ms"] = round(ms, 4)
            res[f"{name}_GBps"] = round(bpe * N / ms / 1e6, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

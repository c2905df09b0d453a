"""The nf_pade maps on one GPU (--kind pade22 | pade32 | tanh): forward, inverse and VJP (nf_pade / nf_pade_vjp) on a
(B, L^4) fp32 field, in GB/s of algorithmic traffic, next to nf_distconv's Expit_ pass on the same field (the element-wise
pass it should match) and, for pade32 and tanh, next to the eager torch composition of the same formulas (`eager_*`:
forward, inverse, and forward + autograd backward against the kernel's fwd + vjp).

  fwd / inv     read x, write y and the per-sample log J: 8 B per element
  fwd_sites     per-site log J (propagate_density): read x, write y and log J: 12 B per element
  vjp           read x and grad y, write grad x (grad log J per sample): 12 B per element
  expit         nf_distconv stage 1 (Expit_.forward): read x, write y: 8 B per element

    python tools/pade_bench.py [--kind pade22] [--batch 1024] [--lattice 32] [--reps 20]
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
from normflow__amd.nn import Expit_, Module_, Pade22_, Pade32_, Tanh_  # noqa: E402

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


LN2 = 0.6931471805599453


def _eager_tanh(x, a, inverse):
    if inverse:
        return torch.atanh(x), -(torch.log1p(x) + torch.log1p(-x)).sum(1)
    ax = x.abs()
    return torch.tanh(x), -2 * (ax + torch.log1p(torch.exp(-2 * ax)) - LN2).sum(1)


def _eager_pade32(x, a, inverse):
    """The kernel's formulas as torch ops (|x| <= 1e3 here: the overflow-free forms are not needed)."""
    def fg(t):
        s = t * t
        den = 1 + a * s
        return t * (a + s) / den, (a * s * s + (3 - a * a) * s + a) / (den * den)
    if not inverse:
        f, g = fg(x)
        return f, torch.log(g).sum(1)
    ay = x.abs()
    small = ay <= 1
    c = 1 / (ay * ay).clamp(min=1e-30)
    A2 = torch.where(small, -a * ay, -a * torch.ones_like(ay))
    A1 = torch.where(small, a * torch.ones_like(ay), a * c)
    A0 = torch.where(small, -ay, -c)
    p3 = (A1 - A2 * A2 / 3) / 3
    hq = -0.5 * (A2 * (2.0 / 27.0 * A2 * A2 - A1 / 3) + A0)
    D = (hq * hq + p3 * p3 * p3).clamp(min=0)
    w = hq + torch.copysign(torch.sqrt(D), hq)
    U = torch.copysign(w.abs().pow(1.0 / 3.0), w)
    t = (U - p3 / U - A2 / 3) * torch.where(small, torch.ones_like(ay), ay)
    for _ in range(2):
        f, g = fg(t)
        t = t - (f - ay) / g
    t = torch.copysign(t, x)
    return t, -torch.log(fg(t)[1]).sum(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", choices=("pade22", "pade32", "tanh"), default="pade22")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--lattice", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pade_bench needs a GPU")
    B, V = args.batch, args.lattice ** 4
    N = B * V
    torch.manual_seed(0)
    d0 = d1 = eager = None
    if args.kind == "pade22":
        mod, code = Pade22_().to(DEV, torch.float32), _hip.PADE22
        with torch.no_grad():
            mod.w0.fill_(0.7)
            mod.w1.fill_(-0.4)
        d0 = torch.nn.functional.softplus(mod.w0.detach(), beta=LN2)
        d1 = torch.nn.functional.softplus(mod.w1.detach(), beta=LN2)
        x = torch.rand((B, V), dtype=torch.float32, device=DEV)
        x_inv = x
    elif args.kind == "pade32":
        mod, code = Pade32_().to(DEV, torch.float32), _hip.PADE32
        with torch.no_grad():
            mod.w0.fill_(0.7)
        d0 = 3 * torch.special.expit(mod.w0.detach())
        x = 2 * torch.randn((B, V), dtype=torch.float32, device=DEV)
        x_inv, eager = x, _eager_pade32
    else:
        mod, code = Tanh_().to(DEV, torch.float32), _hip.TANH
        x = 2.5 * torch.randn((B, V), dtype=torch.float32, device=DEV)
        x_inv, eager = torch.rand((B, V), dtype=torch.float32, device=DEV) * 1.99 - 0.995, _eager_tanh
    gy = torch.randn_like(x)
    gl = torch.randn(B, dtype=torch.float32, device=DEV)
    gx = torch.empty_like(x)
    gd = torch.empty(2, 1, dtype=torch.float64, device=DEV)
    layout = (B, B, 1, V)
    ws = _hip._pade_workspace(layout, DEV)
    lib = _hip.load()

    def vjp():
        _hip._check(lib.nf_pade_vjp(_hip._ptr(x), _hip._ptr(d0), _hip._ptr(d1), _hip._ptr(gy), _hip._ptr(gl),
                                    _hip._ptr(gx), _hip._ptr(gd), *layout, code, 0, 0, _hip._ptr(ws), ws.numel(),
                                    _hip.NF_F32, _hip._stream()), "nf_pade_vjp")

    def sites():
        Module_.propagate_density = True
        try:
            mod(x)
        finally:
            Module_.propagate_density = False

    expit = Expit_()
    res = dict(workload=f"{type(mod).__name__} fp32 ({B}, {args.lattice}^4)", elements=N)
    with torch.no_grad():
        for name, fn, bpe in (("fwd", lambda: mod(x), 8), ("inv", lambda: mod.backward(x_inv), 8),
                              ("fwd_sites", sites, 12), ("vjp", vjp, 12), ("expit", lambda: expit(x), 8)):
            ms = _events_ms(fn, args.reps)
            res[f"{name}_ms"] = round(ms, 4)
            res[f"{name}_GBps"] = round(bpe * N / ms / 1e6, 1)
        if eager is not None:
            a = d0
            res["eager_fwd_ms"] = round(_events_ms(lambda: eager(x, a, False), args.reps), 4)
            res["eager_inv_ms"] = round(_events_ms(lambda: eager(x_inv, a, True), args.reps), 4)
    if eager is not None:
        xg = x.clone().requires_grad_(True)

        def fwd_bwd():
            y, lj = eager(xg, d0, False)
            torch.autograd.grad((y * gy).sum() + (lj * gl).sum(), xg)
        res["eager_fwd_bwd_ms"] = round(_events_ms(fwd_bwd, max(1, args.reps // 4)), 4)
        res["kernel_fwd_plus_vjp_ms"] = round(res["fwd_ms"] + res["vjp_ms"], 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

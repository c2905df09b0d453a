"""Pade22_ on one GPU: forward, inverse and VJP (nf_pade / nf_pade_vjp) on a (B, L^4) fp32 field, in GB/s of
algorithmic traffic, next to nf_distconv's Expit_ pass on the same field (the element-wise pass it should match).

  fwd / inv     read x, write y and the per-sample log J: 8 B per element
  fwd_sites     per-site log J (propagate_density): read x, write y and log J: 12 B per element
  vjp           read x and grad y, write grad x (grad log J per sample): 12 B per element
  expit         nf_distconv stage 1 (Expit_.forward): read x, write y: 8 B per element

    python tools/pade_bench.py [--batch 1024] [--lattice 32] [--reps 20]
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
from normflow__amd.nn import Expit_, Module_, Pade22_  # noqa: E402

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
        raise SystemExit("pade_bench needs a GPU")
    B, V = args.batch, args.lattice ** 4
    N = B * V
    torch.manual_seed(0)
    mod = Pade22_().to(DEV, torch.float32)
    with torch.no_grad():
        mod.w0.fill_(0.7)
        mod.w1.fill_(-0.4)
    x = torch.rand((B, V), dtype=torch.float32, device=DEV)
    gy = torch.randn_like(x)
    gl = torch.randn(B, dtype=torch.float32, device=DEV)
    gx = torch.empty_like(x)
    gd = torch.empty(2, 1, dtype=torch.float64, device=DEV)
    d0 = torch.nn.functional.softplus(mod.w0.detach(), beta=0.6931471805599453)
    d1 = torch.nn.functional.softplus(mod.w1.detach(), beta=0.6931471805599453)
    layout = (B, B, 1, V)
    ws = _hip._pade_workspace(layout, DEV)
    lib = _hip.load()

    def vjp():
        _hip._check(lib.nf_pade_vjp(_hip._ptr(x), _hip._ptr(d0), _hip._ptr(d1), _hip._ptr(gy), _hip._ptr(gl),
                                    _hip._ptr(gx), _hip._ptr(gd), *layout, _hip.PADE22, 0, 0, _hip._ptr(ws), ws.numel(),
                                    _hip.NF_F32, _hip._stream()), "nf_pade_vjp")

    def sites():
        Module_.propagate_density = True
        try:
            mod(x)
        finally:
            Module_.propagate_density = False

    expit = Expit_()
    res = dict(workload=f"Pade22_ fp32 ({B}, {args.lattice}^4)", elements=N)
    with torch.no_grad():
        for name, fn, bpe in (("fwd", lambda: mod(x), 8), ("inv", lambda: mod.backward(x), 8),
                              ("fwd_sites", sites, 12), ("vjp", vjp, 12), ("expit", lambda: expit(x), 8)):
            ms = _events_ms(fn, args.reps)
            res[f"{name}_ms"] = round(ms, 4)
            res[f"{name}_GBps"] = round(bpe * N / ms / 1e6, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""The spectral first block of the example network on one GPU: transform='fft' (torch.fft / rocFFT, the default) against
transform='hartley' (nf_spectral.hip, one launch, the sample resident in LDS), next to the coupling stack of the same
config so that the block's share of a pass is visible.  fp32, HIP events.

  fftnet_fwd     FFTNet_.forward under no_grad
  block_fwd      PSDBlock_.forward under no_grad
  block_train    PSDBlock_ forward + backward of mean(y^2) + mean(log J)
  stack_fwd      the config's coupling stack (config 2: 4 affine layers; config 3: 8 RQ-spline layers), no_grad
each eager and replayed from a HIP graph (GraphedFlow for the no_grad passes; a torch.cuda.graph of forward + backward for
block_train).  A path that cannot be captured is reported as such ("capture failed: ..."), not timed.
  filter_kernel  nf_spectral_filter alone: its algorithmic rate (read x, write y: 8 B/site) as GB/s and as a share of the
                 HBM rate (8 TB/s); PSDBlock_ reads x once more for the zero mode (12 B/site)

    python tools/spectral_bench.py [--reps 200] [--rounds 7] [--only config2|config3]
Every variant is warmed up, then timed in `--rounds` interleaved rounds of `--reps` calls each (both transforms in the same
process and run); the JSON line per shape carries the medians and the [min, max] over the rounds, in microseconds."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
os.environ.setdefault("NORMFLOW_AMD_KEEP_TORCH_DEFAULTS", "1")
import torch  # noqa: E402

from normflow__amd import GraphedFlow, _hip  # noqa: E402
from normflow__amd.nn import FFTNet_, MeanFieldNet_, PSDBlock_  # noqa: E402

DEV = torch.device("cuda:0")
HBM_GBPS = 8000.0


def _events_us(f, reps):
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        f()
    t1.record()
    t1.synchronize()
    return 1e3 * t0.elapsed_time(t1) / reps


def _block(lattice, transform):
    torch.manual_seed(0)
    blk = PSDBlock_(mfnet_=MeanFieldNet_.build(knots_len=10, symmetric=True, final_scale=True, smooth=True),
                    fftnet_=FFTNet_.build(lattice, knots_len=10, ignore_zeromode=True, transform=transform))
    return blk.to(DEV, torch.float32)


def _train_call(blk, x):
    params = list(blk.parameters())

    def step():
        for p in params:
            p.grad = None
        y, lj = blk(x)
        ((y ** 2).mean() + lj.mean()).backward()
    return step


def _graphed_train(blk, x):
    """forward + backward of the block as one HIP graph (what GraphedTrainStep does for a whole model)."""
    step = _train_call(blk, x)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream(DEV).wait_stream(side)
    for p in blk.parameters():
        p.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y, lj = blk(x)
        ((y ** 2).mean() + lj.mean()).backward()
    return graph.replay


def _capture(make):
    try:
        return make(), None
    except Exception as e:                              # reported in the JSON line instead of a time
        torch.cuda.synchronize()
        return None, f"capture failed: {type(e).__name__}: {str(e).splitlines()[0][:120]}"


def measure(name, lattice, kinds, B, reps, rounds):
    from config_bench import build
    torch.manual_seed(0)
    x = torch.randn((B,) + tuple(lattice), device=DEV, dtype=torch.float32)
    calls, failed = {}, {}

    def add(key, eager, make_graph):
        calls[key + ".eager"] = eager
        g, why = _capture(make_graph)
        if g is None:
            failed[key + ".graph"] = why
        else:
            calls[key + ".graph"] = g

    def nograd(f):
        def run():
            with torch.no_grad():
                f()
        return run

    for tr in ("fft", "hartley"):
        blk = _block(lattice, tr)
        add(f"fftnet_fwd.{tr}", nograd(lambda b=blk: b.fftnet_(x)),
            lambda b=blk: (lambda g: (lambda: g(x, clone=False)))(GraphedFlow(b.fftnet_, x)))
        add(f"block_fwd.{tr}", nograd(lambda b=blk: b(x)),
            lambda b=blk: (lambda g: (lambda: g(x, clone=False)))(GraphedFlow(b, x)))
        add(f"block_train.{tr}", _train_call(blk, x), lambda b=blk: _graphed_train(b, x))
    stack = build(tuple(lattice), kinds)
    add("stack_fwd", nograd(lambda: stack(x)), lambda: (lambda g: (lambda: g(x, clone=False)))(GraphedFlow(stack, x)))
    # the kernel alone
    w = _block(lattice, "hartley").fftnet_._weights().detach().contiguous()
    y = torch.empty_like(x)
    lat_c = _hip._c_ints(list(lattice))
    lib = _hip.load()
    calls["filter_kernel"] = lambda: _hip._check(
        lib.nf_spectral_filter(_hip._ptr(x), _hip._ptr(w), None, _hip._ptr(y), None, lat_c, len(lattice), B, _hip.NF_F32,
                               _hip._stream()), "nf_spectral_filter")
    times = {k: [] for k in calls}
    for f in calls.values():                                # warm-up: code objects, FFT plans, allocator
        for _ in range(10):
            f()
    for _ in range(rounds):
        for k, f in calls.items():
            times[k].append(_events_us(f, reps))
    out = dict(shape=name, lattice=list(lattice), batch=B, dtype="float32", reps=reps, rounds=rounds, unit="us")
    for k in calls:
        out[k] = round(statistics.median(times[k]), 2)
        out[k + ".min_max"] = [round(min(times[k]), 2), round(max(times[k]), 2)]
    out.update(failed)
    for q in ("fftnet_fwd", "block_fwd", "block_train"):
        for mode in ("eager", "graph"):
            a, b = out.get(f"{q}.fft.{mode}"), out.get(f"{q}.hartley.{mode}")
            if isinstance(a, float) and isinstance(b, float):
                out[f"{q}.{mode}.fft_over_hartley"] = round(a / b, 2)
    for mode in ("eager", "graph"):
        s = out.get(f"stack_fwd.{mode}")
        for tr in ("fft", "hartley"):
            b = out.get(f"block_fwd.{tr}.{mode}")
            if isinstance(s, float) and isinstance(b, float):
                out[f"block_share_of_pass_pct.{tr}.{mode}"] = round(100.0 * b / (b + s), 1)
    sites = B * x[0].numel()
    gbps = 8.0 * sites / out["filter_kernel"] / 1e3
    out["filter_kernel.algorithmic_GBps"] = round(gbps, 1)
    out["filter_kernel.share_of_hbm_rate_pct"] = round(100.0 * gbps / HBM_GBPS, 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--only", choices=["config2", "config3"], default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("spectral_bench needs a GPU")
    shapes = [("config2", "config2_16x16", (16, 16), ['affine'] * 4, 512),
              ("config3", "config3_16x16x16", (16, 16, 16), ['rqs'] * 8, 1024)]
    for key, name, lattice, kinds, B in shapes:
        if a.only in (None, key):
            print(json.dumps(measure(name, lattice, kinds, B, a.reps, a.rounds)), flush=True)


if __name__ == "__main__":
    main()

"""Rows per second of `measure`'s three paths on one GPU, in one run (HIP events after a warm-up, no_grad):
  kernel    nf_lattice_measure: every statistic of a row in one pass over it (normflow__amd/csrc/nf_measure.hip)
  tiled     nf_lattice_measure_tiled: the same by bricks, for rows of any size (normflow__amd/csrc/nf_measure_tiled.hip);
            timed on the 4-d lattices of the list: 32^4 (fp32: the one class both kernels take) and 48^4
  composed  the same definitions from torch ops in double: d + 3 passes (what `measure` runs where no kernel applies)
on 16^2 x 65536 rows, 16^3 x 4096, 32^3 x 256, 32^4 x 16 and 48^4 x 4, in fp32 and fp64; also the algorithmic bytes per
second a kernel's time stands for: V sizeof(dtype) per row, the field read once.  Where the kernel does not take the
lattice (its planner says why) it is not timed.  The paths are checked against the composed one at the timed size, timed
alternately `--reps` times each, and the figures are medians.  `tiled_beats_composed`: the tiled median beats the composed
one by `margin`, the larger of 10 % and the two paths' spreads (max - min) / median in this run -- the rule by which
`route` (normflow__amd/lib/observables.py) may send a class to the tiled kernel.

    python tools/measure_bench.py [--reps 5] [--shapes all|small|large] [--brick-bytes B]
--brick-bytes: the cap of a brick handed to the tiled kernel (default: the library's).  Prints one JSON line per shape and
dtype."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("NORMFLOW_AMD_KEEP_TORCH_DEFAULTS", "1")
import torch  # noqa: E402

from normflow__amd import _hip  # noqa: E402
from normflow__amd.lib import observables as OB  # noqa: E402

DEV = torch.device("cuda:0")
SHAPES = [((16, 16), 65536), ((16, 16, 16), 4096)]
LARGE = [((32, 32, 32), 256), ((32, 32, 32, 32), 16), ((48, 48, 48, 48), 4)]


def _ms(f):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    f()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def _spread(ts):
    return (max(ts) - min(ts)) / statistics.median(ts)


def bench(lattice, N, dtype, reps, brick_bytes=None):
    g = torch.Generator(device="cpu").manual_seed(0)
    x = torch.randn((N,) + lattice, generator=g, dtype=torch.float32, device="cpu").to(device=DEV, dtype=dtype)
    res = dict(lattice=list(lattice), rows=N, dtype=str(dtype).replace("torch.", ""))
    has_kernel = _hip.measure_supported(lattice, dtype)
    refused = None if has_kernel else _hip.load().nf_last_error_string().decode()       # the planner's reason
    composed = lambda: OB.measure(x, path='composed')
    kernel = (lambda: OB.measure(x, path='kernel')) if has_kernel else (lambda: None)
    call = (lambda: _hip.lattice_measure(x)) if has_kernel else (lambda: None)         # the launches alone
    has_tiled = len(lattice) == 4 and _hip.measure_tiled_supported(lattice, dtype, brick_bytes)
    tcall = (lambda: _hip.lattice_measure_tiled(x, brick_bytes=brick_bytes)) if has_tiled else (lambda: None)
    # what measure(x, path='tiled') does, at the cap asked for
    tiled = (lambda: OB.Measurement(*OB._split(tcall(), lattice), lattice)) if has_tiled else (lambda: None)
    with torch.no_grad():
        for _ in range(2):                      # warm-up: code objects and the allocator
            kernel()
            tiled()
            composed()
        torch.cuda.synchronize()
        rel = lambda a, b: ((a - b).abs().max() / b.abs().max()).item()

        def against(k, c):
            out = {n: float(f"{rel(getattr(k, n), getattr(c, n)):.2e}") for n in ('sum_phi2', 'sum_phi4', 'links')}
            out['slices'] = float(f"{max(rel(a, b) for a, b in zip(k.slices, c.slices)):.2e}")
            return out
        if has_tiled:
            res['tiled_check'] = against(tiled(), composed())
        if has_kernel:                          # the paths against each other at the timed size
            res['check'] = against(kernel(), composed())
        tk, tc, tb, tt, ttc = [], [], [], [], []
        for _ in range(reps):                   # alternate them, so that a drift of the machine hits all
            tk.append(_ms(kernel))
            tt.append(_ms(tiled))
            tc.append(_ms(composed))
            tb.append(_ms(call))
            ttc.append(_ms(tcall))
    ms_c = statistics.median(tc)
    res.update(composed_rows_per_s=round(N / ms_c * 1e3, 1), composed_ms=round(ms_c, 4),
               composed_ms_spread=[round(min(tc), 4), round(max(tc), 4)])
    nbytes = N * x[0].numel() * x.element_size()
    if has_tiled:
        ms_t, ms_tb = statistics.median(tt), statistics.median(ttc)
        margin = max(0.10, _spread(tt), _spread(tc))
        res.update(tiled_rows_per_s=round(N / ms_t * 1e3, 1), tiled_ms=round(ms_t, 4),
                   tiled_ms_spread=[round(min(tt), 4), round(max(tt), 4)], tiled_over_composed=round(ms_c / ms_t, 2),
                   margin=round(margin, 3), tiled_beats_composed=bool(ms_c / ms_t >= 1 + margin),
                   tiled_call_ms=round(ms_tb, 4), tiled_call_ms_spread=[round(min(ttc), 4), round(max(ttc), 4)],
                   tiled_algorithmic_TB_per_s=round(nbytes / (ms_tb * 1e-3) / 1e12, 3),
                   tiled_plan=_hip.measure_tiled_plan(lattice, dtype, brick_bytes))
    if not has_kernel:
        res['kernel'] = refused
        return res
    ms_k, ms_b = statistics.median(tk), statistics.median(tb)
    res.update(kernel_rows_per_s=round(N / ms_k * 1e3, 1), kernel_ms=round(ms_k, 4),
               kernel_ms_spread=[round(min(tk), 4), round(max(tk), 4)], kernel_over_composed=round(ms_c / ms_k, 2),
               call_ms=round(ms_b, 4), call_ms_spread=[round(min(tb), 4), round(max(tb), 4)],
               algorithmic_TB_per_s=round(nbytes / (ms_b * 1e-3) / 1e12, 3), plan=_hip.measure_plan(lattice, dtype))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", choices=("all", "small", "large"), default="all")
    ap.add_argument("--brick-bytes", type=int, default=None, help="the cap of a brick of the tiled kernel (default: the library's)")
    a = ap.parse_args()
    shapes = (SHAPES if a.shapes != "large" else []) + (LARGE if a.shapes != "small" else [])
    for lattice, N in shapes:
        for dtype in (torch.float32, torch.float64):
            print(json.dumps(bench(lattice, N, dtype, a.reps, a.brick_bytes)), flush=True)


if __name__ == "__main__":
    main()

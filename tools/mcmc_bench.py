"""Cost of one `model.mcmc.sample__` call on one GPU, and the Metropolis step's share of it (HIP events, no_grad, fp32):
  proposals   posterior.sample__(B) alone: prior draw, flow, action -- the work every variant has to do
  legacy      mcmc.sample__(B): the reference's host accept/reject (n_chains=None)
  chains1     mcmc.sample__(B, n_chains=1):  nf_metropolis_chains + nf_metropolis_select, one read of the flags
  chains64    mcmc.sample__(B, n_chains=64): the same with 64 independent chains
The sampler's own share is (call - proposals) / call.  Every variant is warmed up, then timed in `--rounds` interleaved
rounds of `--reps` calls each; the JSON line carries the median and the [min, max] over the rounds.  Kernel times of their
own: run under `rocprofv3 --kernel-trace --stats -d DIR -- python tools/mcmc_bench.py`.

    python tools/mcmc_bench.py [--reps 100] [--rounds 7] [--only config2|config3]
Shapes: config 2's net (16^2, 4 affine layers) at batch 512 and config 3's net (16^3, 8 RQ-spline layers) at batch 1024,
each with `posterior.graphed` off and on.  Prints one JSON line per shape and setting."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
os.environ.setdefault("NORMFLOW_AMD_KEEP_TORCH_DEFAULTS", "1")
import numpy as np  # noqa: E402
import torch  # noqa: E402

import normflow__amd as nf  # noqa: E402
from normflow__amd.mcmc import MCMCSampler  # noqa: E402
from normflow__amd.prior import NormalPrior  # noqa: E402
from normflow__amd.action import ScalarPhi4Action  # noqa: E402

DEV = torch.device("cuda:0")
VARIANTS = ("proposals", "legacy", "chains1", "chains64")


def _events_ms(f, reps):
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        f()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / reps


def measure(name, net_, lattice, B, graphed, reps, rounds):
    prior = NormalPrior(loc=torch.zeros(lattice, device=DEV), scale=torch.ones(lattice, device=DEV))
    action = ScalarPhi4Action(kappa=0.25, m_sq=-0.5, lambd=0.5)

    model = nf.Model(net_=net_, prior=prior, action=action)
    model.posterior.graphed = graphed
    samplers = {v: MCMCSampler(model) for v in VARIANTS[1:]}     # one per variant: each keeps its own chain state
    calls = {
        "proposals": lambda: model.posterior.sample__(B),
        "legacy": lambda: samplers["legacy"].sample__(B),
        "chains1": lambda: samplers["chains1"].sample__(B, n_chains=1),
        "chains64": lambda: samplers["chains64"].sample__(B, n_chains=64),
    }
    torch.manual_seed(0)
    np.random.seed(0)
    times = {v: [] for v in VARIANTS}
    with torch.no_grad(), open(os.devnull, "w") as null:
        stdout, sys.stdout = sys.stdout, null          # the samplers announce a fresh start
        try:
            for v in VARIANTS:                         # warm-up: code objects, graph capture, allocator
                for _ in range(5):
                    calls[v]()
            for _ in range(rounds):
                for v in VARIANTS:
                    times[v].append(_events_ms(calls[v], reps))
        finally:
            sys.stdout = stdout
    med = {v: statistics.median(times[v]) for v in VARIANTS}
    out = dict(shape=name, lattice=list(lattice), batch=B, graphed=graphed, reps=reps, rounds=rounds)
    for v in VARIANTS:
        out[f"ms_{v}"] = round(med[v], 4)
        out[f"ms_{v}_min_max"] = [round(min(times[v]), 4), round(max(times[v]), 4)]
    for v in VARIANTS[1:]:
        out[f"sampler_share_pct_{v}"] = round(100.0 * (med[v] - med["proposals"]) / med[v], 2)
        out[f"accept_rate_{v}"] = round(float(np.mean(samplers[v].history.accept_rate)), 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--only", choices=["config2", "config3"], default=None)
    a = ap.parse_args()
    from config_bench import build
    shapes = [("config2", "config2_16x16_4affine", (16, 16), ['affine'] * 4, 512),
              ("config3", "config3_16x16x16_8rqs", (16, 16, 16), ['rqs'] * 8, 1024)]
    for key, name, lattice, kinds, B in shapes:
        if a.only not in (None, key):
            continue
        torch.manual_seed(0)
        net_ = build(lattice, kinds)
        for graphed in (False, True):
            print(json.dumps(measure(name, net_, lattice, B, graphed, a.reps, a.rounds)), flush=True)


if __name__ == "__main__":
    main()

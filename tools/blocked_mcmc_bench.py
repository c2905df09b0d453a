"""Cost of one block step of BlockedMCMCSampler on one GPU, split into its parts (HIP events, no_grad, fp32):
  step          sampler.step: nf_block_propose, flow + action at batch C, nf_block_accept, and the host work between
  flow_action   net_(x), prior.log_prob(x) - logJ and -action(y) alone: the work the sampler has to do anyway
  propose       nf_block_propose alone;  accept: nf_block_accept alone
The sampler's own share is (step - flow_action) / step.  Kernel times of their own: run under
`rocprofv3 --kernel-trace --stats -d DIR -- python tools/blocked_mcmc_bench.py`.

    python tools/blocked_mcmc_bench.py [--reps 50] [--only config3|headline]
Shapes: config 3's net (16^3, 8 RQ-spline layers) with C = 1024 chains and 16 blocks; the headline net (bench.py: 32^4,
one coupling block of 8 RQ-spline layers) with C = 64 and 32 blocks.  Prints one JSON line per shape."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
os.environ.setdefault("NORMFLOW_AMD_KEEP_TORCH_DEFAULTS", "1")
import torch  # noqa: E402

import normflow__amd as nf  # noqa: E402
from normflow__amd import _hip  # noqa: E402
from normflow__amd.prior import NormalPrior  # noqa: E402
from normflow__amd.action import ScalarPhi4Action  # noqa: E402

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


def measure(name, net_, lattice, C, n_blocks, reps):
    prior = NormalPrior(loc=torch.zeros(lattice, device=DEV), scale=torch.ones(lattice, device=DEV))
    model = nf.Model(net_=net_, prior=prior, action=ScalarPhi4Action(kappa=0.25, m_sq=-0.5, lambd=0.5))
    s = model.blocked_mcmc
    bl = prior.nvar // n_blocks
    prior.setup_blockupdater(bl)
    bu = prior.blockupdater
    torch.manual_seed(0)
    x = prior.sample(C).contiguous()
    ref = torch.zeros(C, dtype=torch.float64, device=DEV)
    flags = torch.empty((n_blocks, C), dtype=torch.uint8, device=DEV)
    k = [0]

    def step():
        s.step(x, k[0], ref, flags[k[0]], force_accept=True)
        k[0] = (k[0] + 1) % n_blocks

    def flow_action():
        y, logJ = net_(x)
        return prior.log_prob(x) - logJ, -model.action(y)

    with torch.no_grad():
        t_step = _events_ms(step, reps)
        t_flow = _events_ms(flow_action, reps)
        bu(x, 0)
        logq, logp = flow_action()
        t_prop = _events_ms(lambda: bu(x, 0), reps)
        t_acc = _events_ms(lambda: _hip.block_accept(x, bu.backup_block, logq, logp, ref, flags[0], bl, 0), reps)
        # a whole call of the sampler (n_blocks steps per sweep + one flow pass per sweep to return the state)
        torch.manual_seed(1)
        s.sample__(batch_size=C, n_blocks=n_blocks, n_chains=C)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        s.sample__(batch_size=2 * C, n_blocks=n_blocks, n_chains=C)
        t1.record()
        t1.synchronize()
        t_call = t0.elapsed_time(t1)
    return dict(shape=name, lattice=list(lattice), chains=C, n_blocks=n_blocks, block_len=bl,
                ms_per_block_step=round(t_step, 4), ms_flow_action=round(t_flow, 4),
                ms_propose=round(t_prop, 4), ms_accept=round(t_acc, 4),
                sampler_share_pct=round(100.0 * (t_step - t_flow) / t_step, 2),
                kernels_share_pct=round(100.0 * (t_prop + t_acc) / t_step, 2),
                configs_per_s_steps=round(C / (n_blocks * t_step) * 1e3, 1),
                configs_per_s_sample=round(2 * C / t_call * 1e3, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--only", choices=["config3", "headline"], default=None)
    a = ap.parse_args()
    if a.only in (None, "config3"):
        from config_bench import build
        torch.manual_seed(0)
        net3 = build((16, 16, 16), ['rqs'] * 8)
        print(json.dumps(measure("config3_16x16x16_8rqs", net3, (16, 16, 16), 1024, 16, a.reps)), flush=True)
    if a.only in (None, "headline"):
        from bench import build_net
        net_, _ = build_net((32, 32, 32, 32), 8, 16, DEV, seed=0)
        print(json.dumps(measure("headline_32x32x32x32_8rqs", net_, (32, 32, 32, 32), 64, 32, max(5, a.reps // 5))),
              flush=True)


if __name__ == "__main__":
    main()

"""Trajectories per second of HMCSampler's three paths on one GPU, in one run (HIP events after a warm-up, no_grad):
  fused     nf_phi4_hmc: `--traj` trajectories of every chain in ONE launch (the chain resident in a CU)
  composed  the same algorithm from nf_normal_sample, the action and its VJP, torch ops and nf_block_accept,
            trajectory by trajectory (what the sampler runs where the fused kernel does not apply)
  tiled     nf_phi4_hmc_tiled: the chains in HBM, n_md + 2 launches per trajectory (any lattice)
at n_md = 10, dt = 0.1, fp32 and fp64, on 16^2 x 512 and 16^3 x 1024 chains (all three paths) and on 32^3 x 256, 16^4 x 64,
32^4 x 16 and 48^4 x 4 (beyond the fused kernel: tiled and composed; `--shapes small` leaves these out).  For the tiled
path also the bare call's time per MD step and site and the algorithmic bytes per second it stands for: 16 (fp32) or 32
(fp64) bytes x sites x steps -- phi and pi read once and written once -- over the time of the whole call, which also
contains begin and commit.  The outputs of the paths are checked against each other at the timed sizes (one trajectory,
momenta handed in).  Also the fused kernel's time per MD
step and site: the time of the bare launch / (chains * trajectories * n_md * V); it contains the momentum draw, the two
energy passes and the accept step of every trajectory.  The sampler calls also record every trajectory, compute log p of
the rows and read the statistics back.  The three are timed alternately, `--reps` times each; the figures are medians.

    python tools/hmc_bench.py [--reps 5] [--traj 50] [--composed-traj 5]
Prints one JSON line per shape and dtype.

    python tools/hmc_bench.py --measure [--reps 5] [--traj 50] [--composed-traj 5]
times `hmc.measure(...)` (the observables taken as the chain runs, no rows stored) against `model.measure(hmc.sample(...))`
(the rows stored, then measured) instead: 16^2 x 512 and 16^3 x 1024 chains in fp32 and fp64 (fused, `--traj` recorded
trajectories per call) and 32^4 x 16 chains in fp32 (tiled, `--composed-traj` per call).  Per shape: trajectories per
second of both (medians of `--reps` alternating calls, with the spread) and the rise of torch.cuda.max_memory_allocated
over one call of each.

    python tools/hmc_bench.py --integrator NAME [NAME ...] [--reps 5] [--traj 20] [--shapes small|large|all]
what the integration schemes ('leapfrog', 'omelyan', 'omf4') buy: on chains thermalised at the couplings above, at
trajectory length tau = n_md dt = 1, fp32, 16^3 x 1024 chains on the fused path (`--shapes small`) and 32^4 x 16 on the
tiled path (`--shapes large`), per scheme over a small scan of n_md: the bare call's time per force evaluation (a
trajectory of a scheme of s stages is n_md s of them), the acceptance and the rms dH of `--traj` trajectories from the
same start and Philox position; then the fewest force evaluations per trajectory in the scan that reach an acceptance of
0.8, and the trajectories per second there.  The configurations are timed alternately, `--reps` times each; medians."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("NORMFLOW_AMD_KEEP_TORCH_DEFAULTS", "1")
import torch  # noqa: E402

import normflow__amd as nf  # noqa: E402
from normflow__amd import _hip  # noqa: E402
from normflow__amd.prior import NormalPrior  # noqa: E402
from normflow__amd.action import ScalarPhi4Action  # noqa: E402

DEV = torch.device("cuda:0")
N_MD, DT = 10, 0.1
SHAPES = [((16, 16), 512), ((16, 16, 16), 1024)]
LARGE = [((32, 32, 32), 256), ((16, 16, 16, 16), 64), ((32, 32, 32, 32), 16), ((48, 48, 48, 48), 4)]


def _ms(f):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    f()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def measure(lattice, C, dtype, reps, n_traj, n_traj_composed):
    prior = NormalPrior(loc=torch.zeros(lattice, dtype=dtype, device=DEV), scale=torch.ones(lattice, dtype=dtype, device=DEV))
    model = nf.Model(net_=None, prior=prior, action=ScalarPhi4Action(kappa=0.67, m_sq=-2.68, lambd=0.5))
    s = model.hmc
    has_fused = _hip.hmc_supported(lattice, dtype)
    torch.manual_seed(0)
    s.start(n_chains=C)
    fused = lambda: s.sample(n_traj * C, n_chains=C, n_md=N_MD, dt=DT, path='fused')
    composed = lambda: s.sample(n_traj_composed * C, n_chains=C, n_md=N_MD, dt=DT, path='composed')
    coef = s._coef(lattice)
    kernel = lambda: _hip.phi4_hmc(s._ref['sample'].clone(), *coef, N_MD, DT, n_traj=n_traj)      # the launch alone, on a copy
    n_tiled = n_traj if has_fused else n_traj_composed
    tiled = lambda: s.sample(n_tiled * C, n_chains=C, n_md=N_MD, dt=DT, path='tiled')
    tiled_call = lambda: _hip.phi4_hmc_tiled(s._ref['sample'].clone(), *coef, N_MD, DT, n_traj=n_tiled)
    if not has_fused:
        fused = kernel = lambda: None
    with torch.no_grad():
        for _ in range(2):                      # warm-up: code objects, the allocator, and the chains thermalise
            fused()
            tiled()
            composed()
        kernel()
        tiled_call()
        torch.cuda.synchronize()
        # the paths against each other at the timed size: one trajectory from the same state and momenta
        phi0 = s._ref['sample'].clone()
        pi0 = torch.randn_like(phi0)
        one = {p: s.trajectory(phi0, N_MD, DT, pi=pi0, force_accept=True, path=p, position=(1, 0))
               for p in (['fused'] if has_fused else []) + ['tiled', 'composed']}
        dev = lambda a, b: ((a - b).abs().max() / b.abs().max()).item()
        check = dict(tiled_vs_composed_phi=dev(one['tiled']['phi'], one['composed']['phi']),
                     tiled_vs_composed_dh=(one['tiled']['dh'] - one['composed']['dh']).abs().max().item())
        if has_fused:
            check['tiled_vs_fused_phi'] = dev(one['tiled']['phi'], one['fused']['phi'])
        del one, phi0, pi0
        tf, tc, tk, tt, tb = [], [], [], [], []
        for _ in range(reps):                   # alternate them, so that a drift of the machine hits all
            tf.append(_ms(fused))
            tt.append(_ms(tiled))
            tc.append(_ms(composed))
            tk.append(_ms(kernel))
            tb.append(_ms(tiled_call))
    V = prior.nvar
    ms_t, ms_b = statistics.median(tt), statistics.median(tb)
    per_t = ms_t / n_tiled
    site_steps = C * n_tiled * N_MD * V
    extra = dict(tiled_traj_per_s=round(C / per_t * 1e3, 1), tiled_traj_per_call=n_tiled, tiled_ms_per_call=round(ms_t, 3),
                 tiled_ms_spread=[round(min(tt), 3), round(max(tt), 3)],
                 tiled_call_ms=round(ms_b, 3), tiled_call_ms_spread=[round(min(tb), 3), round(max(tb), 3)],
                 tiled_ns_per_md_step_site=round(ms_b * 1e6 / site_steps, 5),
                 tiled_algorithmic_TB_per_s=round((16 if dtype == torch.float32 else 32) * site_steps / (ms_b * 1e-3) / 1e12, 3),
                 tiled_plan=_hip.hmc_tiled_plan(lattice, dtype), check={k: float(f"{v:.2e}") for k, v in check.items()})
    if not has_fused:
        ms_c = statistics.median(tc)
        per_c = ms_c / n_traj_composed
        return dict(lattice=list(lattice), chains=C, dtype=str(dtype).replace("torch.", ""), n_md=N_MD, dt=DT,
                    composed_traj_per_s=round(C / per_c * 1e3, 1), tiled_over_composed=round(per_c / per_t, 2),
                    composed_ms_per_traj=round(per_c, 3),
                    composed_ms_spread=[round(min(tc) / n_traj_composed, 3), round(max(tc) / n_traj_composed, 3)],
                    accept_rate=round(s.history.accept_rate[-1], 3), **extra)
    ms_f, ms_c, ms_k = statistics.median(tf), statistics.median(tc), statistics.median(tk)
    per_f, per_c = ms_f / n_traj, ms_c / n_traj_composed          # ms per trajectory of all C chains
    return dict(lattice=list(lattice), chains=C, dtype=str(dtype).replace("torch.", ""), n_md=N_MD, dt=DT,
                fused_traj_per_s=round(C / per_f * 1e3, 1), composed_traj_per_s=round(C / per_c * 1e3, 1),
                fused_over_composed=round(per_c / per_f, 2),
                fused_ms_per_call=round(ms_f, 3), fused_traj_per_call=n_traj, fused_ms_spread=[round(min(tf), 3), round(max(tf), 3)],
                composed_ms_per_traj=round(per_c, 3), composed_ms_spread=[round(min(tc) / n_traj_composed, 3), round(max(tc) / n_traj_composed, 3)],
                kernel_ms_per_launch=round(ms_k, 3),
                fused_ns_per_md_step_site=round(ms_k * 1e6 / (C * n_traj * N_MD * V), 5),
                accept_rate=round(s.history.accept_rate[-3], 3), tiled_over_composed=round(per_c / per_t, 2), **extra)


MEASURE_SHAPES = [((16, 16), 512, torch.float32), ((16, 16), 512, torch.float64), ((16, 16, 16), 1024, torch.float32),
                  ((16, 16, 16), 1024, torch.float64), ((32, 32, 32, 32), 16, torch.float32)]


def measure_streaming(lattice, C, dtype, reps, n_traj):
    prior = NormalPrior(loc=torch.zeros(lattice, dtype=dtype, device=DEV), scale=torch.ones(lattice, dtype=dtype, device=DEV))
    model = nf.Model(net_=None, prior=prior, action=ScalarPhi4Action(kappa=0.67, m_sq=-2.68, lambd=0.5))
    s = model.hmc
    torch.manual_seed(0)
    s.start(n_chains=C)
    kw = dict(n_chains=C, n_md=N_MD, dt=DT)
    stream = lambda: s.measure(n_traj * C, **kw)
    store = lambda: model.measure(s.sample(n_traj * C, **kw))

    def peak(f):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(DEV)
        before = torch.cuda.memory_allocated(DEV)
        f()
        torch.cuda.synchronize()
        return (torch.cuda.max_memory_allocated(DEV) - before) / 2 ** 20
    with torch.no_grad():
        for _ in range(2):                      # warm-up: code objects, the allocator, and the chains thermalise
            stream()
            store()
        mem_stream, mem_store = peak(stream), peak(store)
        ts, tr = [], []
        for _ in range(reps):
            ts.append(_ms(stream))
            tr.append(_ms(store))
    ms_s, ms_r = statistics.median(ts), statistics.median(tr)
    rate = lambda ms: round(C * n_traj / ms * 1e3, 1)
    return dict(lattice=list(lattice), chains=C, dtype=str(dtype).replace("torch.", ""), n_md=N_MD, dt=DT,
                path=s._choose(s._ref['sample'], None), traj_per_call=n_traj,
                measure_traj_per_s=rate(ms_s), measure_traj_per_s_spread=[rate(max(ts)), rate(min(ts))],
                store_traj_per_s=rate(ms_r), store_traj_per_s_spread=[rate(max(tr)), rate(min(tr))],
                measure_over_store=round(ms_r / ms_s, 3),
                measure_peak_MiB=round(mem_stream, 2), store_peak_MiB=round(mem_store, 2),
                rows_MiB=round(n_traj * C * prior.nvar * torch.empty((), dtype=dtype).element_size() / 2 ** 20, 2),
                accept_rate=round(s.history.accept_rate[-1], 3))


INTEGRATOR_SHAPES = {'small': ((16, 16, 16), 1024, 'fused'), 'large': ((32, 32, 32, 32), 16, 'tiled')}
INTEGRATOR_SCAN = {1: (6, 8, 10, 12, 16, 24, 32, 48), 2: (3, 4, 5, 6, 8, 12, 16, 24), 5: (1, 2, 3, 4, 6)}      # n_md, by stages


def measure_integrators(names, lattice, C, path, reps, n_traj):
    dtype = torch.float32
    prior = NormalPrior(loc=torch.zeros(lattice, dtype=dtype, device=DEV), scale=torch.ones(lattice, dtype=dtype, device=DEV))
    model = nf.Model(net_=None, prior=prior, action=ScalarPhi4Action(kappa=0.67, m_sq=-2.68, lambd=0.5))
    s = model.hmc
    torch.manual_seed(0)
    s.start(n_chains=C)
    coef = s._coef(lattice)
    kernel = _hip.phi4_hmc if path == 'fused' else _hip.phi4_hmc_tiled
    ws = dict(workspace=s._tiled_workspace(s._ref['sample'])) if path == 'tiled' else {}
    with torch.no_grad():
        s.sample(40 * C, n_chains=C, n_md=16, dt=1.0 / 16, path=path)           # thermalise: 40 trajectories of tau = 1
        start = s._ref['sample'].clone()
        configs = []
        for name in names:
            scheme = _hip.hmc_scheme(name)
            for n_md in INTEGRATOR_SCAN.get(scheme.stages, INTEGRATOR_SCAN[2]):
                kw = dict(ws) if name == 'leapfrog' else dict(ws, scheme=scheme)      # leapfrog: the entry point as it always was
                configs.append(dict(name=name, stages=scheme.stages, n_md=n_md, times=[], run=(
                    lambda n_md=n_md, kw=kw: kernel(start.clone(), *coef, n_md, 1.0 / n_md, n_traj=n_traj, position=(1, 0), **kw))))
        for c in configs:                           # warm-up, and the statistics: every configuration from the same start
            r = c['run']()
            c['accept'] = r['accept'].float().mean().item()
            c['dh_rms'] = r['dh'].double().square().mean().sqrt().item()
        torch.cuda.synchronize()
        for _ in range(reps):                       # alternate them, so that a drift of the machine hits all
            for c in configs:
                c['times'].append(_ms(c['run']))
    V = prior.nvar
    out = dict(lattice=list(lattice), chains=C, dtype="float32", path=path, tau=1.0, traj_per_call=n_traj, schemes={})
    for name in names:
        rows, best = [], None
        for c in (c for c in configs if c['name'] == name):
            ms = statistics.median(c['times'])
            evals = c['n_md'] * c['stages']
            row = dict(n_md=c['n_md'], force_evals=evals, us_per_force_eval=round(ms * 1e3 / (n_traj * evals), 3),
                       ns_per_force_eval_site=round(ms * 1e6 / (n_traj * evals * C * V), 5),
                       ms_spread=[round(min(c['times']), 3), round(max(c['times']), 3)], ms_per_call=round(ms, 3),
                       accept=round(c['accept'], 3), dh_rms=float(f"{c['dh_rms']:.3e}"),
                       traj_per_s=round(C * n_traj / ms * 1e3, 1))
            rows.append(row)
            if row['accept'] >= 0.8 and (best is None or evals < best['force_evals']):
                best = row
        out['schemes'][name] = dict(scan=rows, fewest_force_evals_at_accept_0p8=None if best is None else best['force_evals'],
                                    n_md_there=None if best is None else best['n_md'],
                                    traj_per_s_there=None if best is None else best['traj_per_s'])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--traj", type=int, default=50, help="trajectories per fused call (one launch)")
    ap.add_argument("--composed-traj", type=int, default=5, help="trajectories per composed call")
    ap.add_argument("--shapes", choices=("all", "small", "large"), default="all")
    ap.add_argument("--measure", action="store_true", help="hmc.measure against measure(hmc.sample()) (module docstring)")
    ap.add_argument("--integrator", nargs="+", metavar="NAME", choices=sorted(_hip.HMC_SCHEMES),
                    help="what the integration schemes buy at tau = 1 (module docstring)")
    a = ap.parse_args()
    if a.integrator:
        for key in ('small', 'large'):
            if a.shapes in ('all', key):
                lattice, C, path = INTEGRATOR_SHAPES[key]
                print(json.dumps(measure_integrators(a.integrator, lattice, C, path, a.reps, min(a.traj, 20))), flush=True)
        return
    if a.measure:
        for lattice, C, dtype in MEASURE_SHAPES:
            n = a.traj if _hip.hmc_supported(lattice, dtype) else a.composed_traj
            print(json.dumps(measure_streaming(lattice, C, dtype, a.reps, n)), flush=True)
        return
    shapes = (SHAPES if a.shapes != "large" else []) + (LARGE if a.shapes != "small" else [])
    for lattice, C in shapes:
        for dtype in (torch.float32, torch.float64):
            print(json.dumps(measure(lattice, C, dtype, a.reps, a.traj, a.composed_traj)), flush=True)


if __name__ == "__main__":
    main()

"""What the coupling ladder costs and what it buys, on one GPU in one run (HIP events after a warm-up, no_grad; medians
of `--reps` alternating calls, with the spread):
  (a) a ladder launch (nf_phi4_hmc_ladder, 32 rungs) against nf_phi4_hmc of the same build at the same C, lattice and
      n_md: 16^2 x 512 chains and 16^3 x 1024 chains, fp32 and fp64, `--traj` trajectories in one launch, on copies of the
      same thermalised chains.  The ladder's rungs all carry the couplings of the uniform launch, so both do the same
      arithmetic: the difference is the lookup.  `slower` says whether the ladder's median is above nf_phi4_hmc's by more
      than the larger of 10 % and the run-to-run spread of the two.
  (b) one exchange cycle -- the chains' measure rows (nf_lattice_measure) and the sweep (nf_phi4_ladder_exchange) -- in
      units of an MD step of that launch (the launch's time / (trajectories n_md)).
  (c) tau_int of the magnetisation on the lowest rung of a broken-phase ladder ((8, 8), m_sq = -2.68, lambd = 0.5, kappa
      from 0.67 down to 0.25 in 8 rungs, 32 replica sets), with exchange_every = 1 against 0, from `--steps` recorded
      steps after as many of thermalisation.

    python tools/hmc_ladder_bench.py [--reps 5] [--traj 50] [--steps 2000]
Prints one JSON line per shape and dtype, then one for (c)."""
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
from normflow__amd.action import ScalarPhi4Action, ScalarPhi4Ladder  # noqa: E402
from normflow__amd.lib.observables import Ensemble  # noqa: E402

DEV = torch.device("cuda:0")
N_MD, DT, K = 10, 0.1, 32
COUPLINGS = dict(kappa=0.67, m_sq=-2.68, lambd=0.5)
SHAPES = [((16, 16), 512), ((16, 16, 16), 1024)]


def _ms(f):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    f()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def _model(lattice, dtype, **couplings):
    prior = NormalPrior(loc=torch.zeros(lattice, dtype=dtype, device=DEV), scale=torch.ones(lattice, dtype=dtype, device=DEV))
    return nf.Model(net_=None, prior=prior, action=ScalarPhi4Action(**couplings))


def launches(lattice, C, dtype, reps, n_traj):
    model = _model(lattice, dtype, **COUPLINGS)
    s = model.hmc
    torch.manual_seed(0)
    s.start(n_chains=C)
    with torch.no_grad():
        s.sample(20 * C, n_chains=C, n_md=N_MD, dt=DT)            # thermalise
        phi0 = s._ref['sample'].clone()
        w = s._coef(lattice)
        ladder = ScalarPhi4Ladder(**{k: [v] * K for k, v in COUPLINGS.items()})
        coef = ladder.coef_table(lattice, DEV)
        g = torch.Generator(device="cpu").manual_seed(1)
        rung = torch.cat([torch.randperm(K, generator=g, device="cpu") for _ in range(C // K)]).to(device=DEV, dtype=torch.int32)
        pos = (7, 0)
        uniform = lambda: _hip.phi4_hmc(phi0.clone(), *w, N_MD, DT, n_traj=n_traj, position=pos)
        laddered = lambda: _hip.phi4_hmc_ladder(phi0.clone(), coef, rung, N_MD, DT, n_traj=n_traj, position=pos)
        rows = _hip.lattice_measure(phi0)
        action = torch.zeros(C, dtype=torch.float64, device=DEV)

        def cycle():
            r = _hip.lattice_measure(phi0, out=rows)
            _hip.ladder_exchange(r, coef, rung.clone(), 0, action=action, position=pos)
        a, b = uniform(), laddered()
        same = torch.equal(a['action'], b['action'])              # identical rungs: the same bits per chain
        cycle()
        torch.cuda.synchronize()
        tu, tl, tx = [], [], []
        for _ in range(reps):
            tu.append(_ms(uniform))
            tl.append(_ms(laddered))
            tx.append(_ms(cycle))
    mu, ml, mx = statistics.median(tu), statistics.median(tl), statistics.median(tx)
    spread = max(max(tu) - min(tu), max(tl) - min(tl)) / mu
    margin = max(0.10, spread)
    md_step = ml / (n_traj * N_MD)
    return dict(lattice=list(lattice), chains=C, rungs=K, dtype=str(dtype).replace("torch.", ""), n_md=N_MD, traj_per_launch=n_traj,
                uniform_ms=round(mu, 3), uniform_ms_spread=[round(min(tu), 3), round(max(tu), 3)],
                ladder_ms=round(ml, 3), ladder_ms_spread=[round(min(tl), 3), round(max(tl), 3)],
                ladder_over_uniform=round(ml / mu, 4), margin=round(margin, 4), slower=bool(ml / mu > 1 + margin),
                ladder_traj_per_s=round(C * n_traj / ml * 1e3, 1), same_bits_as_uniform=same,
                exchange_cycle_ms=round(mx, 4), exchange_cycle_ms_spread=[round(min(tx), 4), round(max(tx), 4)],
                us_per_md_step=round(md_step * 1e3, 3), exchange_cycle_in_md_steps=round(mx / md_step, 2))


def tunnelling(steps):
    lattice, rungs, R = (8, 8), 8, 32
    kappas = [0.67 - (0.67 - 0.25) * k / (rungs - 1) for k in range(rungs)]
    ladder = ScalarPhi4Ladder(kappa=kappas, m_sq=COUPLINGS['m_sq'], lambd=COUPLINGS['lambd'])
    model = _model(lattice, torch.float32, **COUPLINGS)
    out = dict(lattice=list(lattice), rungs=rungs, replica_sets=R, kappa=[round(k, 4) for k in kappas], steps=steps)
    for every in (0, 1):
        s = model.hmc.ladder(ladder)
        torch.manual_seed(3)
        s.start(n_chains=rungs * R)
        kw = dict(n_chains=rungs * R, n_md=N_MD, dt=DT, exchange_every=every)
        with torch.no_grad():
            s.measure(steps * rungs * R, **kw)                    # thermalise
            ms = s.measure(steps * rungs * R, **kw)
        e = Ensemble(ms[0], n_chains=R)
        tau = e.tau_int('magnetization')
        absm = ms[0].magnetization().abs().mean().item()
        key = f"exchange_every_{every}"
        out[key] = dict(tau_int_m=[round(float(v), 2) for v in (tau if isinstance(tau, (tuple, list)) else (tau,))],
                        mean_abs_m=round(absm, 4), accept_rate=round(s.history.accept_rate[-1], 3),
                        exchange_rate=[None if r != r else round(r, 3) for r in s.history.exchange_rate[-1]])
    return out


CLUSTER_SHAPES = SHAPES + [((32, 32, 32), 256)]         # the last is beyond nf_phi4_cluster: the tiled kernels


def sweeps(lattice, C, dtype, reps, inner):
    """The ladder sweep (32 rungs, all with the couplings of the plain sweep: the same arithmetic, the difference is the
    lookup) against the plain sweep of the same build on the same thermalised chains, `inner` sweeps in a row per timing."""
    model = _model(lattice, dtype, **COUPLINGS)
    s = model.hmc
    tiled = not _hip.cluster_supported(lattice, dtype)
    torch.manual_seed(0)
    s.start(n_chains=C)
    with torch.no_grad():
        s.measure(20 * C, n_chains=C, n_md=N_MD, dt=DT, cluster_every=1)        # thermalise, sweeps included; no rows
        phi0 = s._ref['sample'].clone()
        w0 = float(model.action.get_coef(len(lattice))[0])
        ladder = ScalarPhi4Ladder(**{k: [v] * K for k, v in COUPLINGS.items()})
        coef = ladder.coef_table(lattice, DEV)
        g = torch.Generator(device="cpu").manual_seed(1)
        rung = torch.cat([torch.randperm(K, generator=g, device="cpu") for _ in range(C // K)]).to(device=DEV, dtype=torch.int32)
        kw = dict(workspace=torch.empty(_hip.cluster_tiled_workspace(C, lattice), dtype=torch.uint8, device=DEV)) if tiled else {}
        plain_k = _hip.phi4_cluster_tiled if tiled else _hip.phi4_cluster
        ladder_k = _hip.phi4_cluster_tiled_ladder if tiled else _hip.phi4_cluster_ladder
        a, b = phi0.clone(), phi0.clone()
        ra = plain_k(a, w0, position=(7, 0), want_labels=True, **kw)
        rb = ladder_k(b, coef, rung, position=(7, 0), want_labels=True, **kw)
        same = bool(torch.equal(a, b) and torch.equal(ra['labels'], rb['labels']))
        work = phi0.clone()

        def plain():
            for _ in range(inner):
                plain_k(work, w0, **kw)

        def laddered():
            for _ in range(inner):
                ladder_k(work, coef, rung, **kw)
        for _ in range(2):
            plain(); laddered()
        torch.cuda.synchronize()
        tp, tl = [], []
        for rep in range(reps):                                   # alternately, and who goes first alternates too
            for f, t in ((plain, tp), (laddered, tl))[::1 if rep % 2 == 0 else -1]:
                t.append(_ms(f) / inner)
    mp, ml = statistics.median(tp), statistics.median(tl)
    spread = max((max(t) - min(t)) / statistics.median(t) for t in (tp, tl))
    margin = max(0.10, spread)
    rnd = lambda t: [round(min(t), 4), round(max(t), 4)]
    return dict(lattice=list(lattice), chains=C, rungs=K, dtype=str(dtype).replace("torch.", ""),
                kernel="nf_phi4_cluster_tiled" if tiled else "nf_phi4_cluster", sweeps_per_timing=inner,
                plain_ms=round(mp, 4), plain_ms_spread=rnd(tp), ladder_ms=round(ml, 4), ladder_ms_spread=rnd(tl),
                ladder_over_plain=round(ml / mp, 4), spread=round(spread, 4), margin=round(margin, 4),
                slower=bool(ml / mp > 1 + margin), same_bits_as_plain=same)


def tunnelling_per_rung(steps):
    """tau_int of the magnetisation on every rung of (c)'s ladder with exchanges, with cluster sweeps, and with both."""
    lattice, rungs, R = (8, 8), 8, 32
    kappas = [0.67 - (0.67 - 0.25) * k / (rungs - 1) for k in range(rungs)]
    ladder = ScalarPhi4Ladder(kappa=kappas, m_sq=COUPLINGS['m_sq'], lambd=COUPLINGS['lambd'])
    model = _model(lattice, torch.float32, **COUPLINGS)
    out = dict(lattice=list(lattice), rungs=rungs, replica_sets=R, kappa=[round(k, 4) for k in kappas], steps=steps)
    for name, ee, ec in (("exchanges", 1, 0), ("sweeps", 0, 1), ("both", 1, 1)):
        s = model.hmc.ladder(ladder)
        torch.manual_seed(3)
        s.start(n_chains=rungs * R)
        kw = dict(n_chains=rungs * R, n_md=N_MD, dt=DT, exchange_every=ee, cluster_every=ec)
        with torch.no_grad():
            s.measure(steps * rungs * R, **kw)                    # thermalise
            ms = s.measure(steps * rungs * R, **kw)
        taus = [Ensemble(m, n_chains=R).tau_int('magnetization') for m in ms]
        out[name] = dict(tau_int_m=[round(float(t[0] if isinstance(t, (tuple, list)) else t), 2) for t in taus],
                         tau_int_m_err=[round(float(t[1]), 2) if isinstance(t, (tuple, list)) and len(t) > 1 else None for t in taus],
                         mean_abs_m=[round(m.magnetization().abs().mean().item(), 4) for m in ms],
                         accept_rate=round(s.history.accept_rate[-1], 3),
                         exchange_rate=[None if r != r else round(r, 3) for r in s.history.exchange_rate[-1]])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--traj", type=int, default=50, help="trajectories per launch")
    ap.add_argument("--steps", type=int, default=2000, help="recorded steps of the tunnelling run (and of its thermalisation)")
    ap.add_argument("--skip-tunnelling", action="store_true")
    ap.add_argument("--cluster", action="store_true",
                    help="instead: the ladder cluster sweeps against the plain ones, and tau_int per rung with exchanges, sweeps, both")
    ap.add_argument("--inner", type=int, default=20, help="--cluster: sweeps per timing")
    a = ap.parse_args()
    if a.cluster:
        for lattice, C in CLUSTER_SHAPES:
            for dtype in (torch.float32, torch.float64):
                print(json.dumps(sweeps(lattice, C, dtype, a.reps, a.inner)), flush=True)
        if not a.skip_tunnelling:
            print(json.dumps(tunnelling_per_rung(a.steps)), flush=True)
        return
    for lattice, C in SHAPES:
        for dtype in (torch.float32, torch.float64):
            print(json.dumps(launches(lattice, C, dtype, a.reps, a.traj)), flush=True)
    if not a.skip_tunnelling:
        print(json.dumps(tunnelling(a.steps)), flush=True)


if __name__ == "__main__":
    main()

"""What Fourier acceleration costs and buys on one GPU (HIP events after a warm-up, no_grad).  It decides nothing:
acceleration is opt-in whatever comes out, and no default or route depends on these figures.  The expectation, stated
beforehand: per force evaluation the accelerated kernel is slower (a filter of 2 d axis passes on the matrix cores
against one stencil pass), and its integrated autocorrelation times are lower in the symmetric phase.

(a) the bare launch: microseconds per force evaluation of nf_phi4_hmc_fa against nf_phi4_hmc of the same build, leapfrog,
    n_md = 10, `--traj` trajectories per launch, on 16^2 x 512 and 16^3 x 1024 chains in fp32 and fp64; the two launches
    are timed alternately `--reps` times, the figures are medians with [min, max].  `ratio` is one accelerated force
    evaluation in MD steps of nf_phi4_hmc: what NF_HMC_FA_MD_STEPS stands for (include/normflow_hip.h).
(b) `--tau`: what it buys.  (16, 16) and (16, 16, 16) at the couplings given (`--kappa --m-sq --lambd`; the defaults lie
    in the symmetric phase near the transition), fp32, `--chains` chains: each sampler at n_md = 10 and its own dt, the
    largest of a small scan with an acceptance of at least 0.8; then `--tau` recorded trajectories after as many dropped,
    and tau_int of V m^2 and of phi^2 (the sum of the chain-averaged autocorrelation function up to the first lag where
    it drops below its own noise, chains as replicas) in trajectories and, times the launch's time per trajectory,
    in milliseconds of one chain set per independent sample.

    python tools/hmc_fa_bench.py --fourier M2 [--reps 7] [--traj 20] [--tau 0]
Prints one JSON line per shape and dtype (a) and per shape and sampler (b)."""
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
N_MD = 10
SHAPES = [((16, 16), 512), ((16, 16, 16), 1024)]


def _ms(f):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    f()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def _model(lattice, dtype, couplings):
    prior = NormalPrior(loc=torch.zeros(lattice, dtype=dtype, device=DEV), scale=torch.ones(lattice, dtype=dtype, device=DEV))
    return nf.Model(net_=None, prior=prior, action=ScalarPhi4Action(**couplings))


def _spread(ts, scale):
    return [round(statistics.median(ts) * scale, 4), round(min(ts) * scale, 4), round(max(ts) * scale, 4)]


def bare(lattice, C, dtype, mass_sq, reps, n_traj, couplings):
    s = _model(lattice, dtype, couplings).hmc
    torch.manual_seed(0)
    s.start(n_chains=C)
    s.sample(20 * C, n_chains=C, n_md=N_MD, dt=0.1)                       # thermalise
    phi0, coef = s._ref['sample'], s._coef(lattice)
    plain = lambda: _hip.phi4_hmc(phi0.clone(), *coef, N_MD, 0.1, n_traj=n_traj)
    fa = lambda: _hip.phi4_hmc_fa(phi0.clone(), *coef, N_MD, 0.1, mass_sq, n_traj=n_traj)
    for _ in range(2):
        plain()
        fa()
    torch.cuda.synchronize()
    tp, tf = [], []
    for _ in range(reps):                                                  # alternate: a drift of the machine hits both
        tp.append(_ms(plain))
        tf.append(_ms(fa))
    per_eval = 1e3 / (n_traj * N_MD)                                       # ms per launch -> us per force evaluation
    out = dict(part="bare", lattice=list(lattice), chains=C, dtype=str(dtype).replace("torch.", ""), n_md=N_MD,
               traj_per_launch=n_traj, reps=reps, fa_mass_sq=mass_sq,
               plain_us_per_eval=_spread(tp, per_eval), fa_us_per_eval=_spread(tf, per_eval),
               ratio=round(statistics.median(tf) / statistics.median(tp), 3),
               ratio_min_max=[round(min(tf) / max(tp), 3), round(max(tf) / min(tp), 3)], plan=_hip.hmc_fa_plan(lattice, dtype, N_MD))
    print(json.dumps(out), flush=True)


def tau_int(x):
    """(tau_int, its window) of the series x (T, C), C chains as replicas: 1/2 + sum of rho(t) up to the first lag at
    which rho drops below 2 sigma of its own noise sqrt(1 / (T C))."""
    x = x.double() - x.double().mean()
    T, C = x.shape
    var = x.square().mean()
    tau, noise = 0.5, 2.0 / (T * C) ** 0.5
    for t in range(1, T // 2):
        rho = ((x[t:] * x[:-t]).mean() / var).item()
        if rho < noise:
            return tau, t
        tau += rho
    return tau, T // 2


def autocorrelation(lattice, C, mass_sq, n_rec, couplings):
    V = 1
    for n in lattice:
        V *= n
    for name, kw in (("plain", {}), ("fa", dict(fa_mass_sq=mass_sq))):
        s = _model(lattice, torch.float32, couplings).hmc
        torch.manual_seed(1)
        s.start(n_chains=C)
        s.sample(C, n_chains=C, n_md=N_MD, dt=0.05, n_skip=99, **kw)     # thermalise
        best = None
        for dt in (0.05, 0.075, 0.1, 0.15, 0.2, 0.3, 0.4):
            s.sample(C, n_chains=C, n_md=N_MD, dt=dt, n_skip=9, **kw)
            acc = s.history.accept_rate[-1]
            if acc >= 0.8:
                best = (dt, acc)
        dt, acc = best if best is not None else (0.05, s.history.accept_rate[-1])
        s.sample(C, n_chains=C, n_md=N_MD, dt=dt, n_skip=n_rec - 1, **kw)
        t0 = _ms(lambda: s.sample(C, n_chains=C, n_md=N_MD, dt=dt, n_skip=19, **kw)) / 20
        y = s.sample(n_rec * C, n_chains=C, n_md=N_MD, dt=dt, **kw).reshape(n_rec, C, V)
        acc = s.history.accept_rate[-1]
        out = dict(part="tau", sampler=name, lattice=list(lattice), chains=C, n_md=N_MD, dt=dt, accept=round(acc, 3),
                   trajectories=n_rec, ms_per_trajectory=round(t0, 4), fa_mass_sq=mass_sq if kw else None, **couplings)
        for key, series in (("m2V", y.mean(dim=2).square() * V), ("phi2", y.square().mean(dim=2))):
            tau, window = tau_int(series)
            out["tau_int_" + key] = round(tau, 2)
            out["window_" + key] = window
            out["ms_per_independent_" + key] = round(2 * tau * t0, 3)
        print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fourier", type=float, required=True, metavar="M2", help="fa_mass_sq of the accelerated runs")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--traj", type=int, default=20)
    ap.add_argument("--tau", type=int, default=0, help="recorded trajectories of part (b); 0: part (a) only")
    ap.add_argument("--chains", type=int, default=256)
    ap.add_argument("--kappa", type=float, default=1.0)
    ap.add_argument("--m-sq", type=float, default=-1.2)
    ap.add_argument("--lambd", type=float, default=0.5)
    args = ap.parse_args()
    couplings = dict(kappa=args.kappa, m_sq=args.m_sq, lambd=args.lambd)
    with torch.no_grad():
        for lattice, C in SHAPES:
            for dtype in (torch.float32, torch.float64):
                bare(lattice, C, dtype, args.fourier, args.reps, args.traj, couplings)
        if args.tau:
            for lattice, _ in SHAPES:
                autocorrelation(lattice, args.chains, args.fourier, args.tau, couplings)


if __name__ == "__main__":
    main()

"""What a cluster sweep costs and what it buys, on one GPU, in one run (HIP events after a warm-up, no_grad):
  (a) the bare sweep, nf_phi4_cluster, against ONE trajectory (n_md = 10) of nf_phi4_hmc of the same build on the same
      chains: what `cluster_every=1` adds to a recorded step.  Both as launches alone, `--inner` in a row per timing (the
      sweep in place on a copy of the chains: a swept state is as good a state; the trajectories inside one launch);
  (b) the kernel against the composed sweep on the device (nf_phi4_cluster_draws + `cluster_sweep`, mcmc/cluster.py,
      which reads one flag per round), per sweep.  The sampler routes to the kernel only where it wins by more than the
      margin: the larger of 10 % and the run's spread;
  on thermalised chains of 16^2 x 512 and 16^3 x 1024, fp32 and fp64, timed alternately `--reps` times: medians and the
  spread.
  (c) tau_int of the magnetisation of an (8, 8) lattice in the broken phase (kappa = 0.67, m_sq = -2.68, lambd = 0.5, 32
      chains, `--steps` recorded steps after as many of thermalisation, fp32) with cluster_every = 0 and 1, and the mean
      fraction of the lattice in the largest cluster.

  --tiled: instead of (a) .. (c), nf_phi4_cluster_tiled on the lattices beyond nf_phi4_cluster -- 32^3 x 256, 16^4 x 64,
      32^4 x 16, 48^4 x 4, fp32 and fp64, thermalised by 20 steps of tiled sweep + tiled trajectory -- at tile_sites 4096,
      8192 and 16384: the sweep (`--inner` in a row per timing, one workspace) against the composed sweep of the same build
      on the same chains and against one trajectory (n_md = 10) of nf_phi4_hmc_tiled, with the same margin rule; the share
      of the active-or-not forward links that cross tiles; and the tiled sweep against nf_phi4_cluster at 16^3 x 1024,
      where both apply.  The ratios and the verdict are those of the library's default tile.

  --improved: instead of (a) .. (c), the cluster-improved estimators: the bare nf_cluster_moments against nf_phi4_cluster of the same build on the same thermalised
      chains and against the composed path (`mcmc.cluster.cluster_moments`) on the device; 16^2 x 512 and 16^3 x 1024, fp32
      and fp64, at kappa = 0.67 (one giant cluster) and kappa = 0.25 (many small ones): the two contention regimes;
      `hmc.measure(cluster_every=1, improved=True)` against `improved=False`; and the variance of (sum phi)^2 and of
      |phi~(p_min)|^2 over that of their improved forms on (8, 8) x 32 chains (`--steps` recorded steps after 200).

  --improved-tiled: instead of (a) .. (c), nf_cluster_moments_tiled on the lattices beyond nf_cluster_moments -- 32^3 x 256,
      16^4 x 64, 32^4 x 16, 48^4 x 4, fp32 and fp64, thermalised at kappa = 0.67 and 0.25 -- at block_sites 2048, 4096 and
      8192: the bare call against the composed path on the device (what runs there without the kernel), against one sweep
      of nf_phi4_cluster_tiled, and against nf_cluster_moments at 16^3 x 1024, where both apply; one
      `hmc.measure(cluster_every=1, improved='hbm')` step against improved='composed'; peak memory of one call of each
      path.  `--shapes 0,1` picks shapes by index (0 is 16^3 x 1024).  The ratios and the verdict are those of the default
      block.

  --spectrum: instead of (a) .. (c), nf_cluster_spectrum on thermalised chains of 16^2 x 512 and 16^3 x 1024, fp32 and
      fp64, at kappa = 0.67 and 0.25, with momenta 1, 2, 4 and all: the bare call against nf_cluster_moments (momenta 1
      must be within the margin of it), against the composed path (`mcmc.cluster.cluster_spectrum`) on the device, and
      against one sweep plus one trajectory (n_md = 10); medians of alternating timings with [min, max], the margin the
      larger of 10 % and the run's spread.  Then the row variance of sum_s S(s) S(s + t) over that of its improved form on
      (8, 8) x 32 chains at kappa = 0.25 and 0.45, fp64 (`--steps` recorded steps after 100).

  --spectrum-tiled: instead of (a) .. (c), nf_cluster_spectrum_tiled on the lattices beyond nf_cluster_spectrum -- 32^3 x 256,
      16^4 x 64, 32^4 x 16, 48^4 x 4 (and 16^3 x 1024, where nf_cluster_spectrum applies too), thermalised as for
      --improved-tiled at kappa = 0.67 and 0.25 -- at momenta 1, 2, 4 and all: against the composed path on the device (at
      momenta 1 and 4: at 'all' it is too slow and too large to repeat), against nf_cluster_moments_tiled at momenta 1,
      against nf_cluster_spectrum at 16^3 x 1024, per quantity against one tiled sweep plus one tiled trajectory, at
      per_pass 4, 8, 16 and block_sites 2048, 4096, 8192, and the peak memory of one call; medians of at least 5
      alternating timings with [min, max].  `--shapes`, `--dtypes`, `--kappas` pick a part of the run.

  --modes: instead of (a) .. (c), nf_cluster_modes on the chains and at the conditions of --spectrum (16^2 x 512 and
      16^3 x 1024, fp32 and fp64, thermalised at kappa = 0.67 and 0.25): the bare call at the ON-AXIS momenta of
      `momenta` 1, 2, 4 and all, given as a list, against nf_cluster_spectrum of the same build with the same Q (the
      expectation: equal per quantity, within the larger of 10 % and the run's spread), and against the composed path
      (`mcmc.cluster.cluster_modes`) on the device, which decides what `measure_modes(path=None)` takes; then the same at
      a list of 16 generic off-axis momenta, against the composed path; medians of alternating timings with [min, max].

  --modes-tiled: instead of (a) .. (c), nf_cluster_modes_tiled on the chains and at the conditions of --spectrum-tiled
      (32^3 x 256, 16^4 x 64, 32^4 x 16, 48^4 x 4 and 16^3 x 1024, thermalised at kappa = 0.67 and 0.25): against the composed
      path (`mcmc.cluster.cluster_modes`) on the device at 3 generic momenta, a list length it can repeat on every class;
      with the on-axis momenta of `momenta` 1, 2, 4 given as a list against nf_cluster_spectrum_tiled of the same build at
      the same Q; against nf_cluster_modes at 16^3 x 1024; per quantity; at per_pass 4, 8, 16 and block_sites 2048, 4096,
      8192 with 16 generic momenta; and the peak memory of one call; medians of at least 5 alternating timings with
      [min, max].  `--shapes`, `--dtypes`, `--kappas` pick a part of the run.

    python tools/cluster_bench.py [--reps 5] [--inner 20] [--steps 1500] [--skip-tau]
                                  [--tiled | --improved | --improved-tiled | --spectrum | --spectrum-tiled | --modes |
                                   --modes-tiled]
Prints one JSON line per shape and dtype and one for (c)."""
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
from normflow__amd.action import ScalarPhi4Action  # noqa: E402
from normflow__amd.lib import Ensemble  # noqa: E402
from normflow__amd.mcmc.cluster import cluster_sweep  # noqa: E402
from normflow__amd.prior import NormalPrior  # noqa: E402

DEV = torch.device("cuda:0")
N_MD, DT = 10, 0.1
COUPLINGS = dict(kappa=0.67, m_sq=-2.68, lambd=0.5)
SHAPES = [((16, 16), 512), ((16, 16, 16), 1024)]


def _ms(f):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    f()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def _model(lattice, dtype):
    prior = NormalPrior(loc=torch.zeros(lattice, dtype=dtype, device=DEV), scale=torch.ones(lattice, dtype=dtype, device=DEV))
    return nf.Model(net_=None, prior=prior, action=ScalarPhi4Action(**COUPLINGS))


def launches(lattice, C, dtype, reps, inner):
    model = _model(lattice, dtype)
    s = model.hmc
    torch.manual_seed(0)
    s.start(n_chains=C)
    with torch.no_grad():
        s.measure(30 * C, n_chains=C, n_md=N_MD, dt=DT, cluster_every=1)             # thermalise, sweeps included; no rows
        phi = s._ref['sample'].clone()
        coef, w0 = s._coef(lattice), float(model.action.get_coef(len(lattice))[0])
        work = phi.clone()

        def sweep():
            for _ in range(inner):
                _hip.phi4_cluster(work, w0)

        def composed():
            u, flip = _hip.phi4_cluster_draws(C, lattice, DEV)
            return cluster_sweep(work, w0, u, flip)

        traj = lambda: _hip.phi4_hmc(work, *coef, N_MD, DT, n_traj=inner)
        for _ in range(2):
            sweep(); traj(); composed()
        torch.cuda.synchronize()
        # the two sweeps against each other at the timed size, from one position
        k = phi.clone()
        r = _hip.phi4_cluster(k, w0, position=(1, 0), want_labels=True)
        c = cluster_sweep(phi, w0, *_hip.phi4_cluster_draws(C, lattice, DEV, position=(1, 0)))
        same = bool(torch.equal(c[0], k) and torch.equal(c[1], r['labels']))
        stats = r['stats'].double()
        ts, tt, tc = [], [], []
        for _ in range(reps):
            ts.append(_ms(sweep) / inner)
            tt.append(_ms(traj) / inner)
            tc.append(_ms(composed))
    ms, mt, mc = statistics.median(ts), statistics.median(tt), statistics.median(tc)
    spread = max((max(t) - min(t)) / statistics.median(t) for t in (ts, tt, tc))
    margin = max(0.10, spread)
    rnd = lambda t: [round(min(t), 4), round(max(t), 4)]
    return dict(lattice=list(lattice), chains=C, dtype=str(dtype).replace("torch.", ""), n_md=N_MD, launches_per_timing=inner,
                sweep_ms=round(ms, 4), sweep_ms_spread=rnd(ts), trajectory_ms=round(mt, 4), trajectory_ms_spread=rnd(tt),
                sweep_over_trajectory=round(ms / mt, 3), composed_ms=round(mc, 3), composed_ms_spread=rnd(tc),
                composed_over_kernel=round(mc / ms, 1), margin=round(margin, 3), kernel_wins=bool(mc / ms > 1 + margin),
                same_bits_as_composed=same, plan=_hip.cluster_plan(lattice, dtype),
                mean_clusters=round(stats[:, 0].mean().item(), 1), mean_largest_fraction=round(stats[:, 2].mean().item() / phi[0].numel(), 4),
                max_rounds=int(stats[:, 3].max().item()), composed_rounds=int(c[2][0, 3].item()))


TILED_SHAPES = [((32, 32, 32), 256), ((16, 16, 16, 16), 64), ((32, 32, 32, 32), 16), ((48, 48, 48, 48), 4)]
TILES = (4096, 8192, 16384)


def crossing_share(lattice, tile_sites):
    """The share of the forward links (x, mu) whose ends lie in different tiles (runs of tile_sites site indices)."""
    V = 1
    for n in lattice:
        V *= n
    x = torch.arange(V, device=DEV).reshape(lattice)
    cross = sum(((x // tile_sites) != (torch.roll(x, -1, dims=a) // tile_sites)).sum().item() for a in range(len(lattice)))
    return cross / (V * len(lattice))


def tiled(lattice, C, dtype, reps, inner, both=False):
    """`both`: a lattice nf_phi4_cluster takes too -- the tiled sweep against it instead of against the composed sweep."""
    model = _model(lattice, dtype)
    s = model.hmc
    torch.manual_seed(0)
    s.start(n_chains=C)
    with torch.no_grad():
        phi = s._ref['sample'].clone()
        coef, w0 = s._coef(lattice), float(model.action.get_coef(len(lattice))[0])
        ws = torch.empty(_hip.cluster_tiled_workspace(C, lattice), dtype=torch.uint8, device=DEV)
        hmc = _hip.phi4_hmc if both else _hip.phi4_hmc_tiled
        for _ in range(20):                                                          # thermalise, sweeps included
            _hip.phi4_cluster_tiled(phi, w0, workspace=ws)
            hmc(phi, *coef, N_MD, DT, n_traj=1)
        work = phi.clone()

        def sweep(tile):
            def f():
                for _ in range(inner):
                    _hip.phi4_cluster_tiled(work, w0, tile_sites=tile, workspace=ws)
            return f

        def other():
            if both:
                for _ in range(inner):
                    _hip.phi4_cluster(work, w0)
                return None
            u, flip = _hip.phi4_cluster_draws(C, lattice, DEV)
            return cluster_sweep(work, w0, u, flip)

        traj = lambda: hmc(work, *coef, N_MD, DT, n_traj=inner)
        for _ in range(2):
            for tile in TILES:
                sweep(tile)()
            traj(); other()
        torch.cuda.synchronize()
        # the sweeps against each other at the timed size, from one position
        k = phi.clone()
        r = _hip.phi4_cluster_tiled(k, w0, position=(1, 0), want_labels=True, workspace=ws)
        if both:
            k2 = phi.clone()
            r2 = _hip.phi4_cluster(k2, w0, position=(1, 0), want_labels=True)
            same = bool(torch.equal(k2, k) and torch.equal(r2['labels'], r['labels']))
            other_rounds = int(r2['stats'][:, 3].max().item())
        else:
            c = cluster_sweep(phi, w0, *_hip.phi4_cluster_draws(C, lattice, DEV, position=(1, 0)))
            same = bool(torch.equal(c[0], k) and torch.equal(c[1], r['labels']) and torch.equal(c[2][:, :3], r['stats'][:, :3]))
            other_rounds = int(c[2][0, 3].item())
            del c
        stats = r['stats'].double()
        local_rounds = int(ws[8 * phi.numel():8 * phi.numel() + 8 * C].view(torch.int32).view(C, 2)[:, 1].max().item())
        ts, tt, to = {tile: [] for tile in TILES}, [], []
        for _ in range(reps):
            for tile in TILES:
                ts[tile].append(_ms(sweep(tile)) / inner)
            tt.append(_ms(traj) / inner)
            to.append(_ms(other) / (inner if both else 1))
    med = {tile: statistics.median(t) for tile, t in ts.items()}
    best = min(TILES, key=lambda tile: med[tile])
    plan = _hip.cluster_tiled_plan(lattice, dtype)
    default = _hip.cluster_tiled_plan((48, 48, 48, 48), dtype)['tile_sites']         # the library's default, one of TILES
    ms, mt, mo = med[default], statistics.median(tt), statistics.median(to)           # the ratios are those of the default
    spread = max((max(t) - min(t)) / statistics.median(t) for t in (ts[default], tt, to))
    margin = max(0.10, spread)
    rnd = lambda t: [round(min(t), 4), round(max(t), 4)]
    V = phi[0].numel()
    return dict(lattice=list(lattice), chains=C, dtype=str(dtype).replace("torch.", ""), n_md=N_MD, launches_per_timing=inner,
                tiled_ms={tile: round(med[tile], 4) for tile in TILES}, tiled_ms_spread={tile: rnd(ts[tile]) for tile in TILES},
                best_tile=best, default_tile=default, trajectory_ms=round(mt, 4), trajectory_ms_spread=rnd(tt), sweep_over_trajectory=round(ms / mt, 3),
                **{("kernel_ms" if both else "composed_ms"): round(mo, 4), ("kernel_ms_spread" if both else "composed_ms_spread"): rnd(to)},
                other_over_tiled=round(mo / ms, 2), margin=round(margin, 3), tiled_wins=bool(mo / ms > 1 + margin),
                same_bits=same, plan=plan, workspace_bytes=_hip.cluster_tiled_workspace(C, lattice),
                crossing_share={tile: round(crossing_share(lattice, min(tile, V)), 4) for tile in TILES},
                mean_clusters=round(stats[:, 0].mean().item(), 1), mean_largest_fraction=round(stats[:, 2].mean().item() / V, 4),
                tiles=int(stats[:, 3].max().item()), local_rounds=local_rounds, other_rounds=other_rounds)


def improved(lattice, C, dtype, kappa, reps, inner):
    """nf_cluster_moments on thermalised chains at `kappa`, against the sweep and the composed path, timed alternately."""
    from normflow__amd.mcmc.cluster import cluster_moments
    prior = NormalPrior(loc=torch.zeros(lattice, dtype=dtype, device=DEV), scale=torch.ones(lattice, dtype=dtype, device=DEV))
    model = nf.Model(net_=None, prior=prior, action=ScalarPhi4Action(**dict(COUPLINGS, kappa=kappa)))
    s = model.hmc
    torch.manual_seed(0)
    s.start(n_chains=C)
    with torch.no_grad():
        s.measure(30 * C, n_chains=C, n_md=N_MD, dt=DT, cluster_every=1)             # thermalise, sweeps included; no rows
        phi = s._ref['sample'].clone()
        w0 = float(model.action.get_coef(len(lattice))[0])
        r = _hip.phi4_cluster(phi.clone(), w0, position=(1, 0), want_labels=True)
        labels, stats = r['labels'], r['stats'].double()
        work = phi.clone()

        def moments():
            for _ in range(inner):
                _hip.cluster_moments(phi, labels)

        def sweep():
            for _ in range(inner):
                _hip.phi4_cluster(work, w0)

        composed = lambda: cluster_moments(phi, labels)
        for _ in range(2):
            moments(); sweep(); composed()
        torch.cuda.synchronize()
        k, c = _hip.cluster_moments(phi, labels, want_moments=True), cluster_moments(phi, labels, want_moments=True)
        same = bool(torch.equal(k['moments'], c['moments']) and torch.equal(k['status'], c['status']))
        rel = ((k['out'] - c['out']).abs() / c['out'].abs()).max().item()
        tm, ts, tc = [], [], []
        for _ in range(reps):
            tm.append(_ms(moments) / inner)
            ts.append(_ms(sweep) / inner)
            tc.append(_ms(composed))
        # the sampler: one recorded step of one trajectory with a sweep, with and without the improved row
        kw = dict(n_chains=C, n_md=N_MD, dt=DT, cluster_every=1)
        plain = lambda: s.measure(4 * C, **kw)
        with_improved = lambda: s.measure(4 * C, improved=True, **kw)
        plain(); with_improved()
        tp, ti = [], []
        for _ in range(reps):
            tp.append(_ms(plain) / 4)
            ti.append(_ms(with_improved) / 4)
    mm, ms, mc, mp, mi = (statistics.median(t) for t in (tm, ts, tc, tp, ti))
    spread = max((max(t) - min(t)) / statistics.median(t) for t in (tm, tc))
    margin = max(0.10, spread)
    rnd = lambda t: [round(min(t), 4), round(max(t), 4)]
    return dict(lattice=list(lattice), chains=C, dtype=str(dtype).replace("torch.", ""), kappa=kappa, launches_per_timing=inner,
                moments_ms=round(mm, 4), moments_ms_spread=rnd(tm),
                sweep_ms=round(ms, 4), sweep_ms_spread=rnd(ts), moments_over_sweep=round(mm / ms, 3),
                composed_ms=round(mc, 3), composed_ms_spread=rnd(tc), composed_over_kernel=round(mc / mm, 1),
                margin=round(margin, 3), kernel_wins=bool(mc / mm > 1 + margin), same_moments_as_composed=same,
                max_rel_diff_of_the_doubles=rel, plan=_hip.cluster_moments_plan(lattice, dtype),
                step_ms=round(mp, 4), step_ms_spread=rnd(tp), step_improved_ms=round(mi, 4), step_improved_ms_spread=rnd(ti),
                improved_over_plain_step=round(mi / mp, 3),
                mean_clusters=round(stats[:, 0].mean().item(), 1), mean_largest_fraction=round(stats[:, 2].mean().item() / phi[0].numel(), 4))


def spectrum(lattice, C, dtype, kappa, reps, inner):
    """nf_cluster_spectrum at momenta 1, 2, 4 and all on thermalised chains at `kappa`, against nf_cluster_moments, the
    composed path and one sweep plus one trajectory, timed alternately."""
    from normflow__amd.mcmc.cluster import cluster_spectrum
    prior = NormalPrior(loc=torch.zeros(lattice, dtype=dtype, device=DEV), scale=torch.ones(lattice, dtype=dtype, device=DEV))
    model = nf.Model(net_=None, prior=prior, action=ScalarPhi4Action(**dict(COUPLINGS, kappa=kappa)))
    s = model.hmc
    torch.manual_seed(0)
    s.start(n_chains=C)
    rnd = lambda t: [round(min(t), 4), round(max(t), 4)]
    rel_spread = lambda t: (max(t) - min(t)) / statistics.median(t)
    out = dict(lattice=list(lattice), chains=C, dtype=str(dtype).replace("torch.", ""), kappa=kappa, launches_per_timing=inner,
               momenta={})
    with torch.no_grad():
        s.measure(30 * C, n_chains=C, n_md=N_MD, dt=DT, cluster_every=1)             # thermalise, sweeps included; no rows
        phi = s._ref['sample'].clone()
        coef, w0 = s._coef(lattice), float(model.action.get_coef(len(lattice))[0])
        labels = _hip.phi4_cluster(phi.clone(), w0, position=(1, 0), want_labels=True)['labels']
        work = phi.clone()

        def moments():
            for _ in range(inner):
                _hip.cluster_moments(phi, labels)

        def step():                                                  # one sweep and one trajectory, in place on a copy
            for _ in range(inner):
                _hip.phi4_cluster(work, w0)
                _hip.phi4_hmc(work, *coef, N_MD, DT, n_traj=1)

        for momenta in (1, 2, 4, 'all'):
            def kernel():
                for _ in range(inner):
                    _hip.cluster_spectrum(phi, labels, momenta)

            composed = lambda: cluster_spectrum(phi, labels, momenta)
            for _ in range(2):
                kernel(); moments(); step(); composed()
            torch.cuda.synchronize()
            k, c = _hip.cluster_spectrum(phi, labels, momenta), composed()
            rel = ((k['out'] - c['out']).abs() / c['out'].abs()).max().item()
            tk, tm, ts, tc = [], [], [], []
            for _ in range(reps):
                tk.append(_ms(kernel) / inner)
                tm.append(_ms(moments) / inner)
                ts.append(_ms(step) / inner)
                tc.append(_ms(composed))
            mk, mm, mst, mc = (statistics.median(t) for t in (tk, tm, ts, tc))
            margin = max(0.10, rel_spread(tk), rel_spread(tm), rel_spread(tc))
            plan = _hip.cluster_spectrum_plan(lattice, dtype, momenta)
            out['momenta'][str(momenta)] = dict(
                spectrum_ms=round(mk, 4), spectrum_ms_spread=rnd(tk), moments_ms=round(mm, 4), moments_ms_spread=rnd(tm),
                spectrum_over_moments=round(mk / mm, 3), composed_ms=round(mc, 3), composed_ms_spread=rnd(tc),
                composed_over_kernel=round(mc / mk, 1), sweep_plus_trajectory_ms=round(mst, 4),
                sweep_plus_trajectory_ms_spread=rnd(ts), spectrum_over_step=round(mk / mst, 3), margin=round(margin, 3),
                kernel_wins=bool(mc / mk > 1 + margin), quantities=plan['quantities'], passes=plan['passes'],
                us_per_quantity=round(1000 * mk / plan['quantities'], 2), max_rel_diff_of_the_doubles=rel,
                same_status=bool(torch.equal(k['status'], c['status'])))
        one = out['momenta']['1']
        out['momenta_1_within_margin_of_moments'] = bool(one['spectrum_over_moments'] <= 1 + one['margin'])
    return out


def modes(lattice, C, dtype, kappa, reps, inner):
    """nf_cluster_modes at the on-axis momenta of `momenta` 1, 2, 4 and all, as a list, against nf_cluster_spectrum at the
    same Q and against the composed path, and at 16 generic off-axis momenta against the composed path, timed alternately
    on chains thermalised at `kappa` as in `spectrum`."""
    from normflow__amd.mcmc.cluster import cluster_modes
    prior = NormalPrior(loc=torch.zeros(lattice, dtype=dtype, device=DEV), scale=torch.ones(lattice, dtype=dtype, device=DEV))
    model = nf.Model(net_=None, prior=prior, action=ScalarPhi4Action(**dict(COUPLINGS, kappa=kappa)))
    s = model.hmc
    torch.manual_seed(0)
    s.start(n_chains=C)
    d = len(lattice)
    rnd = lambda t: [round(min(t), 4), round(max(t), 4)]
    rel_spread = lambda t: (max(t) - min(t)) / statistics.median(t)
    out = dict(lattice=list(lattice), chains=C, dtype=str(dtype).replace("torch.", ""), kappa=kappa, launches_per_timing=inner,
               on_axis={}, off_axis={})
    with torch.no_grad():
        s.measure(30 * C, n_chains=C, n_md=N_MD, dt=DT, cluster_every=1)             # thermalise, sweeps included; no rows
        phi = s._ref['sample'].clone()
        w0 = float(model.action.get_coef(len(lattice))[0])
        labels = _hip.phi4_cluster(phi.clone(), w0, position=(1, 0), want_labels=True)['labels']

        def timed(lst, spectrum_momenta=None):
            def kernel():
                for _ in range(inner):
                    _hip.cluster_modes(phi, labels, lst)

            def spec():
                for _ in range(inner):
                    _hip.cluster_spectrum(phi, labels, spectrum_momenta)

            composed = lambda: cluster_modes(phi, labels, lst)
            fns = [kernel, composed] + ([spec] if spectrum_momenta is not None else [])
            for _ in range(2):
                for f in fns:
                    f()
            torch.cuda.synchronize()
            k, c = _hip.cluster_modes(phi, labels, lst), composed()
            rel = ((k['out'] - c['out']).abs() / c['out'].abs()).max().item()
            tk, tc, ts = [], [], []
            for _ in range(reps):
                tk.append(_ms(kernel) / inner)
                if spectrum_momenta is not None:
                    ts.append(_ms(spec) / inner)
                tc.append(_ms(composed))
            mk, mc = statistics.median(tk), statistics.median(tc)
            plan = _hip.cluster_modes_plan(lattice, dtype, lst)
            margin = max([0.10, rel_spread(tk), rel_spread(tc)] + ([rel_spread(ts)] if ts else []))
            row = dict(momenta_in_list=len(lst), quantities=plan['quantities'], passes=plan['passes'], modes_ms=round(mk, 4),
                       modes_ms_spread=rnd(tk), us_per_quantity=round(1000 * mk / plan['quantities'], 2),
                       composed_ms=round(mc, 3), composed_ms_spread=rnd(tc), composed_over_kernel=round(mc / mk, 1),
                       margin=round(margin, 3), kernel_wins=bool(mc / mk > 1 + margin), max_rel_diff_of_the_doubles=rel,
                       same_status=bool(torch.equal(k['status'], c['status'])))
            if ts:
                ms = statistics.median(ts)
                sp = _hip.cluster_spectrum(phi, labels, spectrum_momenta)
                row.update(spectrum_ms=round(ms, 4), spectrum_ms_spread=rnd(ts), modes_over_spectrum=round(mk / ms, 3),
                           spectrum_quantities=_hip.cluster_spectrum_plan(lattice, dtype, spectrum_momenta)['quantities'],
                           within_margin_of_spectrum=bool(mk / ms <= 1 + margin),
                           same_bits_as_spectrum=bool(torch.equal(k['out'], sp['out'])))
            return row

        for momenta in (1, 2, 4, 'all'):
            K = _hip.spectrum_momenta(lattice, momenta)
            lst = [tuple(k if b == a else 0 for b in range(d)) for a in range(d) for k in range(1, K[a] + 1)]
            out['on_axis'][str(momenta)] = timed(lst, momenta)
        generic = [tuple((1 + i + 2 * a) % L for a, L in enumerate(lattice)) for i in range(16)]
        out['off_axis']['16 generic'] = timed(generic)
    out['all_within_margin_of_spectrum'] = all(r['within_margin_of_spectrum'] for r in out['on_axis'].values())
    out['kernel_wins_everywhere'] = all(r['kernel_wins'] for part in (out['on_axis'], out['off_axis']) for r in part.values())
    return out


def correlator_variance_ratios(steps):
    """Row variance of sum_s S(s) S(s + t) over that of its improved form, t = 0 .. L / 2, and the jackknife errors of
    G(L / 2) both ways: (8, 8), 32 chains, fp64, `steps` recorded steps after 100, a sweep before every step."""
    from normflow__amd.lib.observables import ImprovedEnsemble
    lattice, C, drop = (8, 8), 32, 100
    out = dict(lattice=list(lattice), chains=C, steps=steps, m_sq=COUPLINGS['m_sq'], lambd=COUPLINGS['lambd'], rows={})
    for kappa in (0.25, 0.45):
        prior = NormalPrior(loc=torch.zeros(lattice, dtype=torch.float64, device=DEV), scale=torch.ones(lattice, dtype=torch.float64, device=DEV))
        model = nf.Model(net_=None, prior=prior, action=ScalarPhi4Action(**dict(COUPLINGS, kappa=kappa)))
        s = model.hmc
        torch.manual_seed(1)
        s.start(n_chains=C)
        with torch.no_grad():
            m = s.measure((drop + steps) * C, n_chains=C, n_md=N_MD, dt=DT, cluster_every=1, improved=True, momenta='all')
        plain, imp = m.correlator(axis=0)[drop * C:], m.improved.correlator(axis=0)[drop * C:]
        (g, ge), (ig, ige) = (Ensemble(m, n_chains=C, drop=drop).correlator(axis=0),
                              ImprovedEnsemble(m.improved, n_chains=C, drop=drop).correlator(axis=0))
        out['rows'][str(kappa)] = dict(
            var_ratio_t=[round((plain[:, t].var() / imp[:, t].var()).item(), 2) for t in range(5)],
            G_plain=[round(float(x), 6) for x in g[:5]], G_plain_err=[round(float(x), 6) for x in ge[:5]],
            G_improved=[round(float(x), 6) for x in ig[:5]], G_improved_err=[round(float(x), 6) for x in ige[:5]],
            refused_rows=int(m.improved.status.sum().item()))
    return out


BLOCKS = (2048, 4096, 8192)


def _peak_mb(f):
    """Peak device memory of one call of f above what is allocated before it, in MB."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    f()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 1e6, 1)


def improved_tiled(lattice, C, dtype, kappa, reps, inner, both=False):
    """nf_cluster_moments_tiled on chains thermalised at `kappa` (20 steps of tiled sweep + tiled trajectory), at
    block_sites 2048, 4096 and 8192, against the composed path on the device, against one sweep of nf_phi4_cluster_tiled,
    and one `hmc.measure(cluster_every=1, improved='hbm')` step against improved='composed'; timed alternately.  `both`: a
    lattice nf_cluster_moments takes too -- against it as well."""
    from normflow__amd.mcmc.cluster import cluster_moments
    prior = NormalPrior(loc=torch.zeros(lattice, dtype=dtype, device=DEV), scale=torch.ones(lattice, dtype=dtype, device=DEV))
    model = nf.Model(net_=None, prior=prior, action=ScalarPhi4Action(**dict(COUPLINGS, kappa=kappa)))
    s = model.hmc
    torch.manual_seed(0)
    s.start(n_chains=C)
    with torch.no_grad():
        phi = s._ref['sample'].clone()
        coef, w0 = s._coef(lattice), float(model.action.get_coef(len(lattice))[0])
        sweep_ws = torch.empty(_hip.cluster_tiled_workspace(C, lattice), dtype=torch.uint8, device=DEV)
        hmc = _hip.phi4_hmc if both else _hip.phi4_hmc_tiled
        for _ in range(20):                                                          # thermalise, sweeps included
            _hip.phi4_cluster_tiled(phi, w0, workspace=sweep_ws)
            hmc(phi, *coef, N_MD, DT, n_traj=1)
        r = _hip.phi4_cluster_tiled(phi.clone(), w0, position=(1, 0), want_labels=True, workspace=sweep_ws)
        labels, stats = r['labels'], r['stats'].double()
        work = phi.clone()
        pp = _hip.cluster_moments_tiled_per_pass(C, lattice)
        ws = torch.empty(max(_hip.cluster_moments_tiled_workspace(C, lattice, b, pp) for b in BLOCKS), dtype=torch.uint8, device=DEV)

        def moments(block):
            def f():
                for _ in range(inner):
                    _hip.cluster_moments_tiled(phi, labels, block_sites=block, per_pass=pp, workspace=ws)
            return f

        def sweep():
            for _ in range(inner):
                _hip.phi4_cluster_tiled(work, w0, workspace=sweep_ws)

        def one_cu():
            for _ in range(inner):
                _hip.cluster_moments(phi, labels)

        composed = lambda: cluster_moments(phi, labels)
        for _ in range(2):
            for block in BLOCKS:
                moments(block)()
            sweep(); composed()
            if both:
                one_cu()
        torch.cuda.synchronize()
        k, c = _hip.cluster_moments_tiled(phi, labels, want_moments=True), cluster_moments(phi, labels, want_moments=True)
        same = bool(torch.equal(k['moments'], c['moments']) and torch.equal(k['status'], c['status']))
        rel = ((k['out'] - c['out']).abs() / c['out'].abs()).max().item()
        del k, c
        tm, ts, tc, t1 = {b: [] for b in BLOCKS}, [], [], []
        for _ in range(reps):
            for block in BLOCKS:
                tm[block].append(_ms(moments(block)) / inner)
            ts.append(_ms(sweep) / inner)
            tc.append(_ms(composed))
            if both:
                t1.append(_ms(one_cu) / inner)
        peak = dict(hbm=_peak_mb(lambda: _hip.cluster_moments_tiled(phi, labels)), composed=_peak_mb(composed))
        out = dict(lattice=list(lattice), chains=C, dtype=str(dtype).replace("torch.", ""), kappa=kappa, launches_per_timing=inner)
        if not both:             # the sampler: one recorded step of one trajectory with a sweep and the improved row
            kw = dict(n_chains=C, n_md=N_MD, dt=DT, cluster_every=1)
            s._ref.update(sample=phi.clone(), action=model.action(phi.double()).double())
            with_hbm = lambda: s.measure(2 * C, improved='hbm', **kw)
            with_composed = lambda: s.measure(2 * C, improved='composed', **kw)
            with_hbm(); with_composed()
            th, to = [], []
            for _ in range(reps):
                th.append(_ms(with_hbm) / 2)
                to.append(_ms(with_composed) / 2)
    rnd = lambda t: [round(min(t), 4), round(max(t), 4)]
    med = statistics.median
    mm, mc = med(tm[4096]), med(tc)
    spread = max((max(t) - min(t)) / med(t) for t in (tm[4096], tc))
    margin = max(0.10, spread)
    out.update(moments_ms={b: round(med(tm[b]), 4) for b in BLOCKS}, moments_ms_spread={b: rnd(tm[b]) for b in BLOCKS},
               sweep_ms=round(med(ts), 4), sweep_ms_spread=rnd(ts), moments_over_sweep=round(mm / med(ts), 3),
               composed_ms=round(mc, 3), composed_ms_spread=rnd(tc), composed_over_kernel=round(mc / mm, 1),
               margin=round(margin, 3), kernel_wins=bool(mc / mm > 1 + margin), same_moments_as_composed=same,
               max_rel_diff_of_the_doubles=rel, plan=_hip.cluster_moments_tiled_plan(lattice, dtype, 0, pp),
               workspace_mb=round(ws.numel() / 1e6, 1), peak_mb=peak,
               mean_clusters=round(stats[:, 0].mean().item(), 1),
               mean_largest_fraction=round(stats[:, 2].mean().item() / phi[0].numel(), 4))
    if both:
        out.update(one_cu_kernel_ms=round(med(t1), 4), one_cu_kernel_ms_spread=rnd(t1), hbm_over_one_cu=round(mm / med(t1), 2))
    else:
        out.update(step_hbm_ms=round(med(th), 4), step_hbm_ms_spread=rnd(th), step_composed_ms=round(med(to), 4),
                   step_composed_ms_spread=rnd(to), composed_over_hbm_step=round(med(to) / med(th), 2))
    return out


SPECTRUM_MOMENTA = (1, 2, 4, 'all')
PER_PASSES = (4, 8, 16)


def spectrum_tiled(lattice, C, dtype, kappa, reps, inner, both=False, composed_momenta=(1, 4)):
    """nf_cluster_spectrum_tiled on chains thermalised at `kappa` as in `improved_tiled`, at momenta 1, 2, 4 and all with the
    default block and the footprint's per_pass, timed alternately against: (a) the composed path on the device at
    `composed_momenta` (at 'all' it is too slow and too large to repeat on the large lattices: its cost is linear in the
    quantities); (b) nf_cluster_moments_tiled at momenta 1; (c) `both`: nf_cluster_spectrum, on a lattice it takes too;
    (d) one tiled sweep plus one tiled trajectory (n_md = 10); (e) per_pass 4, 8, 16 and block_sites 2048, 4096, 8192 at
    'all'; (f) the peak memory of one call above what is resident."""
    from normflow__amd.mcmc.cluster import cluster_spectrum
    prior = NormalPrior(loc=torch.zeros(lattice, dtype=dtype, device=DEV), scale=torch.ones(lattice, dtype=dtype, device=DEV))
    model = nf.Model(net_=None, prior=prior, action=ScalarPhi4Action(**dict(COUPLINGS, kappa=kappa)))
    s = model.hmc
    torch.manual_seed(0)
    s.start(n_chains=C)
    med = statistics.median
    rnd = lambda t: [round(min(t), 4), round(max(t), 4)]
    with torch.no_grad():
        phi = s._ref['sample'].clone()
        coef, w0 = s._coef(lattice), float(model.action.get_coef(len(lattice))[0])
        sweep_ws = torch.empty(_hip.cluster_tiled_workspace(C, lattice), dtype=torch.uint8, device=DEV)
        hmc = _hip.phi4_hmc if both else _hip.phi4_hmc_tiled
        for _ in range(20):                                                          # thermalise, sweeps included
            _hip.phi4_cluster_tiled(phi, w0, workspace=sweep_ws)
            hmc(phi, *coef, N_MD, DT, n_traj=1)
        r = _hip.phi4_cluster_tiled(phi.clone(), w0, position=(1, 0), want_labels=True, workspace=sweep_ws)
        labels, stats = r['labels'], r['stats'].double()
        work = phi.clone()
        Q = {m: _hip.cluster_spectrum_tiled_plan(lattice, dtype, m)['quantities'] for m in SPECTRUM_MOMENTA}
        pp = {m: _hip.cluster_spectrum_tiled_per_pass(C, lattice, m) for m in SPECTRUM_MOMENTA}
        variants = [('all', 0, p) for p in PER_PASSES if p <= Q['all']] + [('all', b, min(16, Q['all'])) for b in BLOCKS]
        ws = torch.empty(max([_hip.cluster_spectrum_tiled_workspace(C, lattice, m, 0, pp[m]) for m in SPECTRUM_MOMENTA]
                             + [_hip.cluster_spectrum_tiled_workspace(C, lattice, m, b, p) for m, b, p in variants]),
                         dtype=torch.uint8, device=DEV)
        mpp = _hip.cluster_moments_tiled_per_pass(C, lattice)
        mws = torch.empty(_hip.cluster_moments_tiled_workspace(C, lattice, 0, mpp), dtype=torch.uint8, device=DEV)

        def tiled(m, block=0, per_pass=None):
            per_pass = pp[m] if per_pass is None else per_pass

            def f():
                for _ in range(inner):
                    _hip.cluster_spectrum_tiled(phi, labels, m, block_sites=block, per_pass=per_pass, workspace=ws)
            return f

        def moments():
            for _ in range(inner):
                _hip.cluster_moments_tiled(phi, labels, per_pass=mpp, workspace=mws)

        def sweep():
            for _ in range(inner):
                _hip.phi4_cluster_tiled(work, w0, workspace=sweep_ws)

        def trajectory():
            hmc(work, *coef, N_MD, DT, n_traj=inner)

        def one_cu(m):
            def f():
                for _ in range(inner):
                    _hip.cluster_spectrum(phi, labels, m)
            return f

        composed = lambda m: (lambda: cluster_spectrum(phi, labels, m))
        runs = {f"tiled_k{m}": tiled(m) for m in SPECTRUM_MOMENTA}
        runs.update({f"tiled_all_b{b}_p{p}": tiled(m, b, p) for m, b, p in variants})
        runs.update(moments_tiled=moments, sweep=sweep, trajectory=trajectory)
        if both:
            runs.update({f"one_cu_k{m}": one_cu(m) for m in SPECTRUM_MOMENTA})
        single = {f"composed_k{m}": composed(m) for m in composed_momenta}      # one call per timing
        for f in list(runs.values()) + list(single.values()):
            f()
        torch.cuda.synchronize()
        k, c = _hip.cluster_spectrum_tiled(phi, labels, composed_momenta[-1]), cluster_spectrum(phi, labels, composed_momenta[-1])
        same = bool(torch.equal(k['status'], c['status']))
        rel = ((k['out'] - c['out']).abs() / c['out'].abs()).max().item()
        del k, c
        t = {name: [] for name in list(runs) + list(single)}
        for _ in range(max(5, reps)):                                                # alternating
            for name, f in runs.items():
                t[name].append(_ms(f) / inner)
            for name, f in single.items():
                t[name].append(_ms(f))
        peak = dict(hbm_all=_peak_mb(lambda: _hip.cluster_spectrum_tiled(phi, labels, 'all')),
                    **{f"composed_k{m}": _peak_mb(composed(m)) for m in composed_momenta})
    spread = max((max(v) - min(v)) / med(v) for v in t.values())
    margin = max(0.10, spread)
    out = dict(lattice=list(lattice), chains=C, dtype=str(dtype).replace("torch.", ""), kappa=kappa, launches_per_timing=inner,
               timings=max(5, reps), quantities={str(m): Q[m] for m in SPECTRUM_MOMENTA},
               per_pass={str(m): pp[m] for m in SPECTRUM_MOMENTA},
               ms={name: round(med(v), 4) for name, v in t.items()}, ms_spread={name: rnd(v) for name, v in t.items()},
               margin=round(margin, 3), same_status_as_composed=same, max_rel_diff_of_the_doubles=rel,
               plan_all=_hip.cluster_spectrum_tiled_plan(lattice, dtype, 'all', 0, pp['all']),
               workspace_mb_all=round(_hip.cluster_spectrum_tiled_workspace(C, lattice, 'all', 0, pp['all']) / 1e6, 1), peak_mb=peak,
               mean_clusters=round(stats[:, 0].mean().item(), 1),
               mean_largest_fraction=round(stats[:, 2].mean().item() / phi[0].numel(), 4))
    ms = {name: med(v) for name, v in t.items()}
    step = ms['sweep'] + ms['trajectory']
    out.update(
        a_composed_over_tiled={str(m): round(ms[f"composed_k{m}"] / ms[f"tiled_k{m}"], 1) for m in composed_momenta},
        a_composed_ms_per_quantity={str(m): round(ms[f"composed_k{m}"] / Q[m], 3) for m in composed_momenta},
        b_tiled_k1_over_moments_tiled=round(ms['tiled_k1'] / ms['moments_tiled'], 3),
        b_within_margin=bool(abs(ms['tiled_k1'] / ms['moments_tiled'] - 1) <= margin),
        d_sweep_plus_trajectory_ms=round(step, 4),
        d_tiled_ms_per_quantity={str(m): round(ms[f"tiled_k{m}"] / Q[m], 4) for m in SPECTRUM_MOMENTA},
        d_tiled_all_over_step=round(ms['tiled_kall'] / step, 2),
        e_per_pass_ms={str(p): round(ms[f"tiled_all_b0_p{p}"], 4) for p in PER_PASSES if p <= Q['all']},
        e_block_sites_ms={str(b): round(ms[f"tiled_all_b{b}_p{min(16, Q['all'])}"], 4) for b in BLOCKS})
    if both:
        out.update(c_tiled_over_one_cu={str(m): round(ms[f"tiled_k{m}"] / ms[f"one_cu_k{m}"], 2) for m in SPECTRUM_MOMENTA})
    return out


def modes_tiled(lattice, C, dtype, kappa, reps, inner, both=False):
    """nf_cluster_modes_tiled on chains thermalised at `kappa` as in `spectrum_tiled`, with the default block and the
    footprint's per_pass, timed alternately against: (a) the composed path on the device (`mcmc.cluster.cluster_modes`) at
    3 generic momenta, a list length it can repeat on every class (its cost is linear in the quantities; at 16 momenta
    it is left out); (b) nf_cluster_spectrum_tiled of the same build at momenta 1, 2 and 4, with the same on-axis momenta
    given as a list: the same Q; (c) `both`: nf_cluster_modes, on a lattice it takes too; (d) per_pass 4, 8, 16 and
    block_sites 2048, 4096, 8192 at 16 generic momenta (Q = 33); (e) the peak memory of one call above what is resident."""
    from normflow__amd.mcmc.cluster import cluster_modes
    prior = NormalPrior(loc=torch.zeros(lattice, dtype=dtype, device=DEV), scale=torch.ones(lattice, dtype=dtype, device=DEV))
    model = nf.Model(net_=None, prior=prior, action=ScalarPhi4Action(**dict(COUPLINGS, kappa=kappa)))
    s = model.hmc
    torch.manual_seed(0)
    s.start(n_chains=C)
    d = len(lattice)
    med = statistics.median
    rnd = lambda t: [round(min(t), 4), round(max(t), 4)]
    with torch.no_grad():
        phi = s._ref['sample'].clone()
        coef, w0 = s._coef(lattice), float(model.action.get_coef(d)[0])
        sweep_ws = torch.empty(_hip.cluster_tiled_workspace(C, lattice), dtype=torch.uint8, device=DEV)
        hmc = _hip.phi4_hmc if both else _hip.phi4_hmc_tiled
        for _ in range(20):                                                          # thermalise, sweeps included
            _hip.phi4_cluster_tiled(phi, w0, workspace=sweep_ws)
            hmc(phi, *coef, N_MD, DT, n_traj=1)
        r = _hip.phi4_cluster_tiled(phi.clone(), w0, position=(1, 0), want_labels=True, workspace=sweep_ws)
        labels, stats = r['labels'], r['stats'].double()
        on_axis = {}
        for m in (1, 2, 4):
            K = _hip.spectrum_momenta(lattice, m)
            on_axis[m] = tuple(tuple(k if b == a else 0 for b in range(d)) for a in range(d) for k in range(1, K[a] + 1))
        generic = tuple(tuple((1 + i + 2 * a) % L for a, L in enumerate(lattice)) for i in range(16))
        lists = {f"k{m}": on_axis[m] for m in on_axis}
        lists.update(g3=generic[:3], g16=generic)
        Q = {name: _hip.modes_quantities(lattice, lst) for name, lst in lists.items()}
        pp = {name: _hip.cluster_modes_tiled_per_pass(C, lattice, lst) for name, lst in lists.items()}
        variants = [(0, p) for p in PER_PASSES if p <= Q['g16']] + [(b, min(16, Q['g16'])) for b in BLOCKS]
        ws = torch.empty(max([_hip.cluster_modes_tiled_workspace(C, lattice, Q[n], 0, pp[n]) for n in lists]
                             + [_hip.cluster_modes_tiled_workspace(C, lattice, Q['g16'], b, p) for b, p in variants]),
                         dtype=torch.uint8, device=DEV)
        spp = {m: _hip.cluster_spectrum_tiled_per_pass(C, lattice, m) for m in on_axis}
        sws = torch.empty(max(_hip.cluster_spectrum_tiled_workspace(C, lattice, m, 0, spp[m]) for m in on_axis),
                          dtype=torch.uint8, device=DEV)

        def tiled(name, block=0, per_pass=None):
            per_pass = pp[name] if per_pass is None else per_pass

            def f():
                for _ in range(inner):
                    _hip.cluster_modes_tiled(phi, labels, lists[name], block_sites=block, per_pass=per_pass, workspace=ws)
            return f

        def spectrum_of(m):
            def f():
                for _ in range(inner):
                    _hip.cluster_spectrum_tiled(phi, labels, m, per_pass=spp[m], workspace=sws)
            return f

        def one_cu(name):
            def f():
                for _ in range(inner):
                    _hip.cluster_modes(phi, labels, lists[name])
            return f

        composed = lambda: cluster_modes(phi, labels, lists['g3'])
        runs = {f"tiled_{name}": tiled(name) for name in lists}
        runs.update({f"tiled_g16_b{b}_p{p}": tiled('g16', b, p) for b, p in variants})
        runs.update({f"spectrum_tiled_k{m}": spectrum_of(m) for m in on_axis})
        if both:
            runs.update({f"one_cu_{name}": one_cu(name) for name in lists})
        single = dict(composed_g3=composed)                                          # one call per timing
        for f in list(runs.values()) + list(single.values()):
            f()
        torch.cuda.synchronize()
        k, c = _hip.cluster_modes_tiled(phi, labels, lists['g3']), composed()
        same = bool(torch.equal(k['status'], c['status']))
        rel = ((k['out'] - c['out']).abs() / c['out'].abs()).max().item()
        sp = _hip.cluster_spectrum_tiled(phi, labels, 4)
        same_bits = bool(torch.equal(_hip.cluster_modes_tiled(phi, labels, lists['k4'])['out'], sp['out']))
        del k, c, sp
        t = {name: [] for name in list(runs) + list(single)}
        for _ in range(max(5, reps)):                                                # alternating
            for name, f in runs.items():
                t[name].append(_ms(f) / inner)
            for name, f in single.items():
                t[name].append(_ms(f))
        peak = dict(hbm_g16=_peak_mb(lambda: _hip.cluster_modes_tiled(phi, labels, lists['g16'])),
                    hbm_g3=_peak_mb(lambda: _hip.cluster_modes_tiled(phi, labels, lists['g3'])), composed_g3=_peak_mb(composed))
    spread = max((max(v) - min(v)) / med(v) for v in t.values())
    margin = max(0.10, spread)
    ms = {name: med(v) for name, v in t.items()}
    out = dict(lattice=list(lattice), chains=C, dtype=str(dtype).replace("torch.", ""), kappa=kappa, launches_per_timing=inner,
               timings=max(5, reps), quantities=Q, per_pass=pp, spectrum_per_pass={str(m): spp[m] for m in spp},
               ms={name: round(v, 4) for name, v in ms.items()}, ms_spread={name: rnd(v) for name, v in t.items()},
               margin=round(margin, 3), same_status_as_composed=same, max_rel_diff_of_the_doubles=rel,
               on_axis_k4_same_bits_as_spectrum_tiled=same_bits,
               plan_g16=_hip.cluster_modes_tiled_plan(lattice, dtype, lists['g16'], 0, pp['g16']),
               workspace_mb_g16=round(_hip.cluster_modes_tiled_workspace(C, lattice, Q['g16'], 0, pp['g16']) / 1e6, 1),
               peak_mb=peak, mean_clusters=round(stats[:, 0].mean().item(), 1),
               mean_largest_fraction=round(stats[:, 2].mean().item() / phi[0].numel(), 4))
    out.update(
        a_composed_over_tiled_g3=round(ms['composed_g3'] / ms['tiled_g3'], 1),
        a_tiled_wins=bool(ms['composed_g3'] / ms['tiled_g3'] > 1 + margin),
        b_tiled_over_spectrum_tiled={str(m): round(ms[f"tiled_k{m}"] / ms[f"spectrum_tiled_k{m}"], 3) for m in on_axis},
        b_within_margin=bool(all(ms[f"tiled_k{m}"] / ms[f"spectrum_tiled_k{m}"] <= 1 + margin for m in on_axis)),
        us_per_quantity={name: round(1000 * ms[f"tiled_{name}"] / Q[name], 2) for name in lists},
        d_per_pass_ms={str(p): round(ms[f"tiled_g16_b0_p{p}"], 4) for p in PER_PASSES if p <= Q['g16']},
        d_block_sites_ms={str(b): round(ms[f"tiled_g16_b{b}_p{min(16, Q['g16'])}"], 4) for b in BLOCKS})
    if both:
        out.update(c_tiled_over_one_cu={name: round(ms[f"tiled_{name}"] / ms[f"one_cu_{name}"], 2) for name in lists},
                   c_tiled_is_slower=bool(all(ms[f"tiled_{name}"] / ms[f"one_cu_{name}"] > 1 + margin for name in lists)))
    return out


def variance_ratios(steps):
    """Row variance of (sum phi)^2 over that of sum_C M_C^2, and of |phi~(p_min)|^2 over that of sum_C |M~_C(p_min)|^2, with
    the means both ways: (8, 8), 32 chains, fp64, `steps` recorded steps after 200, a sweep before every step."""
    from normflow__amd.lib.observables import ImprovedEnsemble
    lattice, C, drop = (8, 8), 32, 200
    out = dict(lattice=list(lattice), chains=C, steps=steps, m_sq=COUPLINGS['m_sq'], lambd=COUPLINGS['lambd'], rows={})
    for kappa in (0.67, 0.45, 0.35, 0.25):
        prior = NormalPrior(loc=torch.zeros(lattice, dtype=torch.float64, device=DEV), scale=torch.ones(lattice, dtype=torch.float64, device=DEV))
        model = nf.Model(net_=None, prior=prior, action=ScalarPhi4Action(**dict(COUPLINGS, kappa=kappa)))
        s = model.hmc
        torch.manual_seed(3)
        s.start(n_chains=C)
        with torch.no_grad():
            m = s.measure((drop + steps) * C, n_chains=C, n_md=N_MD, dt=DT, cluster_every=1, improved=True)
        im = m.improved
        plain2, imp2 = (m.sum_phi ** 2)[drop * C:], im.sum_m2[drop * C:]
        plainp, impp = (m.propagator()[:, 1] * 64)[drop * C:], im.prop1.mean(dim=1)[drop * C:]
        e, ie = Ensemble(m, n_chains=C, drop=drop), ImprovedEnsemble(im, n_chains=C, drop=drop)
        r4 = lambda v: [round(float(x), 4) for x in v]
        out['rows'][str(kappa)] = dict(
            var_ratio_m2=round((plain2.var() / imp2.var()).item(), 2), var_ratio_prop1=round((plainp.var() / impp.var()).item(), 2),
            chi_plain=r4([64 * x for x in e.mean('m2')]), chi_improved=r4(ie.susceptibility()),
            binder_plain=r4(e.binder()), binder_improved=r4(ie.binder()), xi2_plain=r4(e.xi2()), xi2_improved=r4(ie.xi2()),
            refused_rows=int(im.status.sum().item()))
    return out


def tunnelling(steps):
    lattice, C = (8, 8), 32
    out = dict(lattice=list(lattice), chains=C, steps=steps, **COUPLINGS)
    for every in (0, 1):
        model = _model(lattice, torch.float32)
        s = model.hmc
        torch.manual_seed(3)
        s.start(n_chains=C)
        kw = dict(n_chains=C, n_md=N_MD, dt=DT, cluster_every=every)
        with torch.no_grad():
            s.measure(steps * C, **kw)                                               # thermalise
            m = s.measure(steps * C, **kw)
        tau = Ensemble(m, n_chains=C).tau_int('magnetization')
        row = dict(tau_int_m=[round(float(v), 2) for v in tau], mean_abs_m=round(m.magnetization().abs().mean().item(), 4),
                   accept_rate=round(s.history.accept_rate[-1], 3))
        if every:
            row['mean_largest_fraction'] = round(s.last['cluster'][..., 2].double().mean().item() / 64, 4)
        out[f"cluster_every_{every}"] = row
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20, help="launches (sweeps) or trajectories per timing")
    ap.add_argument("--steps", type=int, default=1500, help="recorded steps of the tau_int run (and of its thermalisation)")
    ap.add_argument("--skip-tau", action="store_true")
    ap.add_argument("--tiled", action="store_true", help="nf_phi4_cluster_tiled on the lattices beyond nf_phi4_cluster")
    ap.add_argument("--improved", action="store_true", help="nf_cluster_moments and the improved estimators")
    ap.add_argument("--improved-tiled", action="store_true", help="nf_cluster_moments_tiled on the lattices beyond nf_cluster_moments")
    ap.add_argument("--spectrum", action="store_true", help="nf_cluster_spectrum and the improved correlator")
    ap.add_argument("--spectrum-tiled", action="store_true", help="nf_cluster_spectrum_tiled on the lattices beyond nf_cluster_spectrum")
    ap.add_argument("--modes", action="store_true", help="nf_cluster_modes against nf_cluster_spectrum and the composed path")
    ap.add_argument("--modes-tiled", action="store_true", help="nf_cluster_modes_tiled on the lattices beyond nf_cluster_modes")
    ap.add_argument("--shapes", default="", help="--improved-tiled, --spectrum-tiled, --modes-tiled: comma-separated indices into 16^3 x 1024 and "
                                                  "the four tiled shapes")
    ap.add_argument("--dtypes", default="float32,float64", help="--spectrum-tiled, --modes-tiled: the dtypes of the run")
    ap.add_argument("--kappas", default="0.67,0.25", help="--spectrum-tiled, --modes-tiled: the couplings of the run")
    a = ap.parse_args()
    if a.modes_tiled:
        shapes = [((16, 16, 16), 1024, True)] + [(lat, C, False) for lat, C in TILED_SHAPES]
        picked = [int(i) for i in a.shapes.split(",") if i != ""] or range(len(shapes))
        for i in picked:
            lattice, C, both = shapes[i]
            for dtype in [getattr(torch, d) for d in a.dtypes.split(",")]:
                for kappa in [float(k) for k in a.kappas.split(",")]:
                    print(json.dumps(modes_tiled(lattice, C, dtype, kappa, a.reps, a.inner, both=both)), flush=True)
        return
    if a.modes:
        for lattice, C in SHAPES:
            for dtype in (torch.float32, torch.float64):
                for kappa in (0.67, 0.25):
                    print(json.dumps(modes(lattice, C, dtype, kappa, a.reps, a.inner)), flush=True)
        return
    if a.spectrum_tiled:
        shapes = [((16, 16, 16), 1024, True)] + [(lat, C, False) for lat, C in TILED_SHAPES]
        picked = [int(i) for i in a.shapes.split(",") if i != ""] or range(len(shapes))
        for i in picked:
            lattice, C, both = shapes[i]
            for dtype in [getattr(torch, d) for d in a.dtypes.split(",")]:
                for kappa in [float(k) for k in a.kappas.split(",")]:
                    print(json.dumps(spectrum_tiled(lattice, C, dtype, kappa, a.reps, a.inner, both=both)), flush=True)
        return
    if a.spectrum:
        for lattice, C in SHAPES:
            for dtype in (torch.float32, torch.float64):
                for kappa in (0.67, 0.25):
                    print(json.dumps(spectrum(lattice, C, dtype, kappa, a.reps, a.inner)), flush=True)
        if not a.skip_tau:
            print(json.dumps(correlator_variance_ratios(a.steps)), flush=True)
        return
    if a.improved_tiled:
        shapes = [((16, 16, 16), 1024, True)] + [(lat, C, False) for lat, C in TILED_SHAPES]
        picked = [int(i) for i in a.shapes.split(",") if i != ""] or range(len(shapes))
        for i in picked:
            lattice, C, both = shapes[i]
            for dtype in (torch.float32, torch.float64):
                for kappa in (0.67, 0.25):
                    print(json.dumps(improved_tiled(lattice, C, dtype, kappa, a.reps, a.inner, both=both)), flush=True)
        return
    if a.improved:
        for lattice, C in SHAPES:
            for dtype in (torch.float32, torch.float64):
                for kappa in (0.67, 0.25):
                    print(json.dumps(improved(lattice, C, dtype, kappa, a.reps, a.inner)), flush=True)
        if not a.skip_tau:
            print(json.dumps(variance_ratios(a.steps)), flush=True)
        return
    if a.tiled:
        for dtype in (torch.float32, torch.float64):
            print(json.dumps(tiled((16, 16, 16), 1024, dtype, a.reps, a.inner, both=True)), flush=True)
        for lattice, C in TILED_SHAPES:
            for dtype in (torch.float32, torch.float64):
                print(json.dumps(tiled(lattice, C, dtype, a.reps, a.inner)), flush=True)
        return
    for lattice, C in SHAPES:
        for dtype in (torch.float32, torch.float64):
            print(json.dumps(launches(lattice, C, dtype, a.reps, a.inner)), flush=True)
    if not a.skip_tau:
        print(json.dumps(tunnelling(a.steps)), flush=True)


if __name__ == "__main__":
    main()

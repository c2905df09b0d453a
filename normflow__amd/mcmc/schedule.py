"""How the HMC samplers cut `rows` recorded steps, each of `every` trajectories of `n_md` MD steps, into kernel launches
that stay under the library's work caps: integers in, a list of actions out -- no tensors, no device.

The four kernels keep the rules they were written with (mcmc/hmc.py, mcmc/ladder.py), told apart by `tiled` and `ladder`:
  * `budget` is `_hip.hmc_fused_budget` (MD steps of one launch) or `_hip.hmc_tiled_budget` (trajectories of one call);
    a launch without rows holds per = max(1, budget // n_md) (fused) or max(1, budget) (tiled) trajectories;
  * a launch holds `fit` whole recorded steps.  Fused: budget // group, group = every * n_md, plus `measure_cost` MD steps
    where the launch measures (`stats`); the plain sampler without statistics counts per // every instead, so its forced
    single trajectory (budget < n_md) is still a recording launch.  Tiled: per // every, and with statistics -- which
    the tiled kernels leave to a measure kernel on the chains in place -- 1 at most (ladder) or never (plain);
  * fit = 0, a recorded step is more than a launch: launches of min(per, left) trajectories without rows, then the row
    is taken from the chains where they lie.  The plain fused sampler with statistics instead ends the step with a
    measuring launch of the last = max(1, min(every, (budget - measure_cost) // n_md)) trajectories."""
from typing import NamedTuple, Optional


class Launch(NamedTuple):
    """One kernel call: n_traj trajectories; with record_every it fills the rows row0 .. row0 + n_rows - 1 (the rows
    themselves where `record`, their statistics where `measure`)."""
    n_traj: int
    record_every: Optional[int] = None
    measure: bool = False
    record: bool = True
    row0: int = 0
    n_rows: int = 0


class Take(NamedTuple):
    """Row `row` from the chains where they lie: its statistics where wanted, and the row itself where `copy`."""
    row: int
    copy: bool = True


def schedule(rows, every, n_md, budget, *, tiled, ladder, stats, want_rows, measure_cost=0):
    """The ordered actions of a span of `rows` recorded steps."""
    per = max(1, budget if tiled else budget // n_md)
    in_launch = stats and not tiled
    if tiled:
        fit = per // every if not stats else min(1, per // every) if ladder else 0
    elif ladder or stats:
        fit = budget // (every * n_md + (measure_cost if stats else 0))
    else:
        fit = per // every
    acts = []
    if fit >= 1:
        record_every = every if want_rows or not tiled else None
        for r in range(0, rows, fit):
            k = min(fit, rows - r)
            acts.append(Launch(k * every, record_every, in_launch, want_rows, r, k if record_every else 0))
            if stats and tiled:
                acts.append(Take(r, copy=False))
        return acts
    last = max(1, min(every, (budget - measure_cost) // n_md)) if in_launch and not ladder else 0
    for r in range(rows):
        left = every - last
        while left:
            k = min(per, left)
            acts.append(Launch(k))
            left -= k
        acts.append(Launch(last, last, True, want_rows, r, 1) if last else Take(r, copy=want_rows))
    return acts


def schedule_fa(rows, every, cost, budget, *, want_rows, stats):
    """The ordered actions of a span of `rows` recorded steps of the Fourier-accelerated kernel (nf_phi4_hmc_fa), an entry
    of its own: `cost` is `_hip.hmc_fa_cost(n_md * s)`, the MD steps one trajectory counts as under the cap (its force
    evaluations and NF_HMC_FA_MD_STEPS per filter), `budget` is `_hip.hmc_fused_budget`.  A launch holds per = max(1,
    budget // cost) trajectories, fit = per // every whole recorded steps.  The kernel does not measure: with `stats` a
    launch records its rows (whether or not the caller wants them) and they are measured afterwards, which `record` of
    the Launch says and `measure` never does.  fit = 0: launches of min(per, left) trajectories without rows, then the
    row is taken from the chains where they lie."""
    per = max(1, budget // cost)
    fit = per // every
    acts = []
    if fit >= 1:
        for r in range(0, rows, fit):
            k = min(fit, rows - r)
            acts.append(Launch(k * every, every, False, want_rows or stats, r, k))
        return acts
    for r in range(rows):
        left = every
        while left:
            k = min(per, left)
            acts.append(Launch(k))
            left -= k
        acts.append(Take(r, copy=want_rows))
    return acts

"""The samplers' runs split at a lowered work cap, on the device: the branches that no other test reaches -- the tiled
kernels under NF_HMC_TILED_MAX_LAUNCHES and both ladder kernels under their caps.

Every case is one setup, lattice (6, 6), fp32, n_md = 2, n_skip = 1 (a recorded step is two trajectories: the per-row
branch has a launch before its last one), 6 recorded steps, and a sweep period of 2 (sweeps inside a call and at its
end); the ladder has K = 2 rungs and C = 4 chains (two replica sets).  The cap is lowered so that a launch holds two
recorded steps, one, or one trajectory, and everything the call leaves -- rows, statistics, chains, `last`, `history`,
the generator's offset -- must be bit for bit what the same call leaves under the real caps, from equal chain and
generator state; the wrapper is counted to see that the run really was split."""
import functools

import pytest
import torch

from normflow__amd import _hip

import hmc_cases as H
import ladder_cases as Lc
from hmc_cases import DEV, field as _field

pytestmark = pytest.mark.gpu

F32 = torch.float32
LATTICE, N_MD, DT, N_SKIP, STEPS, E, K = (6, 6), 2, 0.15, 1, 6, 2, 2
TILED_CAPS = (16, 8, 4)                     # (n_md + 2) = 4 launches per trajectory: 4, 2, 1 trajectories per call
# sampler, path, chains, the wrapper, the constant, {measuring: the caps for two steps / one step / one trajectory per launch}
KINDS = {
    'plain-tiled': ('plain', 'tiled', 3, 'phi4_hmc_tiled', 'HMC_TILED_MAX_LAUNCHES', {False: TILED_CAPS, True: TILED_CAPS}),
    # a recorded step is 2 * 2 MD steps, and NF_HMC_MEASURE_MD_STEPS = 16 more where the launch measures
    'ladder-fused': ('ladder', 'fused', 4, 'phi4_hmc_ladder', 'HMC_MAX_WORK',
                     {False: (256 * 8, 256 * 4, 256 * 2), True: (256 * 40, 256 * 20, 256 * 3)}),
    'ladder-tiled': ('ladder', 'tiled', 4, 'phi4_hmc_tiled_ladder', 'HMC_TILED_MAX_LAUNCHES',
                     {False: TILED_CAPS, True: TILED_CAPS}),
}
RUNS = ('sample', 'measure', 'measure_rows')
CASES = ([('plain-tiled', 'sample', 0), ('plain-tiled', 'measure', 0), ('plain-tiled', 'sample', E),
          ('plain-tiled', 'measure_rows', E)]
         + [(kind, run, E) for kind in ('ladder-fused', 'ladder-tiled') for run in RUNS])


def _measurement(m):
    return dict(sum_phi=m.sum_phi, sum_phi2=m.sum_phi2, sum_phi4=m.sum_phi4, links=m.links, action=m.action,
                **{f"slices_{mu}": s for mu, s in enumerate(m.slices)})


def _run(kind, run, every_e):
    """Everything one call leaves: {name: tensor or plain value}."""
    sampler, path, C = KINDS[kind][:3]
    if sampler == 'plain':
        s = H.model(LATTICE, F32, DEV, **H.INTERACTING).hmc
        kw = dict(cluster_every=every_e)
    else:
        m, ladder = Lc.model(LATTICE, F32, DEV, **Lc.DISTINCT(K))
        s = m.hmc.ladder(ladder)
        kw = dict(exchange_every=every_e)
    s.start(_field((C,) + LATTICE, F32, 1700))
    torch.manual_seed(17)
    kw.update(n_chains=C, n_md=N_MD, dt=DT, n_skip=N_SKIP, path=path)
    left = {}
    if run == 'sample':
        left['rows'] = s.sample(STEPS * C, **kw)
    else:
        got = s.measure(STEPS * C, return_rows=run == 'measure_rows', **kw)
        if run == 'measure_rows':
            got, left['rows'] = got
        for k, m in enumerate(got if sampler == 'ladder' else [got]):
            left.update({f"measure[{k}].{name}": t for name, t in _measurement(m).items()})
    left['offset'] = torch.cuda.default_generators[DEV.index].get_offset()
    left.update({f"_ref.{key}": t for key, t in s._ref.items()})
    left.update({f"last.{key}": t for key, t in s.last.items()})
    left.update({f"history.{key}": repr(getattr(s.history, key)) for key in s.history._KEYS})
    return left


@functools.lru_cache(maxsize=None)
def _whole(kind, run, every_e):
    """The call under the real caps: computed once per case, before any cap is lowered, and never written."""
    return _run(kind, run, every_e)


@pytest.mark.parametrize("level", (0, 1, 2), ids=("two-steps", "one-step", "one-trajectory"))
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{c[1]}-E{c[2]}")
def test_split_run_is_the_whole_run(case, level, monkeypatch):
    kind, run, every_e = case
    sampler, path, C, wrapper, constant, caps = KINDS[kind]
    whole = _whole(kind, run, every_e)
    want_keys = {'offset', '_ref.sample', '_ref.action', 'last.dh', 'last.accept', 'history.accept_rate',
                 'history.exp_mdh', 'history.dh_rms'}
    want_keys |= {'_ref.rung', 'last.swapped', 'history.exchange_rate'} if sampler == 'ladder' else set()
    want_keys |= {'last.cluster'} if sampler == 'plain' and every_e else set()
    want_keys |= {'rows'} if run != 'measure' else set()
    assert want_keys <= set(whole) and (run == 'sample' or 'measure[0].links' in whole)
    assert sampler != 'ladder' or run == 'sample' or f'measure[{K - 1}].links' in whole
    assert whole['last.dh'].shape == (STEPS * (N_SKIP + 1), C)
    calls, real = [], getattr(_hip, wrapper)

    def counted(*a, **k):
        calls.append(k.get('n_traj'))
        return real(*a, **k)
    monkeypatch.setattr(_hip, wrapper, counted)
    monkeypatch.setattr(_hip, constant, caps[run != 'sample'][level])
    part = _run(kind, run, every_e)
    assert len(calls) > 1 and sum(calls) == STEPS * (N_SKIP + 1), calls
    assert part.keys() == whole.keys()
    for key, want in whole.items():
        got = part[key]
        same = torch.equal(got, want) if isinstance(want, torch.Tensor) else got == want
        assert same, (key, calls)

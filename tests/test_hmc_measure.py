"""nf_phi4_hmc_measure and `HMCSampler.measure` on the device: observables taken inside the HMC launch.

The contract is bitwise.  A row of `measure` is the row nf_lattice_measure gives for the recorded configuration (the same
routine on the same LDS image by the same team), and measuring changes nothing else: phi, the action, dH and the accept
flags are nf_phi4_hmc's bits.  The lattices are the ones where the two kernels' lane maps change (the table in `LATTICES`).
Every kernel case runs 6 trajectories of 4 MD steps with record_every = 2 at an explicit Philox position, at a step
length and position picked from a fixed ladder so that the recorded trajectories hold accepted AND rejected ones (asserted): after a
reject the LDS image holds the proposal and the measurement has to come from the restored state.  An independent check
holds three of the shapes to the numpy long-double reference of tests/measure_cases.py within its double-sum bound."""
import functools

import pytest
import torch

from normflow__amd import _hip
from normflow__amd.lib import Ensemble, observables as OB

import hmc_cases as H
import measure_cases as MC
from hmc_cases import DEV, field as _field

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
_name = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v).replace("torch.", "")
N_TRAJ, EVERY, N_MD = 6, 2, 4
LATTICES = [
    ((5,), (F32, F64)),                # one axis
    ((1, 7), (F32, F64)),              # an axis of extent 1: its slice entry and the w2 fold
    ((2, 6), (F32, F64)),              # extent 2
    ((3, 3), (F32, F64)),              # the smallest packed
    ((16, 16), (F32, F64)),            # V = 256: one team wave, three idle waves
    ((17, 16), (F32, F64)),            # V = 272: 320 lanes, team 256, a ragged last wave
    ((5, 7, 9), (F32, F64)),           # three odd axes
    ((2, 3, 4, 5), (F32, F64)),        # four axes
    ((16, 16, 16), (F32, F64)),        # 4 sites per lane, 1024 lanes, team 256
    ((17, 16, 16), (F32, F64)),        # V = 4352: 8 sites per lane, 576 lanes, team 512 (fp64: measure_image out of line)
    ((24, 24, 24), (F32,)),            # 16 sites per lane
    ((8, 8, 8, 16), (F32, F64)),       # fp64: exactly 64 KiB
]
MANY = {(5,), (1, 7), (3, 3)}          # C = 300 on the three smallest: chains beyond the resident workgroups
CASES = [(lat, dt, C) for lat, dts in LATTICES for dt in dts for C in ((1, 3, 300) if lat in MANY else (1, 3))]
_id = lambda c: f"{_name(c[0])}-{_name(c[1])}-C{c[2]}"
# dH of a trajectory grows like dt^2 sqrt(V): from steps that reject nearly everything on the small lattices down to
# steps that accept nearly everything on the large ones; somewhere between, the three recorded flags differ
LADDER = (1.0, 0.8, 0.64, 0.5, 0.4, 0.32, 0.25, 0.2, 0.16, 0.125, 0.1, 0.08, 0.064, 0.05, 0.04, 0.032, 0.025)
OFFSETS = (64, 1064, 2064)             # with one chain there are three recorded flags: three positions per step length


def _launch(phi, coef, n_traj, pos, **kw):
    return H.launch(_hip.phi4_hmc, phi, coef, n_traj, pos, n_md=N_MD, **kw)


@functools.lru_cache(maxsize=None)
def _case(lattice, dtype, C):
    """(model coefficients, the start, the position, dt, the RECORDING launch's (phi, dict)): computed once per case,
    shared by the tests and never written.  (dt, position) is the first of LADDER x OFFSETS at which the recorded
    trajectories of the recording launch hold both decisions."""
    m = H.model(lattice, dtype, DEV, **H.INTERACTING)
    coef = m.hmc._coef(lattice)
    phi0 = _field((C,) + lattice, dtype, 500 + C)
    for dt in LADDER:
        for off in OFFSETS:
            pos = (0xC0FFEE + C, off)
            phi, r = _launch(phi0, coef, N_TRAJ, pos, dt=dt, record_every=EVERY)
            flags = r['accept'][EVERY - 1::EVERY]
            if 0 < int(flags.sum()) < flags.numel():
                return coef, phi0, pos, dt, phi, r
    raise AssertionError(f"no step length of {LADDER} gives both decisions on {lattice} {dtype} C={C}")


def _eq(a, b):
    """Bit for bit: the dH of a trajectory that overflowed at the top of the ladder is a NaN, which equals its own bits."""
    if a.is_floating_point():
        bits = {F32: torch.int32, F64: torch.int64}[a.dtype]
        return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(bits), b.contiguous().view(bits))
    return torch.equal(a, b)


def _same_run(a, b, phi_a, phi_b):
    assert _eq(phi_a, phi_b)
    for key in ('action', 'dh', 'accept'):
        assert _eq(a[key], b[key]), key


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_measure_in_the_launch_is_measure_of_the_record(case):
    lattice, dtype, C = case
    coef, phi0, pos, dt, phi_r, rec = _case(lattice, dtype, C)
    flags = rec['accept'][EVERY - 1::EVERY]
    print(f"{_id(case)}: dt {dt} at offset {pos[1]}, recorded trajectories accepted {int(flags.sum())} of {flags.numel()}")
    assert 0 < int(flags.sum()) < flags.numel()                    # the restore-then-measure branch and the other
    n_out = _hip.measure_plan(lattice, dtype)['n_out']
    want = _hip.lattice_measure(rec['record'].flatten(0, 1)).reshape(N_TRAJ // EVERY, C, n_out)
    # measuring alone: no rows
    phi_m, mea = _launch(phi0, coef, N_TRAJ, pos, dt=dt, record_every=EVERY, measure=True, record=False)
    assert mea['record'] is None and mea['measure'].dtype == F64 and mea['measure'].shape == want.shape
    assert _eq(mea['measure'], want)
    _same_run(mea, rec, phi_m, phi_r)
    # record and measure together give what each gives alone
    phi_b, both = _launch(phi0, coef, N_TRAJ, pos, dt=dt, record_every=EVERY, measure=True)
    assert _eq(both['record'], rec['record']) and _eq(both['measure'], want)
    _same_run(both, rec, phi_b, phi_r)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_launches_compose(case):
    """One launch of 6 trajectories == three of 2 == one of 4 and one of 2, at the offsets the first consumes."""
    lattice, dtype, C = case
    coef, phi0, pos, dt, phi_r, rec = _case(lattice, dtype, C)
    _, one = _launch(phi0, coef, N_TRAJ, pos, dt=dt, record_every=EVERY, measure=True, record=False)
    for split in ((2, 2, 2), (4, 2)):
        phi, t0, parts = phi0, 0, []
        for n in split:
            phi, r = _launch(phi, coef, n, (pos[0], pos[1] + 2 * t0), dt=dt, record_every=EVERY, measure=True, record=False)
            parts.append(r)
            t0 += n
        assert _eq(torch.cat([r['measure'] for r in parts]), one['measure']), split
        assert _eq(torch.cat([r['dh'] for r in parts]), rec['dh'])
        assert _eq(torch.cat([r['accept'] for r in parts]), rec['accept'])
        assert _eq(phi, phi_r) and _eq(parts[-1]['action'], rec['action'])


@pytest.mark.parametrize("case", [((1, 7), F64, 3), ((17, 16), F32, 3), ((17, 16, 16), F64, 1)], ids=_id)
def test_rows_against_the_reference(case, parity_report):
    lattice, dtype, C = case
    coef, phi0, pos, dt, _, rec = _case(lattice, dtype, C)
    _, mea = _launch(phi0, coef, N_TRAJ, pos, dt=dt, record_every=EVERY, measure=True, record=False)
    ref = MC.ref_measure(rec['record'].flatten(0, 1).cpu().numpy())
    res = MC.worst(MC.unpack(mea['measure'].flatten(0, 1), lattice), ref)
    for q, (err, bound) in res.items():
        parity_report(f"hmc measure {_id(case)}", q, err, bound)
        assert err <= bound, (q, err, bound)


# ------------------------------------------------------------------------------------------------------ the sampler
def _tensors(m):
    return dict(sum_phi=m.sum_phi, sum_phi2=m.sum_phi2, sum_phi4=m.sum_phi4, links=m.links, action=m.action,
                **{f"slices_{mu}": s for mu, s in enumerate(m.slices)})


def _offset():
    return torch.cuda.default_generators[DEV.index].get_offset()


def _sampler_pair(lattice, dtype, C, batch, seed, path=None, **kw):
    """`model.measure(hmc.sample())` and `hmc.measure()` from equal chain and generator state: everything they leave."""
    a, b = H.model(lattice, dtype, DEV, **H.INTERACTING), H.model(lattice, dtype, DEV, **H.INTERACTING)
    start = _field((C,) + lattice, dtype, 900 + C)
    a.hmc.start(start); b.hmc.start(start)
    torch.manual_seed(seed)
    y = a.hmc.sample(batch, n_chains=C, path=path, **kw)
    stored, end_a = a.measure(y), _offset()
    torch.manual_seed(seed)
    m = b.hmc.measure(batch, n_chains=C, path=path, **kw)
    end_b = _offset()
    assert a.hmc._choose(start, path) == b.hmc._choose(start, path)
    want, got = _tensors(stored), _tensors(m)
    assert want.keys() == got.keys() and len(m) == batch and m.lattice == lattice
    for key in want:
        assert got[key].dtype == F64 and torch.equal(got[key], want[key]), key
    for key in ('sample', 'action'):
        assert torch.equal(a.hmc._ref[key], b.hmc._ref[key]), key
    for key in ('dh', 'accept'):
        assert torch.equal(a.hmc.last[key], b.hmc.last[key]), key
    for key in ('accept_rate', 'exp_mdh', 'dh_rms'):
        assert getattr(a.hmc.history, key) == getattr(b.hmc.history, key) and len(getattr(b.hmc.history, key)) == 1
    assert end_a == end_b
    return a, b, y, m


@pytest.mark.parametrize("dtype", [F32, F64], ids=_name)
def test_sampler_fused(dtype):
    a, b, y, m = _sampler_pair((16, 16), dtype, 64, 64 * 5, seed=31, n_md=5, dt=0.2, n_skip=1)
    assert a.hmc._choose(a.hmc._ref['sample'], None) == 'fused'
    assert 0 < a.hmc.history.accept_rate[-1] < 1
    # the rows on request are the sampler's rows, and the next call continues the chains
    torch.manual_seed(32)
    y2 = a.hmc.sample(64 * 2, n_chains=64, n_md=5, dt=0.2)
    torch.manual_seed(32)
    m2, rows = b.hmc.measure(64 * 2, n_chains=64, n_md=5, dt=0.2, return_rows=True)
    assert torch.equal(rows, y2) and torch.equal(m2.sum_phi2, a.measure(y2).sum_phi2)
    e = Ensemble(m, n_chains=64)
    assert e.steps == 5 and torch.equal(e.series('sum_phi')[:, :, 0], m.sum_phi.reshape(5, 64).cpu())


def test_sampler_fused_split_under_the_work_cap(monkeypatch):
    """With the cap lowered on the host side the run is split into several measuring launches, and where one recorded
    step is more than a launch into plain launches and a measuring one: the same bits either way."""
    lattice, C, kw = (16, 16), 8, dict(n_md=5, dt=0.2, n_skip=2)
    whole = _sampler_pair(lattice, F32, C, C * 4, seed=41, **kw)[3]
    for cap in (256 * 40, 256 * 14):          # 40 MD steps: one recorded step (15 + 16) per launch; 14: 2 plain trajectories + 1 measured
        monkeypatch.setattr(_hip, 'HMC_MAX_WORK', cap)
        part = _sampler_pair(lattice, F32, C, C * 4, seed=41, **kw)[3]
        for key, t in _tensors(whole).items():
            assert torch.equal(_tensors(part)[key], t), (cap, key)


def test_sampler_tiled_segmented():
    lattice = (12, 12, 12, 12)
    assert not _hip.hmc_supported(lattice, F64) and _hip.measure_plan(lattice, F64)['regime'] == 'segmented'
    a, _, _, _ = _sampler_pair(lattice, F64, 3, 3 * 2, seed=33, n_md=3, dt=0.05, n_skip=1)
    assert a.hmc._choose(a.hmc._ref['sample'], None) == 'tiled'


def test_sampler_tiled_bricks():
    lattice = (32, 32, 32, 32)
    a, _, y, _ = _sampler_pair(lattice, F64, 1, 2, seed=34, n_md=2, dt=0.02)
    assert a.hmc._choose(a.hmc._ref['sample'], None) == 'tiled' and OB.route(y) == 'tiled'


def test_sampler_composed_on_the_device():
    _sampler_pair((5, 7, 9), F64, 3, 3 * 3, seed=35, path='composed', n_md=4, dt=0.1, n_skip=1)


def test_no_rows_are_allocated():
    """(16, 16, 16) fp32, 64 chains, 64 recorded steps: the rows would be 64 MiB.  The statistics are under 2 MiB (twice:
    the launch's and the sampler's) and the copy of the chains 1 MiB, so a quarter of the rows is a cap with room -- a
    condition, not a measurement."""
    lattice, C, steps = (16, 16, 16), 64, 64
    m = H.model(lattice, F32, DEV, **H.INTERACTING)
    m.hmc.start(_field((C,) + lattice, F32, 77))
    torch.manual_seed(36)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(DEV)
    before = torch.cuda.memory_allocated(DEV)
    got = m.hmc.measure(C * steps, n_chains=C, n_md=3, dt=0.05)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated(DEV) - before
    rows = C * steps * 16 ** 3 * 4
    print(f"peak rise {rise / 2 ** 20:.2f} MiB against {rows / 2 ** 20:.0f} MiB of rows")
    assert len(got) == C * steps and rise < rows // 4

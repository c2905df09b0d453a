"""Integration schemes on the device: nf_phi4_hmc_scheme and nf_phi4_hmc_tiled_scheme against the fp64 restatement of
tests/hmc_integrator_cases.py, and the bitwise identities the schemes must keep.

Every case runs n_md = 4 steps of dt = 0.1 on the smallest lattices where the fused kernel's lane map and the tiled
kernel's regime change.  The inputs are fp32-representable, so one restated trajectory per case serves both dtypes.
fp64: phi and pi within 1e-11 of the largest entry, dH within 1e-9, the same decisions away from ties.  fp32: 4 x the
error of the composed path in fp32 on the same inputs (hmc_cases.fp32_bounds)."""
import functools

import numpy as np
import pytest
import torch

from normflow__amd import _hip

import hmc_cases as H
import hmc_integrator_cases as I
import ladder_cases as Lc
from hmc_cases import DEV, field as _field, rel as _rel

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
N_MD, DT = 4, 0.1
SCHEMES = ['omelyan', 'omf4', 'yoshida']
FUSED = [(lat, C) for lat in [(5,), (2, 6), (17, 16), (3, 4, 5), (2, 3, 4, 5), (16, 16, 16)] for C in (1, 300)]
TILED = [(lat, 3) for lat in [(1, 7), (3, 3), (5, 7, 9), (9, 3, 4), (2, 3, 4, 5)]] + [((40, 40, 24), 2)]
_name = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v).replace("torch.", "")
_case = lambda v: f"{_name(v[0])}-C{v[1]}"


@functools.lru_cache(maxsize=None)
def _inputs(lattice, C):
    """(phi0, pi0) in fp32 on the device."""
    return _field((C,) + lattice, F32, 100 + C), _field((C,) + lattice, F32, 300 + C, scale=1.0)


@functools.lru_cache(maxsize=None)
def _reference(lattice, C, scheme):
    """The restated trajectory of the case, computed once and left alone: dict(phi, pi, dh) fp64 on the device."""
    phi0, pi0 = _inputs(lattice, C)
    action = H.model(lattice, F64, DEV, **H.INTERACTING).action
    phi, pi, dh = I.ref_trajectory(phi0, pi0, action, N_MD, DT, I.WEIGHTS[scheme])
    return dict(phi=phi.to(DEV), pi=pi.to(DEV), dh=dh.to(DEV))


def _against_the_restatement(path, lattice, C, scheme, dtype, parity_report):
    phi0, pi0 = _inputs(lattice, C)
    ref = _reference(lattice, C, scheme)
    m = H.model(lattice, dtype, DEV, **H.INTERACTING)
    pos = (0x51C0 + C, 24)
    run = lambda p, force: m.hmc.trajectory(phi0.to(dtype), N_MD, DT, pi=pi0.to(dtype), force_accept=force, path=p,
                                            position=pos, integrator=I.INTEGRATORS[scheme])
    k = run(path, True)
    name = f"hmc {scheme} {path} {_name(dtype)} {_name(lattice)} C={C}"
    assert k['phi'].dtype == dtype and k['dh'].dtype == F64 and bool(k['accept'].all())
    if dtype == F32:
        H.fp32_bounds(name, k, run('composed', True), ref, parity_report)
        return
    for key in ('phi', 'pi'):
        err = _rel(k[key], ref[key])
        parity_report(name, key, err, 1e-11)
        assert err <= 1e-11, (name, key, err)
    e_dh = (k['dh'] - ref['dh']).abs().max().item()
    parity_report(name, 'dH (abs)', e_dh, 1e-9)
    assert e_dh <= 1e-9, (name, e_dh)
    # the decisions: the documented rule on the restated uniform and the restated dH, away from ties
    d = run(path, False)
    logu, dh = H.log_uniforms(pos[0], pos[1] + 1, C), ref['dh'].cpu().numpy()
    clear = np.abs(logu + dh) > 1e-6
    assert (~clear).sum() <= max(1, 0.02 * C)
    got = d['accept'].cpu().numpy().astype(bool)
    assert np.array_equal(got[clear], (logu < -dh)[clear])
    keep = torch.as_tensor(~got, device=DEV)
    assert torch.equal(d['phi'][keep], phi0.to(dtype)[keep])              # rejected: the old bits


@pytest.mark.parametrize("dtype", [F64, F32], ids=_name)
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("case", FUSED, ids=_case)
def test_fused_against_the_restatement(case, scheme, dtype, parity_report):
    _against_the_restatement('fused', *case, scheme, dtype, parity_report)


@pytest.mark.parametrize("dtype", [F64, F32], ids=_name)
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("case", TILED, ids=_case)
def test_tiled_against_the_restatement(case, scheme, dtype, parity_report):
    _against_the_restatement('tiled', *case, scheme, dtype, parity_report)


# ---------------------------------------------------------------------------------------------- bitwise identities
def _same(a, b, keys=('action', 'dh', 'accept', 'record', 'measure', 'pi')):
    for key in keys:
        if key in a or key in b:
            x, y = a.get(key), b.get(key)
            assert (x is None and y is None) or torch.equal(x, y), key


def _ladder(lattice, dtype, K, C):
    m, ladder = Lc.model(lattice, dtype, DEV, **Lc.DISTINCT(K))
    coef = ladder.coef_table(lattice, DEV)
    rung = Lc.permuted_rung(C // K, K, 7, device=DEV)
    return m, coef, rung


ENTRY_KINDS = ['fused', 'measure', 'ladder', 'tiled', 'tiled-ladder']


@pytest.mark.parametrize("dtype", [F32, F64], ids=_name)
@pytest.mark.parametrize("kind", ENTRY_KINDS)
def test_scheme_entries_with_leapfrog_or_null_are_the_old_entries(kind, dtype):
    lattice, C, K = (6, 6), 6, 3
    m, coef, rung = _ladder(lattice, dtype, K, C)
    phi0 = _field((C,) + lattice, dtype, 700)
    wrapper = dict(fused=_hip.phi4_hmc, measure=_hip.phi4_hmc, ladder=_hip.phi4_hmc_ladder, tiled=_hip.phi4_hmc_tiled)
    wrapper['tiled-ladder'] = _hip.phi4_hmc_tiled_ladder
    couplings = (coef, rung) if 'ladder' in kind else m.hmc._coef(lattice)
    kw = dict(measure=True) if kind in ('measure', 'ladder') else {}

    def run(**extra):
        phi = phi0.clone()
        r = wrapper[kind](phi, *couplings, 3, 0.15, n_traj=4, record_every=2, want_pi=True, position=(321, 8), **kw, **extra)
        return phi, r
    phi_old, old = run()
    assert 0 < int(old['accept'].sum()) and ('measure' in old) == bool(kw)
    for scheme in ('leapfrog', _hip.hmc_scheme(I.SCHEMES['leapfrog']), _hip.NULL_SCHEME):
        phi_new, new = run(scheme=scheme)
        assert torch.equal(phi_new, phi_old), scheme
        _same(old, new)
    phi_mn, mn = run(scheme='omelyan')                                   # and another scheme is another trajectory
    assert not torch.equal(mn['dh'], old['dh'])


@pytest.mark.parametrize("scheme", ['omelyan', 'omf4'])
@pytest.mark.parametrize("lattice", [(16, 16), (5, 7, 9), (2, 3, 4, 5)], ids=_name)
def test_fused_is_tiled_in_fp64(lattice, scheme, parity_report):
    """The same update lengths, formed once on the host, on both paths: the fields agree bit for bit; the energies are
    summed in another order (lanes and waves against tiles), so dH agrees to the rounding of the sums."""
    C = 5
    m = H.model(lattice, F64, DEV, **H.INTERACTING)
    phi0 = _field((C,) + lattice, F64, 150)
    run = lambda path: m.hmc.trajectory(phi0, N_MD, DT, force_accept=True, path=path, position=(991, 12), integrator=scheme)
    f, t = run('fused'), run('tiled')
    e_dh = (f['dh'] - t['dh']).abs().max().item()
    parity_report(f"hmc {scheme} fused vs tiled fp64 {_name(lattice)}", 'dH (abs)', e_dh, 1e-9)
    assert torch.equal(f['phi'], t['phi']) and torch.equal(f['pi'], t['pi'])
    assert e_dh <= 1e-9


@pytest.mark.parametrize("dtype", [F32, F64], ids=_name)
@pytest.mark.parametrize("path", ['fused', 'tiled'])
def test_three_trajectories_in_one_launch(path, dtype):
    lattice, C = (6, 6), 5
    m = H.model(lattice, dtype, DEV, **H.INTERACTING)
    coef = m.hmc._coef(lattice)
    kernel = _hip.phi4_hmc if path == 'fused' else _hip.phi4_hmc_tiled
    phi0 = _field((C,) + lattice, dtype, 400)
    seed, off = 99, 1000
    phi_a, a = H.launch(kernel, phi0, coef, 3, (seed, off), record_every=1, scheme='omf4', dt=0.3)
    phi_b, dh, acc, rec = phi0, [], [], []
    for t in range(3):
        phi_b, b = H.launch(kernel, phi_b, coef, 1, (seed, off + 2 * t), scheme='omf4', dt=0.3)
        dh.append(b['dh'][0]); acc.append(b['accept'][0]); rec.append(phi_b)
    assert torch.equal(phi_a, phi_b) and torch.equal(a['record'], torch.stack(rec))
    assert torch.equal(a['dh'], torch.stack(dh)) and torch.equal(a['accept'], torch.stack(acc))
    assert torch.equal(a['action'], b['action'])


@pytest.mark.parametrize("scheme", ['omelyan', 'omf4'])
@pytest.mark.parametrize("path", ['fused', 'tiled'])
def test_ladder_is_the_plain_kernel_rung_by_rung(path, scheme):
    lattice, C, K = (6, 6), 6, 3
    m, coef, rung = _ladder(lattice, F32, K, C)
    phi0 = _field((C,) + lattice, F32, 800)
    plain = _hip.phi4_hmc if path == 'fused' else _hip.phi4_hmc_tiled
    ladder = _hip.phi4_hmc_ladder if path == 'fused' else _hip.phi4_hmc_tiled_ladder
    kw = dict(n_traj=3, record_every=1, position=(55, 4), scheme=scheme)
    phi_l = phi0.clone()
    l = ladder(phi_l, coef, rung, N_MD, 0.2, **kw)
    chains = torch.arange(C, device=DEV)
    col = (chains // K) * K + rung.long()
    for k in range(K):
        phi_p = phi0.clone()
        p = plain(phi_p, *coef[k].tolist(), N_MD, 0.2, **kw)
        on = rung == k                                                    # the chains that hold rung k
        assert int(on.sum()) == C // K
        assert torch.equal(phi_l[on], phi_p[on]) and torch.equal(l['action'][on], p['action'][on])
        for key in ('dh', 'accept', 'record'):
            assert torch.equal(l[key][:, col[on]], p[key][:, on]), (k, key)


def _measurement(m):
    return [m.sum_phi, m.sum_phi2, m.sum_phi4, m.links, m.action] + list(m.slices)


@pytest.mark.parametrize("lattice,path", [((6, 6), 'fused'), ((8, 8), 'tiled')], ids=["fused", "tiled"])
def test_measure_is_measure_of_the_sampled_rows(lattice, path):
    C, n = 3, 4
    m = H.model(lattice, F32, DEV, **H.INTERACTING)
    phi0 = _field((C,) + lattice, F32, 900)
    kw = dict(n_chains=C, n_md=3, dt=0.2, n_skip=1, path=path, integrator='omf4')
    torch.manual_seed(5)
    y = m.hmc.start(phi0).sample(n * C, **kw)
    want, last = m.measure(y), m.hmc.last
    torch.manual_seed(5)
    got = m.hmc.start(phi0).measure(n * C, **kw)
    assert all(torch.equal(a, b) for a, b in zip(_measurement(got), _measurement(want)))
    assert m.hmc.last['integrator'] == last['integrator'] == 'omf4' and torch.equal(m.hmc.last['dh'], last['dh'])


def _sampler_run(kind, path, run):
    """Everything one call with 2MN leaves; `kind` plain or ladder."""
    lattice, K = (6, 6), 2
    if kind == 'plain':
        C, s, kw = 3, H.model(lattice, F32, DEV, **H.INTERACTING).hmc, {}
    else:
        m, ladder = Lc.model(lattice, F32, DEV, **Lc.DISTINCT(K))
        C, s, kw = 4, m.hmc.ladder(ladder), dict(exchange_every=2)
    s.start(_field((C,) + lattice, F32, 1700))
    torch.manual_seed(17)
    kw.update(n_chains=C, n_md=2, dt=0.15, n_skip=1, path=path, integrator='omelyan')
    left = {}
    if run == 'sample':
        left['rows'] = s.sample(6 * C, **kw)
    else:
        got = s.measure(6 * C, **kw)
        for k, m in enumerate(got if kind == 'ladder' else [got]):
            left.update({f"measure[{k}].{i}": t for i, t in enumerate(_measurement(m))})
    left['offset'] = torch.cuda.default_generators[DEV.index].get_offset()
    left.update({f"_ref.{key}": t for key, t in s._ref.items()})
    left.update({f"last.{key}": t for key, t in s.last.items()})
    left.update({f"history.{key}": repr(getattr(s.history, key)) for key in s.history._KEYS})
    return left


@functools.lru_cache(maxsize=None)
def _whole(kind, path, run):
    return _sampler_run(kind, path, run)


# a recorded step is 2 trajectories of n_md s = 4 force evaluations (2MN), and 16 more where the launch measures; a tiled
# trajectory is 4 + 2 = 6 launches.  The caps: two recorded steps, one, one trajectory per launch.
SPLIT_CAPS = {('fused', 'sample'): (256 * 16, 256 * 8, 256 * 4), ('fused', 'measure'): (256 * 48, 256 * 24, 256 * 5),
              ('tiled', 'sample'): (24, 12, 6), ('tiled', 'measure'): (24, 12, 6)}


@pytest.mark.parametrize("level", (0, 1, 2), ids=("two-steps", "one-step", "one-trajectory"))
@pytest.mark.parametrize("run", ['sample', 'measure'])
@pytest.mark.parametrize("path", ['fused', 'tiled'])
@pytest.mark.parametrize("kind", ['plain', 'ladder'])
def test_split_run_is_the_whole_run(kind, path, run, level, monkeypatch):
    whole = _whole(kind, path, run)
    assert whole['last.integrator'] == 'omelyan' and whole['last.dh'].shape[0] == 12
    wrapper = 'phi4_hmc' + ('_tiled' if path == 'tiled' else '') + ('_ladder' if kind == 'ladder' else '')
    calls, real = [], getattr(_hip, wrapper)

    def counted(*a, **k):
        assert k['scheme'].name == 'omelyan'
        calls.append(k.get('n_traj'))
        return real(*a, **k)
    monkeypatch.setattr(_hip, wrapper, counted)
    monkeypatch.setattr(_hip, 'HMC_MAX_WORK' if path == 'fused' else 'HMC_TILED_MAX_LAUNCHES', SPLIT_CAPS[path, run][level])
    part = _sampler_run(kind, path, run)
    assert len(calls) > 1 and sum(calls) == 12, calls
    assert part.keys() == whole.keys()
    for key, want in whole.items():
        got = part[key]
        assert torch.equal(got, want) if isinstance(want, torch.Tensor) else got == want, (key, calls)


@pytest.mark.parametrize("scheme", ['omelyan', 'omf4'])
@pytest.mark.parametrize("path", ['fused', 'tiled'])
def test_reject_and_restore(path, scheme):
    """dt = 1.5: the integrator is unstable and dH enormous (or not a number); the rejected chains keep their bits."""
    lattice, C = (16, 16), 40
    m = H.model(lattice, F32, DEV, **H.INTERACTING)
    phi0 = _field((C,) + lattice, F32, 500, scale=0.05)
    kernel = _hip.phi4_hmc if path == 'fused' else _hip.phi4_hmc_tiled
    phi, r = H.launch(kernel, phi0, m.hmc._coef(lattice), 1, (5, 0), n_md=20, dt=1.5, scheme=scheme)
    rej = r['accept'][0] == 0
    assert int(rej.sum()) >= C // 2, "dt = 1.5 should reject nearly everything"
    assert torch.equal(phi[rej], phi0[rej])
    s0 = H.ref_action(phi0.double().cpu(), m.action)
    assert ((r['action'].cpu() - s0).abs() / s0.abs().clamp_min(1.0))[rej.cpu()].max().item() <= 1e-12


def test_graph_replay_is_the_eager_launch():
    lattice, C = (16, 16), 8
    m = H.model(lattice, F32, DEV, **H.INTERACTING)
    coef = m.hmc._coef(lattice)
    phi0 = _field((C,) + lattice, F32, 1100)
    kw = dict(n_traj=3, record_every=1, position=(808, 16), scheme=_hip.hmc_scheme('omelyan'))
    phi_e = phi0.clone()
    e = _hip.phi4_hmc(phi_e, *coef, N_MD, 0.2, **kw)
    static = phi0.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        r = _hip.phi4_hmc(static, *coef, N_MD, 0.2, **kw)
    torch.cuda.synchronize()
    assert torch.equal(static, phi0)                                     # capture ran nothing
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(static, phi_e) and torch.equal(r['record'], e['record'])
    assert torch.equal(r['dh'], e['dh']) and torch.equal(r['accept'], e['accept']) and torch.equal(r['action'], e['action'])


# ---------------------------------------------------------------------------------------------- statistics
def test_free_field_distribution_omelyan_fp32():
    torch.manual_seed(13)
    m = H.model((16,), F32, DEV, **H.FREE)
    y = m.hmc.sample(256 * 160, n_chains=256, n_md=2, dt=0.6, path='fused', integrator='omelyan')
    mean, err = H.chain_stats(y, 256, drop=30)
    rate = m.hmc.history.accept_rate[-1]
    print(f"free field, 2MN fp32: <phi^2> {mean:.5f} +- {err:.5f} ({(mean - H.FREE_PHI2) / err:+.2f} sigma), accept rate {rate:.3f}")
    assert m.hmc.last['integrator'] == 'omelyan'
    assert abs(mean - H.FREE_PHI2) <= 5 * err
    assert 0.5 < rate < 0.9999

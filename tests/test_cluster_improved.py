"""nf_cluster_moments on the device against the numpy restatement (tests/improved_cases.py): the clusters' fixed-point sums
and the status bit for bit, the sums of squares within the stated bound; the bitwise properties (repeat, permutation, a
chain alone, graph replay); the composed path on the device; the refused inputs; the exact
free-field values; and `measure(improved=True)` of the fused and the ladder sampler."""
import math

import numpy as np
import pytest
import torch

from normflow__amd import _hip
from normflow__amd.action import ScalarPhi4Action, ScalarPhi4Ladder
from normflow__amd.lib import observables as ob
from normflow__amd.mcmc.cluster import cluster_moments

import hmc_cases as H
import improved_cases as Ic

pytestmark = pytest.mark.gpu
DEV = H.DEV
F32, F64 = torch.float32, torch.float64
MAX_CHAINS = max(Ic.CHAINS)
_CASES = {}


def case(lat, dt):
    """MAX_CHAINS chains of the case, chain i with the label kind i % 6 (the two sweeps are nf_phi4_cluster's, of an ordered
    field at kappa = 0.67 and of a disordered one at kappa = 0.25), and their restatement: computed once, never changed."""
    key = (lat, dt)
    if key not in _CASES:
        V = Ic.volume(lat)
        phi = Ic.field(lat, dt, MAX_CHAINS)
        phi[0::6] = Ic.field(lat, dt, MAX_CHAINS, ordered=True)[0::6]
        labels = np.zeros((MAX_CHAINS, V), dtype=np.int32)
        for i, kind in enumerate(Ic.KINDS):
            n = len(range(i, MAX_CHAINS, 6))
            if kind.startswith('sweep'):
                w0 = ScalarPhi4Action(kappa=0.67 if kind == 'sweep67' else 0.25, m_sq=-2.68, lambd=0.5).get_coef(len(lat))[0]
                p = torch.from_numpy(phi[i::6].copy()).to(DEV).reshape((n,) + tuple(lat))
                r = _hip.phi4_cluster(p, w0, position=(77, 10 + i), want_labels=True)
                assert (r['stats'][:, 3] >= 1).all()
                labels[i::6] = r['labels'].reshape(n, V).cpu().numpy()
            else:
                labels[i::6] = Ic.synthetic_labels(kind, n, V)
        ref = Ic.restate(phi, labels, lat, _hip.twiddle_table(lat).numpy())
        assert (ref['status'] == 0).all()
        for a in (phi, labels, ref['moments'], ref['out'], ref['bound'], ref['status']):
            a.setflags(write=False)
        _CASES[key] = dict(phi=phi, labels=labels, ref=ref)
    return _CASES[key]


def _dev(c, lat, rows):
    shape = (len(rows),) + tuple(lat)
    return (torch.from_numpy(c['phi'][rows].copy()).to(DEV).reshape(shape),
            torch.from_numpy(c['labels'][rows].copy()).to(DEV).reshape(shape))


def _ref_rows(ref, rows):
    return {k: ref[k][rows] for k in ('moments', 'status', 'out', 'bound')}


def _host(r):
    return r['out'].cpu().numpy(), r['status'].cpu().numpy(), None if r['moments'] is None else r['moments'].cpu().numpy()


@pytest.mark.parametrize("C", Ic.CHAINS)
@pytest.mark.parametrize("lat,dt", Ic.CASES, ids=[Ic.case_id(c) for c in Ic.CASES])
def test_kernel_equals_the_restatement(lat, dt, C, parity_report):
    c = case(lat, dt)
    rows = np.arange(C)
    phi, labels = _dev(c, lat, rows)
    before = phi.clone()
    r = _hip.cluster_moments(phi, labels, want_moments=True)
    assert torch.equal(phi, before)
    assert r['out'].dtype == F64 and tuple(r['out'].shape) == (C, 2 + len(lat)) and r['status'].dtype == torch.int32
    assert r['moments'].dtype == torch.int64 and tuple(r['moments'].shape) == (C,) + tuple(lat)
    Ic.check_against(f"kernel {Ic.case_id((lat, dt))} C={C}", *_host(r), _ref_rows(c['ref'], rows), lat,
                     parity_report if C == MAX_CHAINS else None)
    assert _hip.cluster_moments(phi, labels)['moments'] is None


@pytest.mark.parametrize("lat,dt", Ic.CASES, ids=[Ic.case_id(c) for c in Ic.CASES])
def test_same_bits_on_repeat_under_permutation_and_alone(lat, dt):
    c = case(lat, dt)
    rows = np.arange(14)
    phi, labels = _dev(c, lat, rows)
    a = _hip.cluster_moments(phi, labels, want_moments=True)
    b = _hip.cluster_moments(phi, labels, want_moments=True)
    for k in ('out', 'status', 'moments'):
        assert torch.equal(a[k], b[k]), k
    perm = torch.from_numpy(np.random.default_rng(3).permutation(len(rows))).to(DEV)
    p = _hip.cluster_moments(phi[perm].contiguous(), labels[perm].contiguous(), want_moments=True)
    for k in ('out', 'status', 'moments'):
        assert torch.equal(a[k][perm], p[k]), k
    for i in (0, 4, 11):                                     # a sweep's chain, the two alternating keys, a random one: alone
        one = _hip.cluster_moments(phi[i:i + 1].contiguous(), labels[i:i + 1].contiguous(), want_moments=True)
        for k in ('out', 'status', 'moments'):
            assert torch.equal(a[k][i:i + 1], one[k]), (k, i)


GRAPH = [((16, 16), 'float32'), ((16, 16, 16), 'float64'), ((128, 128), 'float32')]


@pytest.mark.parametrize("lat,dt", GRAPH, ids=[Ic.case_id(c) for c in GRAPH])
def test_graph_replay_equals_eager(lat, dt):
    c = case(lat, dt)
    phi, labels = _dev(c, lat, np.arange(7))
    eager = _hip.cluster_moments(phi, labels, want_moments=True)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        r = _hip.cluster_moments(phi, labels, want_moments=True)
    g.replay()
    torch.cuda.synchronize()
    for k in ('out', 'status', 'moments'):
        assert torch.equal(eager[k], r[k]), k


@pytest.mark.parametrize("lat,dt", Ic.CASES, ids=[Ic.case_id(c) for c in Ic.CASES])
def test_kernel_equals_the_composed_path_on_the_device(lat, dt):
    c = case(lat, dt)
    rows = np.arange(13)
    phi, labels = _dev(c, lat, rows)
    k = _hip.cluster_moments(phi, labels, want_moments=True)
    o = cluster_moments(phi, labels, want_moments=True)
    assert o['out'].is_cuda and torch.equal(k['moments'], o['moments']) and torch.equal(k['status'], o['status'])
    ref = _ref_rows(c['ref'], rows)
    Ic.check_against(f"composed on the device {Ic.case_id((lat, dt))}", *_host(o), ref, lat)
    bound = torch.from_numpy(ref['bound'][:, Ic.columns(lat)]).to(DEV)
    assert ((k['out'] - o['out']).abs() <= 2 * bound).all()
    assert ob.route_improved(phi) == 'kernel'
    m = ob.measure_improved(phi, labels)
    assert torch.equal(m.out, k['out']) and torch.equal(m.status, k['status'])


REFUSALS = [("nan", 'float32', float('nan'), None), ("inf", 'float64', float('inf'), None), ("2^16", 'float32', 2.0 ** 16, None),
            ("-2^16", 'float64', -2.0 ** 16, None), ("label -1", 'float32', None, -1), ("label V", 'float64', None, 256)]


@pytest.mark.parametrize("name,dt,value,label", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refused_inputs_on_the_device(name, dt, value, label):
    """The guard is part of the ABI: the chain is refused before any slot is indexed.  The same inputs go through the
    composed path first, which never indexes with them either."""
    lat = (16, 16)
    c = case(lat, dt)
    rows = np.arange(3)
    phi, labels = c['phi'][rows].copy(), c['labels'][rows].copy()
    if value is not None:
        phi[1, 77] = value
    else:
        labels[1, 77] = label
    ref = Ic.restate(phi, labels, lat, _hip.twiddle_table(lat).numpy())
    assert ref['status'].tolist() == [0, 1, 0]
    shape = (3,) + lat
    dphi, dlab = torch.from_numpy(phi).to(DEV).reshape(shape), torch.from_numpy(labels).to(DEV).reshape(shape)
    o = cluster_moments(dphi, dlab, want_moments=True)
    Ic.check_against(f"composed, {name}", *_host(o), ref, lat)
    k = _hip.cluster_moments(dphi, dlab, want_moments=True)
    Ic.check_against(f"kernel, {name}", *_host(k), ref, lat)
    assert torch.isnan(k['out'][1]).all() and (k['moments'][1] == 0).all()
    good = _ref_rows(c['ref'], rows)
    for i in (0, 2):                                         # the neighbours are what they were
        assert np.array_equal(k['moments'][i].cpu().numpy().reshape(-1), good['moments'][i])


def test_largest_values_in_range():
    lat = (16, 16)
    for dt in Ic.DTYPES:
        c = case(lat, dt)
        phi, labels = c['phi'][:2].copy(), c['labels'][:2].copy()
        phi[1, 3] = np.nextafter(np.array(2.0 ** 16, dtype=dt), np.array(0, dtype=dt))
        phi[1, 4] = -phi[1, 3]
        labels[1, 3] = 255
        ref = Ic.restate(phi, labels, lat, _hip.twiddle_table(lat).numpy())
        assert ref['status'].tolist() == [0, 0]
        shape = (2,) + lat
        k = _hip.cluster_moments(torch.from_numpy(phi).to(DEV).reshape(shape), torch.from_numpy(labels).to(DEV).reshape(shape),
                                 want_moments=True)
        Ic.check_against(f"edge of the range {dt}", *_host(k), ref, lat)


def test_wrapper_refuses_what_it_cannot_take():
    phi = torch.zeros((2, 4, 4), dtype=F32, device=DEV)
    with pytest.raises(_hip.NormflowHipError, match="labels"):
        _hip.cluster_moments(phi, torch.zeros((2, 4, 4), dtype=torch.int64, device=DEV))
    with pytest.raises(_hip.NormflowHipError, match="class"):
        _hip.cluster_moments(torch.zeros((1, 32, 32, 32), dtype=F32, device=DEV),
                             torch.zeros((1, 32, 32, 32), dtype=torch.int32, device=DEV))
    big = torch.zeros((1, 32, 32, 32), dtype=F32, device=DEV)
    assert ob.route_improved(big) == 'composed'
    with pytest.raises(_hip.NormflowHipError):
        ob.measure_improved(big, torch.zeros(big.shape, dtype=torch.int32, device=DEV), path='kernel')


# ---------------------------------------------------------------- the samplers on the device
def _bound_of(rows, V):
    """Every term of the sums of squares is >= 0, so sum |terms| is the sum: twice the bound, for two computed values."""
    return 2 * (V + 8) * 2.0 ** -53 * rows.abs()


def test_free_field_exactness():
    """lambda = 0: V <m^2> = 1 / m^2 and <|phi~(p_min)|^2> / V = 1 / (m^2 + 2 kappa (1 - cos(2 pi / 8))), exactly."""
    lat, C, drop, steps = (8, 8), 256, 60, 160
    m = H.model(lat, F64, DEV, **H.FREE)
    torch.manual_seed(5)
    m.hmc.start(n_chains=C)
    got = m.hmc.measure(C * (drop + steps), n_chains=C, n_md=10, dt=0.1, cluster_every=1, improved=True)
    assert (got.improved.status == 0).all()
    e = ob.ImprovedEnsemble(got.improved, n_chains=C, drop=drop)
    chi, chi_err = e.susceptibility()
    g1, g1_err = e.propagator1()
    want_chi = 1 / H.FREE['m_sq']
    want_g1 = 1 / (H.FREE['m_sq'] + 2 * H.FREE['kappa'] * (1 - math.cos(2 * math.pi / 8)))
    pchi, pchi_err = ob.Ensemble(got, n_chains=C, drop=drop).mean('m2')
    print(f"V<m^2> improved {chi:.5f} +- {chi_err:.5f} (plain {64 * pchi:.5f} +- {64 * pchi_err:.5f}), exact {want_chi:.5f}; "
          f"G(p_min) improved {g1:.5f} +- {g1_err:.5f}, exact {want_g1:.5f}")
    assert abs(chi - want_chi) <= 5 * chi_err and abs(g1 - want_g1) <= 5 * g1_err
    assert chi_err < 0.05 * want_chi and g1_err < 0.05 * want_g1


def _state(s):
    return (s._ref['sample'].clone(), s._ref['action'].clone(), {k: v.clone() for k, v in s.last.items()},
            [list(getattr(s.history, k)) for k in type(s.history)._KEYS], torch.cuda.default_generators[0].get_offset())


def _same_state(a, b):
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[3] == b[3] and a[4] == b[4]
    assert set(a[2]) == set(b[2])
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k


@pytest.mark.parametrize("dt", [F32, F64], ids=['float32', 'float64'])
def test_fused_sampler_improved_changes_nothing_else(dt):
    lat, C = (8, 8), 5
    m = H.model(lat, dt, DEV, **H.INTERACTING)
    runs = {}
    for improved in (False, True, 'composed'):
        torch.manual_seed(9)
        m.hmc.history.reset_history()
        m.hmc.start(n_chains=C)
        got = m.hmc.measure(C * 6, n_chains=C, n_md=5, dt=0.1, cluster_every=2, improved=improved)
        runs[improved] = (got, _state(m.hmc))
    plain, with_kernel, with_composed = runs[False], runs[True], runs['composed']
    for other in (with_kernel, with_composed):
        _same_state(plain[1], other[1])
        for key in ('sum_phi', 'sum_phi2', 'sum_phi4', 'links', 'action'):
            assert torch.equal(getattr(plain[0], key), getattr(other[0], key)), key
    assert plain[0].improved is None
    k, o = with_kernel[0].improved, with_composed[0].improved
    assert len(k) == 3 * C and tuple(k.prop1.shape) == (3 * C, 2) and k.out.is_cuda and (k.status == 0).all()
    assert torch.equal(k.status, o.status) and ((k.out - o.out).abs() <= _bound_of(o.out, 64)).all()
    assert not torch.equal(k.out[:C], k.out[C:2 * C])                     # row s C + c: the sweeps differ
    # what ran was the fused HMC kernel, nf_phi4_cluster and nf_cluster_moments
    chains = m.hmc._ref['sample']
    assert m.hmc._choose(chains, None) == 'fused' and m.hmc._sweep_path(chains) == 'kernel'
    assert ob.route_improved(chains) == 'kernel'


def _synchronising_calls(fn):
    """How often torch reports a synchronising call while fn runs (torch.cuda.set_sync_debug_mode('warn'))."""
    import warnings
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")               # itself warns once that the mode is a prototype
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode(prev)
    texts = [str(w.message).lower() for w in seen]
    return sum(1 for t in texts if "synchroniz" in t and "prototype" not in t)


@pytest.mark.parametrize("which", ["fused", "ladder"])
def test_improved_adds_no_device_to_host_read(which):
    """Still one read per call: with improved=True torch reports as many synchronising calls as without, and at least the
    one that fills `history`."""
    lat = (8, 8)
    m = H.model(lat, F32, DEV, **H.INTERACTING)
    if which == "fused":
        s, C, kw = m.hmc, 4, {}
    else:
        s, C, kw = m.hmc.ladder(ScalarPhi4Ladder(kappa=(0.3, 0.5, 0.67), m_sq=-2.68, lambd=0.5)), 6, dict(exchange_every=1)
    counts = {}
    for improved in (False, True, False, True):              # the second pair is the one compared: everything is warm
        torch.manual_seed(2)
        s.start(n_chains=C)
        counts[improved] = _synchronising_calls(
            lambda: s.measure(C * 4, n_chains=C, n_md=4, dt=0.1, cluster_every=1, improved=improved, **kw))
    print(f"{which}: synchronising calls without / with improved: {counts[False]} / {counts[True]}")
    assert counts[False] >= 1 and counts[True] == counts[False]


def test_ladder_sampler_improved_changes_nothing_else():
    lat, K, R = (8, 8), 3, 2
    C = K * R
    m = H.model(lat, F32, DEV, **H.INTERACTING)
    lad = m.hmc.ladder(ScalarPhi4Ladder(kappa=(0.3, 0.5, 0.67), m_sq=-2.68, lambd=0.5))
    runs = {}
    for improved in (False, True, 'composed'):
        torch.manual_seed(9)
        lad.history.reset_history()
        lad.start(n_chains=C)
        got = lad.measure(C * 6, n_chains=C, n_md=5, dt=0.1, exchange_every=1, cluster_every=2, improved=improved)
        runs[improved] = (got, _state(lad) + (lad._ref['rung'].clone(),))
    for other in (runs[True], runs['composed']):
        _same_state(runs[False][1], other[1])
        assert torch.equal(runs[False][1][5], other[1][5])
        for a, b in zip(runs[False][0], other[0]):
            for key in ('sum_phi', 'sum_phi2', 'sum_phi4', 'links', 'action'):
                assert torch.equal(getattr(a, key), getattr(b, key)), key
    for k in range(K):
        a, b = runs[True][0][k].improved, runs['composed'][0][k].improved
        assert runs[False][0][k].improved is None
        assert len(a) == 3 * R and tuple(a.prop1.shape) == (3 * R, 2) and (a.status == 0).all()
        assert ((a.out - b.out).abs() <= _bound_of(b.out, 64)).all()
    # rung order: the first sweep of the call falls on the identity state, rung[c] = c % K; its rows by chain are those
    # of the bare sweep from the same position
    torch.manual_seed(9)
    lad.start(n_chains=C)
    phi0 = lad._ref['sample'].clone()
    seed, offset = torch.cuda.default_generators[0].initial_seed(), torch.cuda.default_generators[0].get_offset() // 4
    r = lad.cluster(phi0, position=(seed, offset))
    by_chain = ob.measure_improved(r['phi'], r['labels'])
    for c in range(C):
        assert torch.equal(runs[True][0][c % K].improved.out[c // K], by_chain.out[c]), c

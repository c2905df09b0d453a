"""nf_cluster_modes on the device against the numpy restatement (tests/modes_cases.py): every lane map, pass structure and
column-writing branch; the header's four consequences against nf_cluster_moments and nf_cluster_spectrum; a column's bits
under another list, C and row position; the refused inputs; graph replay; `measure(improved=True, modes=...)` of the fused
sampler and the ladder; and the exact free-field propagator off the axes."""
import math

import numpy as np
import pytest
import torch

from normflow__amd import _hip
from normflow__amd.action import ScalarPhi4Action, ScalarPhi4Ladder
from normflow__amd.lib import observables as ob
from normflow__amd.mcmc.cluster import cluster_modes

import hmc_cases as H
import improved_cases as Ic
import modes_cases as Mc
import spectrum_cases as Sc

pytestmark = pytest.mark.gpu
DEV = H.DEV
F32, F64 = torch.float32, torch.float64
DISTINCT = 12                   # chains of a case; a batch of C rows repeats them in a cycle
_CASES = {}


def all_modes(lat):
    """Every list of `mode_lists(lat)` one after the other: the restatement is made once for all of them."""
    return [m for lst in Mc.mode_lists(lat).values() for m in lst]


def case(lat, dt):
    """DISTINCT chains of the case, chain i with the label kind i % 6 (the two sweeps are nf_phi4_cluster's, of an ordered
    field at kappa = 0.67 and of a disordered one at kappa = 0.25), and their restatement at `all_modes(lat)`: computed
    once, never changed."""
    key = (lat, dt)
    if key not in _CASES:
        V = Ic.volume(lat)
        phi = Ic.field(lat, dt, DISTINCT)
        phi[0::6] = Ic.field(lat, dt, DISTINCT, ordered=True)[0::6]
        labels = np.zeros((DISTINCT, V), dtype=np.int32)
        for i, kind in enumerate(Ic.KINDS):
            n = len(range(i, DISTINCT, 6))
            if kind.startswith('sweep'):
                w0 = ScalarPhi4Action(kappa=0.67 if kind == 'sweep67' else 0.25, m_sq=-2.68, lambd=0.5).get_coef(len(lat))[0]
                p = torch.from_numpy(phi[i::6].copy()).to(DEV).reshape((n,) + tuple(lat))
                r = _hip.phi4_cluster(p, w0, position=(77, 10 + i), want_labels=True)
                assert (r['stats'][:, 3] >= 1).all()
                labels[i::6] = r['labels'].reshape(n, V).cpu().numpy()
            else:
                labels[i::6] = Ic.synthetic_labels(kind, n, V)
        modes = all_modes(lat)
        ref = Mc.restate(phi, labels, lat, _hip.mode_twiddle_table(lat).numpy(), modes)
        assert (ref['status'] == 0).all()
        for a in (phi, labels, ref['out'], ref['bound'], ref['status']):
            a.setflags(write=False)
        _CASES[key] = dict(phi=phi, labels=labels, ref=ref, modes=modes)
    return _CASES[key]


def select(c, lat, lst):
    """The restatement of the list `lst`, whose momenta are among the case's: its columns."""
    cols = [0, 1] + [2 + c['modes'].index(m) for m in lst]
    ref = c['ref']
    return dict(status=ref['status'], out=ref['out'][:, cols], bound=ref['bound'][:, cols], modes=Mc.reduce(lat, lst))


def _dev(c, lat, rows):
    rows = np.asarray(rows) % DISTINCT
    shape = (len(rows),) + tuple(lat)
    return (torch.from_numpy(c['phi'][rows].copy()).to(DEV).reshape(shape),
            torch.from_numpy(c['labels'][rows].copy()).to(DEV).reshape(shape))


def _host(r):
    return r['out'].cpu().numpy(), r['status'].cpu().numpy()


CASES = ([(lat, dt) for lat in Mc.GPU_LATTICES for dt in Mc.DTYPES] + [(lat, 'float32') for lat in Mc.F32_ONLY])


@pytest.mark.parametrize("C", Mc.CHAINS)
@pytest.mark.parametrize("lat,dt", CASES, ids=[Ic.case_id(c) for c in CASES])
def test_kernel_equals_the_restatement(lat, dt, C, parity_report):
    """Every list of `mode_lists` (the zero momentum first, a corner in the middle, negative components, on-axis and
    generic entries, an R that ends a pass) and all of them in one call; the composed path's status bit for bit and its
    doubles within the two bounds."""
    c = case(lat, dt)
    phi, labels = _dev(c, lat, np.arange(C))
    before = phi.clone()
    lists = dict(Mc.mode_lists(lat), everything=c['modes'])
    for name, lst in lists.items():
        r = _hip.cluster_modes(phi, labels, lst)
        assert r['modes'] == Mc.reduce(lat, lst) and r['out'].dtype == F64 and tuple(r['out'].shape) == (C, 2 + len(lst))
        assert r['status'].dtype == torch.int32
        want = Mc.tile(select(c, lat, lst), C)
        Mc.check_against(f"modes {Ic.case_id((lat, dt))} {name} C={C}", *_host(r), want,
                         parity_report if C == max(Mc.CHAINS) and name == 'everything' else None)
        if C == 3:
            o = cluster_modes(phi, labels, lst)
            assert torch.equal(o['status'], r['status']) and o['modes'] == r['modes']
            assert ((o['out'] - r['out']).abs().cpu().numpy() <= 2 * want['bound']).all(), name
    assert torch.equal(phi, before)


@pytest.mark.parametrize("lat,dt", CASES, ids=[Ic.case_id(c) for c in CASES])
def test_composed_integer_sums_are_the_kernels(lat, dt):
    """The per-cluster int64 sums are exact whatever the order: the composed path's scatter gives the restatement's slot
    arrays bit for bit (they are what the kernel adds up in LDS; nf_cluster_moments exposes its A the same way)."""
    c = case(lat, dt)
    phi, labels = _dev(c, lat, np.arange(4))
    V = Ic.volume(lat)
    x, lab = phi.double().reshape(4, V), labels.reshape(4, V).long()
    tw = _hip.mode_twiddle_table(lat, DEV)
    N = _hip.modes_lcm(lat)
    coords = [torch.from_numpy(a).to(DEV) for a in np.unravel_index(np.arange(V), lat)]
    ref = Mc.restate(c['phi'][:4], c['labels'][:4], lat, _hip.mode_twiddle_table(lat).numpy(), c['modes'][:3])
    for m, (R, I) in zip(ref['modes'], ref['slots']):
        j = sum((n * (N // L)) * xm for n, L, xm in zip(m, lat, coords)) % N
        for comp, want in ((0, R), (1, I)):
            if want is None:
                continue
            q = torch.round(x * tw[j][:, comp] * 2.0 ** 32).to(torch.int64)
            got = torch.zeros((4, V), dtype=torch.int64, device=DEV).scatter_add_(1, lab, q)
            assert np.array_equal(got.cpu().numpy(), want), (m, comp)
    mom = _hip.cluster_moments(phi, labels, want_moments=True)
    assert np.array_equal(mom['moments'].reshape(4, V).cpu().numpy(), ref['A'])


@pytest.mark.parametrize("lat,dt", CASES, ids=[Ic.case_id(c) for c in CASES])
def test_the_four_consequences(lat, dt):
    """1: columns 0 and 1 are nf_cluster_moments'; 2: the zero momentum's column is column 0; 3: an on-axis momentum's column
    is nf_cluster_spectrum's, bit for bit where N / L_mu is a power of two and within the bound at (3, 5) and (5, 7, 3);
    4: a flip of clusters changes no bit."""
    c = case(lat, dt)
    C, d = 40, len(lat)
    phi, labels = _dev(c, lat, np.arange(C))
    K = Sc.kmax_of(lat, 3)
    on_axis = [tuple(k if b == a else 0 for b in range(d)) for a in range(d) for k in range(1, K[a] + 1)]
    lst = [(0,) * d] + on_axis + c['modes'][:2]
    r = _hip.cluster_modes(phi, labels, lst)
    m, s = _hip.cluster_moments(phi, labels), _hip.cluster_spectrum(phi, labels, 3)
    assert torch.equal(r['out'][:, :2], m['out'][:, :2]) and torch.equal(r['status'], m['status'])
    assert torch.equal(r['out'][:, 2], r['out'][:, 0])
    got, want = r['out'][:, 3:3 + len(on_axis)], s['out'][:, 2:]
    if lat in Mc.POW2_RATIO:
        assert torch.equal(got, want)
    else:
        ref = Sc.restate(c['phi'], c['labels'], lat, _hip.twiddle_table(lat).numpy(), 3)
        bound = Sc.tile(ref, C)['bound'][:, 2:]
        assert ((got - want).abs().cpu().numpy() <= 2 * bound).all()
    flipped = torch.where(labels % 3 == 0, -phi, phi)
    assert not torch.equal(flipped, phi)
    f = _hip.cluster_modes(flipped, labels, lst)
    assert torch.equal(f['out'], r['out']) and torch.equal(f['status'], r['status'])


@pytest.mark.parametrize("lat,dt", CASES, ids=[Ic.case_id(c) for c in CASES])
def test_a_columns_bits_depend_on_its_momentum_alone(lat, dt):
    """A permuted list, a sub-list, another C and another row position; two calls agree."""
    c = case(lat, dt)
    C = 300
    phi, labels = _dev(c, lat, np.arange(C))
    modes = c['modes']
    a = _hip.cluster_modes(phi, labels, modes)
    b = _hip.cluster_modes(phi, labels, modes)
    assert torch.equal(a['out'], b['out']) and torch.equal(a['status'], b['status'])
    perm = np.random.default_rng(len(modes)).permutation(len(modes)).tolist()
    p = _hip.cluster_modes(phi, labels, [modes[i] for i in perm])
    assert torch.equal(p['out'][:, 2:], a['out'][:, [2 + i for i in perm]]) and torch.equal(p['out'][:, :2], a['out'][:, :2])
    for sub in (modes[1::2], modes[-1:], modes[2:5]):                  # other pass layouts, other R / I parities
        s = _hip.cluster_modes(phi, labels, sub)
        assert torch.equal(s['out'][:, 2:], a['out'][:, [2 + modes.index(m) for m in sub]]), sub
    for i in (0, 150, 299):
        one = _hip.cluster_modes(phi[i:i + 1].contiguous(), labels[i:i + 1].contiguous(), modes)
        assert torch.equal(a['out'][i:i + 1], one['out']) and torch.equal(a['status'][i:i + 1], one['status']), i
    im = ob.measure_improved(phi, labels, modes=modes)                # path=None: the kernel
    assert torch.equal(im.mode_power, a['out'][:, 2:]) and im.modes == a['modes']
    assert torch.equal(im.out, _hip.cluster_moments(phi, labels)['out'])


GRAPH = [((16, 16), 'float32'), ((16, 16, 16), 'float64'), ((5, 7, 3), 'float32')]


@pytest.mark.parametrize("lat,dt", GRAPH, ids=[Ic.case_id(c) for c in GRAPH])
def test_graph_replay_equals_eager(lat, dt):
    """One linear stream; the tables are on the device before the capture (the eager call put them there)."""
    c = case(lat, dt)
    phi, labels = _dev(c, lat, np.arange(7))
    eager = _hip.cluster_modes(phi, labels, c['modes'])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        r = _hip.cluster_modes(phi, labels, c['modes'])
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(eager['out'], r['out']) and torch.equal(eager['status'], r['status'])


REFUSALS = [("nan", 'float32', float('nan'), None), ("inf", 'float64', float('inf'), None), ("2^16", 'float32', 2.0 ** 16, None),
            ("label -1", 'float32', None, -1), ("label V", 'float64', None, 256)]


@pytest.mark.parametrize("name,dt,value,label", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refused_inputs_on_the_device(name, dt, value, label):
    """The guard is part of the ABI: the chain is refused before any slot is indexed.  The same inputs go through the
    composed path first, which never indexes with them either."""
    lat = (16, 16)
    c = case(lat, dt)
    modes = c['modes']
    phi, labels = c['phi'][:3].copy(), c['labels'][:3].copy()
    if value is not None:
        phi[1, 77] = value
    else:
        labels[1, 77] = label
    ref = Mc.restate(phi, labels, lat, _hip.mode_twiddle_table(lat).numpy(), modes)
    assert ref['status'].tolist() == [0, 1, 0]
    shape = (3,) + lat
    dphi, dlab = torch.from_numpy(phi).to(DEV).reshape(shape), torch.from_numpy(labels).to(DEV).reshape(shape)
    o = cluster_modes(dphi, dlab, modes)
    Mc.check_against(f"composed, {name}", *_host(o), ref)
    k = _hip.cluster_modes(dphi, dlab, modes)
    Mc.check_against(f"kernel, {name}", *_host(k), ref)
    assert torch.isnan(k['out'][1]).all()
    good = _hip.cluster_modes(*_dev(c, lat, np.arange(3)), modes)
    for i in (0, 2):                                         # the neighbouring chains are what they were
        assert torch.equal(k['out'][i], good['out'][i])


def test_wrapper_refuses_what_it_cannot_take():
    phi = torch.zeros((2, 4, 4), dtype=F32, device=DEV)
    lab = torch.zeros((2, 4, 4), dtype=torch.int32, device=DEV)
    with pytest.raises(_hip.NormflowHipError, match="labels"):
        _hip.cluster_modes(phi, lab.long(), [(1, 1)])
    with pytest.raises(_hip.NormflowHipError, match="modes"):
        _hip.cluster_modes(phi, lab, [(1, 1, 1)])
    with pytest.raises(_hip.NormflowHipError, match="extent 1"):
        _hip.cluster_modes(phi.reshape(2, 1, 16), lab.reshape(2, 1, 16), [(1, 1)])
    big = torch.zeros((1, 32, 32, 32), dtype=F32, device=DEV)
    blab = torch.zeros(big.shape, dtype=torch.int32, device=DEV)
    with pytest.raises(_hip.NormflowHipError, match="class"):
        _hip.cluster_modes(big, blab, [(1, 1, 0)])
    with pytest.raises(_hip.NormflowHipError):
        ob.measure_improved(big, blab, path='kernel', modes=[(1, 1, 0)])
    im = ob.measure_modes(big, [(1, 1, 0), (0, 0, 0)])                  # beyond one CU: the composed path
    assert im.modes == ((1, 1, 0), (0, 0, 0)) and (im.status == 0).all() and tuple(im.mode_power.shape) == (1, 2)


# ---------------------------------------------------------------- the samplers on the device
def _state(s):
    return (s._ref['sample'].clone(), s._ref['action'].clone(), {k: v.clone() for k, v in s.last.items()},
            [list(getattr(s.history, k)) for k in type(s.history)._KEYS], torch.cuda.default_generators[0].get_offset())


def _same_state(a, b):
    # the histories by their text: with exchange_every=0 the ladder's exchange rates are NaN, and NaN != NaN
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and repr(a[3]) == repr(b[3]) and a[4] == b[4]
    assert set(a[2]) == set(b[2])
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k


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


MODES = [(1, 1), (0, 0), (2, -1), (8, 8), (3, 0)]


@pytest.mark.parametrize("which", ["fused", "ladder"])
def test_sampler_modes_change_nothing_else_and_are_measure_improved_of_the_same_sweeps(which):
    lat, K = (16, 16), 3
    m = H.model(lat, F32, DEV, **H.INTERACTING)
    if which == "fused":
        s, C, kw = m.hmc, 5, {}
    else:
        s, C, kw = m.hmc.ladder(ScalarPhi4Ladder(kappa=(0.3, 0.5, 0.67), m_sq=-2.68, lambd=0.5)), 6, dict(exchange_every=0)
    runs, counts = {}, {}
    for modes in (None, MODES, None, MODES):                 # the second pair is the one compared: everything is warm
        torch.manual_seed(9)
        s.history.reset_history()
        s.start(n_chains=C)
        start = s._ref['sample'].clone()
        offset = torch.cuda.default_generators[0].get_offset()
        box = []
        counts[modes is None] = _synchronising_calls(lambda: box.append(
            s.measure(C * 3, n_chains=C, n_md=5, dt=0.1, cluster_every=1, improved=True, modes=modes, return_rows=True, **kw)))
        runs[modes is None] = (box[0], _state(s))
    (bare, ybare), (full, yfull) = runs[True][0], runs[False][0]
    _same_state(runs[True][1], runs[False][1])
    print(f"{which}: synchronising calls without / with modes: {counts[True]} / {counts[False]}")
    assert counts[True] >= 1 and counts[False] == counts[True]
    assert torch.equal(ybare, yfull)
    for a, b in zip(bare if which == "ladder" else [bare], full if which == "ladder" else [full]):
        for key in ('sum_phi', 'sum_phi2', 'sum_phi4', 'links', 'action'):
            assert torch.equal(getattr(a, key), getattr(b, key)), key
        assert torch.equal(a.improved.out, b.improved.out) and torch.equal(a.improved.status, b.improved.status)
        assert a.improved.modes is None and b.improved.modes == ((1, 1), (0, 0), (2, 15), (8, 8), (3, 0))
        assert (b.improved.status == 0).all() and torch.equal(b.improved.mode_power[:, 1], b.improved.sum_m2)
    chains = s._ref['sample']
    assert ob.improved_kernel_applies(chains)
    # the first sweep of the call is the sweep of the starting chains at the generator's state of the start
    torch.manual_seed(9)
    torch.cuda.default_generators[0].set_offset(offset)
    if which == "fused":
        r = s.cluster(start)
        first = ob.measure_improved(r['phi'], r['labels'], modes=MODES)
        assert torch.equal(first.out, full.improved.out[:C]) and torch.equal(first.mode_power, full.improved.mode_power[:C])
        # the first recorded rows are one trajectory after that sweep, so the sweeps' fields are not the rows'; the labels
        # of `cluster` are the call's, and the kernel's row is the composed path's within the two bounds
        o = ob.measure_improved(r['phi'], r['labels'], path='composed', modes=MODES)
        assert ((o.mode_power - first.mode_power).abs() <= 2 * (256 + 8) * 2.0 ** -53 * o.mode_power.abs()).all()
    else:
        rung = (torch.arange(C, device=DEV) % K).to(torch.int32)
        r = s.cluster(start, rung)
        by_chain = ob.measure_improved(r['phi'], r['labels'], modes=MODES)
        for c in range(C):
            k, row = int(rung[c]), c // K
            assert torch.equal(full[k].improved.out[row], by_chain.out[c]), (c, k)
            assert torch.equal(full[k].improved.mode_power[row], by_chain.mode_power[c]), (c, k)


def test_free_field_propagator_off_the_axes():
    """lambda = 0 on (8, 8), the parameters and run length of test_cluster_improved.py::test_free_field_exactness:
    <|phi~(p)|^2> / V = 1 / (m^2 + 2 kappa sum_mu (1 - cos(2 pi n_mu / L_mu))) at n = (1, 1), (1, 2) and (2, -1), exactly;
    its criteria: within 5 jackknife errors, and an error below 5 % of the value."""
    lat, C, drop, steps = (8, 8), 256, 60, 160
    modes = [(1, 1), (1, 2), (2, -1)]
    m = H.model(lat, F64, DEV, **H.FREE)
    torch.manual_seed(5)
    m.hmc.start(n_chains=C)
    got = m.hmc.measure(C * (drop + steps), n_chains=C, n_md=10, dt=0.1, cluster_every=1, improved=True, modes=modes)
    assert (got.improved.status == 0).all()
    g, err = ob.ImprovedEnsemble(got.improved, n_chains=C, drop=drop).mode_propagator()
    for i, n in enumerate(modes):
        want = 1 / (H.FREE['m_sq'] + 2 * H.FREE['kappa'] * sum(1 - math.cos(2 * math.pi * k / L) for k, L in zip(n, lat)))
        print(f"free 8^2 improved G(p) at n = {n}: {g[i]:.5f} +- {err[i]:.5f}, exact {want:.5f}")
        assert abs(g[i] - want) <= 5 * err[i] and err[i] < 0.05 * want, n

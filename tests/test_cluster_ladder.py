"""nf_phi4_cluster_ladder and nf_phi4_cluster_tiled_ladder (the Swendsen-Wang sweep with the hopping coefficient of every
chain's rung) and LadderHMCSampler(cluster_every) on the device.

A chain on rung k gets nf_phi4_cluster's bits at w0_k: the ladder kernels are held BIT FOR BIT -- fields, labels and the
stats, read at the rung-ordered row -- to the plain kernels run once per rung on all chains, and to the numpy union-find
of tests/cluster_cases.py, on fields that tests/test_cluster_ladder_host.py finds clear of ties at every rung."""
import functools

import numpy as np
import pytest
import torch

from normflow__amd import _hip
from normflow__amd.lib import observables as ob

import hmc_cases as H
import ladder_cases as Lc
import cluster_cases as Cc
import cluster_ladder_cases as Clc
from hmc_cases import DEV

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64


def _np(phi, r):
    """(fields after, labels (C, V), stats) as numpy."""
    torch.cuda.synchronize()
    C = phi.shape[0]
    return phi.cpu().numpy(), r['labels'].cpu().numpy().reshape(C, -1), r['stats'].cpu().numpy()


def _dev(phi_np):
    return torch.from_numpy(np.ascontiguousarray(phi_np)).to(DEV)


def _ladder(phi_np, coef, rung, tile=None):
    """One ladder sweep at Cc.POS by the fused kernel (tile None) or the tiled one."""
    phi = _dev(phi_np)
    if tile is None:
        return _np(phi, _hip.phi4_cluster_ladder(phi, coef, rung, position=Cc.POS, want_labels=True))
    return _np(phi, _hip.phi4_cluster_tiled_ladder(phi, coef, rung, position=Cc.POS, want_labels=True, tile_sites=tile))


def _plain(phi_np, w0, tile=None):
    phi = _dev(phi_np)
    if tile is None:
        return _np(phi, _hip.phi4_cluster(phi, w0, position=Cc.POS, want_labels=True))
    return _np(phi, _hip.phi4_cluster_tiled(phi, w0, position=Cc.POS, want_labels=True, tile_sites=tile))


@functools.lru_cache(maxsize=None)
def _restated(case, k):
    """The numpy sweep of all chains of the case at the w0 of rung k, computed once and shared: leave it unchanged."""
    lat, dt, chains, K = case
    return Cc.sweep(Clc.field(case), lat, Clc.W0S[K][k], *Cc.POS)


def _state(case):
    lat, dt, chains, K = case
    return Clc.field(case), Clc.coef_table(K, DEV), Clc.rung(chains, K, DEV)


def _held_to(got, rung, K, k, want, what, columns=3):
    """The chains of `got` (a ladder sweep) on rung k against the same chains of `want` (all chains swept at w0_k): fields
    and labels at the chain's index, stats at the rung-ordered row of `got` and at the chain's row of `want`."""
    r = rung.cpu().numpy()
    on = np.nonzero(r == k)[0]
    rows = Clc.rows_of(r, K)[on]
    assert on.size == r.size // K, (what, "chains on the rung")
    assert np.array_equal(got[1][on], want[1][on]), (what, "labels")
    assert np.array_equal(Cc.bits(got[0])[on], Cc.bits(want[0])[on]), (what, "fields")
    assert np.array_equal(got[2][rows, :columns], want[2][on, :columns]), (what, "stats", got[2][rows], want[2][on])
    assert (got[2][rows, 3] >= 1).all(), (what, "rounds", got[2][rows, 3])


@pytest.mark.parametrize("case", Clc.FUSED, ids=Clc.case_id)
def test_fused_ladder_is_the_plain_kernel_rung_by_rung(case):
    lat, dt, chains, K = case
    phi, coef, rung = _state(case)
    got = _ladder(phi, coef, rung)
    flipped = 0
    for k, w0 in enumerate(Clc.W0S[K]):
        _held_to(got, rung, K, k, _plain(phi, w0), f"{Clc.case_id(case)} rung {k} against nf_phi4_cluster")
        _held_to(got, rung, K, k, _restated(case, k), f"{Clc.case_id(case)} rung {k} against the restatement")
        flipped += int(_restated(case, k)[2][:, 1].sum())
    assert flipped > 0


@pytest.mark.parametrize("tile", Clc.TILES, ids=lambda t: f"tile{t}")
@pytest.mark.parametrize("case", Clc.TILED, ids=Clc.case_id)
def test_tiled_ladder_is_the_plain_tiled_kernel_rung_by_rung(case, tile):
    lat, dt, chains, K = case
    phi, coef, rung = _state(case)
    V = int(np.prod(lat))
    got = _ladder(phi, coef, rung, tile)
    assert (got[2][:, 3] == -(-V // (tile or V))).all()                   # the tiles of a chain; the default tile holds V
    fused = _ladder(phi, coef, rung)
    assert np.array_equal(got[1], fused[1]) and np.array_equal(Cc.bits(got[0]), Cc.bits(fused[0]))
    assert np.array_equal(got[2][:, :3], fused[2][:, :3])
    for k, w0 in enumerate(Clc.W0S[K]):
        what = f"{Clc.case_id(case)} tile {tile} rung {k}"
        _held_to(got, rung, K, k, _plain(phi, w0, tile), what + " against nf_phi4_cluster_tiled", columns=4)
        _held_to(got, rung, K, k, _restated(case, k), what + " against the restatement")


def test_tiled_ladder_beyond_the_fused_class():
    """(32, 32, 32) fp32, one replica set of three rungs at the default tile (2 tiles, LDS beyond 64 KiB)."""
    lat, dt, chains, K = Clc.BIG
    assert not _hip.cluster_supported(lat, F32) and _hip.cluster_tiled_plan(lat, F32)['tiles'] == 2
    phi, coef, rung = _state(Clc.BIG)
    got = _ladder(phi, coef, rung, 0)
    seen = set()
    for k, w0 in enumerate(Clc.W0S[K]):
        want = _plain(phi, w0, 0)
        _held_to(got, rung, K, k, want, f"32^3 rung {k}", columns=4)
        seen.add(tuple(want[2][:, 0].tolist()))
    assert len(seen) == K and (got[2][:, 3] == 2).all()
    with pytest.raises(_hip.NormflowHipError, match="outside the class"):
        _hip.phi4_cluster_ladder(_dev(phi), coef, rung)


@pytest.mark.parametrize("tile", [None, 16], ids=["fused", "tiled"])
def test_a_rung_outside_the_table_is_clamped(tile):
    case = ((8, 8), 'float64', Clc.CHAINS, 3)
    phi, coef, _ = _state(case)
    outside = torch.tensor([-1, 1, 3, 3, -1, 1], dtype=torch.int32, device=DEV)
    inside = torch.tensor([0, 1, 2, 2, 0, 1], dtype=torch.int32, device=DEV)
    got, want = _ladder(phi, coef, outside, tile), _ladder(phi, coef, inside, tile)
    assert np.array_equal(Cc.bits(got[0]), Cc.bits(want[0])) and np.array_equal(got[1], want[1])
    columns = 3 if tile is None else 4                                     # the fused kernel's rounds are not pinned
    assert np.array_equal(got[2][:, :columns], want[2][:, :columns]) and (got[2][:, 3] >= 1).all()
    assert outside.tolist() == [-1, 1, 3, 3, -1, 1]                        # the kernel does not write the rungs


def test_positions_come_from_the_generator_and_labels_are_optional():
    case = ((16, 16), 'float32', Clc.CHAINS, 3)
    phi, coef, rung = _state(case)
    torch.manual_seed(19)
    gen = torch.cuda.default_generators[0]
    seed, off = gen.initial_seed(), gen.get_offset()
    t = _dev(phi)
    r = _hip.phi4_cluster_ladder(t, coef, rung)
    assert gen.get_offset() == off + 8 and r['labels'] is None
    want = _dev(phi)
    _hip.phi4_cluster_ladder(want, coef, rung, position=(seed, off // 4))
    assert torch.equal(t, want)
    ws = torch.empty(_hip.cluster_tiled_workspace(Clc.CHAINS, (16, 16), 64), dtype=torch.uint8, device=DEV)
    t2 = _dev(phi)
    _hip.phi4_cluster_tiled_ladder(t2, coef, rung, tile_sites=64, workspace=ws)
    assert gen.get_offset() == off + 16
    with pytest.raises(_hip.NormflowHipError, match="workspace"):
        _hip.phi4_cluster_tiled_ladder(t2, coef, rung, tile_sites=64, workspace=ws[:-16])
    for bad in (dict(coef=coef.float()), dict(rung=rung.long()), dict(rung=rung[:3]), dict(coef=coef[:, :2].contiguous()),
                dict(coef=coef.cpu()), dict(coef=torch.cat([coef, coef[:1]]))):
        with pytest.raises(_hip.NormflowHipError):
            _hip.phi4_cluster_ladder(t, **dict(dict(coef=coef, rung=rung), **bad))


def test_graph_capture():
    """The sweep neither allocates nor synchronises: one capture, replayed twice on copies of the same chains, equals the
    eager call both times."""
    case = ((16, 16), 'float32', Clc.CHAINS, 3)
    phi, coef, rung = _state(case)
    eager = _ladder(phi, coef, rung)
    start = _dev(phi)
    static = start.clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        r = _hip.phi4_cluster_ladder(static, coef, rung, position=Cc.POS, want_labels=True)
    torch.cuda.synchronize()
    assert torch.equal(static, start)                                      # capture ran nothing
    for replay in range(2):
        static.copy_(start)
        r['stats'].zero_()
        r['labels'].zero_()
        g.replay()
        got = _np(static, r)
        assert np.array_equal(Cc.bits(got[0]), Cc.bits(eager[0])), replay
        assert np.array_equal(got[1], eager[1]) and np.array_equal(got[2][:, :3], eager[2][:, :3]), replay
        assert (got[2][:, 3] >= 1).all(), replay


# ---------------------------------------------------------------- the sampler
def _sampler(lattice, dtype, couplings):
    m, ladder = Lc.model(lattice, dtype, DEV, **couplings)
    return m, ladder, m.hmc.ladder(ladder)


PATHS = [((6, 6), 'fused'), ((8, 8), 'tiled')]


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("lat,path", PATHS, ids=[p[1] for p in PATHS])
def test_equal_rungs_are_the_plain_sampler(lat, path, K):
    """K = 1, and three equal rungs without exchanges: the plain sampler's chain from the same seed, bit for bit."""
    C, n = 6, 5
    m, ladder, s = _sampler(lat, F32, dict(kappa=[H.INTERACTING['kappa']] * K, m_sq=H.INTERACTING['m_sq'],
                                           lambd=H.INTERACTING['lambd']))
    phi0 = H.field((C,) + lat, F32, 43, scale=1.2)
    kw = dict(n_chains=C, n_md=3, dt=0.1, path=path, cluster_every=2)
    torch.manual_seed(31)
    plain = m.hmc.start(phi0).sample(n * C, **kw)
    torch.manual_seed(31)
    s.start(phi0)
    got = s.sample(n * C, exchange_every=1 if K == 1 else 0, **kw)
    assert torch.equal(got, plain) and torch.equal(s.last['dh'], m.hmc.last['dh'])
    assert torch.equal(s.last['cluster'][..., :3], m.hmc.last['cluster'][..., :3]) and s.last['cluster'].shape == (3, C, 4)
    assert (s.last['cluster'][..., 3] >= 1).all() and s.last['cluster'][..., 1].sum().item() > 0
    assert torch.equal(s._ref['action'], m.hmc._ref['action'])


@pytest.mark.parametrize("lat,path", PATHS, ids=[p[1] for p in PATHS])
def test_measure_is_measure_of_the_split_rows_with_both_sweeps(lat, path):
    K, R, n = 3, 2, 5
    C = K * R
    m, ladder, s = _sampler(lat, F32, Lc.DISTINCT(K))
    phi0 = H.field((C,) + lat, F32, 44, scale=1.2)
    kw = dict(n_chains=C, n_md=3, dt=0.1, path=path, exchange_every=1, cluster_every=2)
    torch.manual_seed(33)
    s.start(phi0)
    y = s.sample(n * C, **kw)
    cl, rung, sw = s.last['cluster'], s._ref['rung'].clone(), s.last['swapped']
    assert cl.shape == ((n + 1) // 2, C, 4) and cl.dtype == torch.int32 and cl.is_cuda and (cl[..., 3] >= 1).all()
    assert sw.shape == (n, R, K - 1)
    assert torch.equal(rung.reshape(R, K).sort(dim=1).values.long(), torch.arange(K, device=DEV).expand(R, K))
    col = torch.arange(C, device=DEV) // K * K + rung.long()
    assert torch.equal(y[-C:][col], s._ref['sample'])
    torch.manual_seed(33)
    s.start(phi0)
    ms = s.measure(n * C, **kw)
    assert torch.equal(cl[..., :3], s.last['cluster'][..., :3]) and torch.equal(rung, s._ref['rung']) and torch.equal(sw, s.last['swapped'])
    parts = s.split(y)
    for k in range(K):
        want = ob.measure(parts[k], action=ladder.rung(k))
        for key in ('sum_phi', 'sum_phi2', 'sum_phi4', 'links', 'action'):
            assert torch.equal(getattr(ms[k], key), getattr(want, key)), (k, key)
        assert all(torch.equal(a, b) for a, b in zip(ms[k].slices, want.slices))


def test_sampler_sweeps_at_its_positions_with_the_rungs_of_the_moment():
    """(6, 6), 2 replica sets of 3 rungs, 4 steps with exchange_every = 1 and cluster_every = 2, replayed call by call:
    2 positions per sweep, 2 per trajectory, 1 per exchange; the sweep before step 2 takes the rungs the exchanges left."""
    lat, K, R, n_md, dt = (6, 6), 3, 2, 3, 0.1
    C = K * R
    m, ladder, s = _sampler(lat, F32, Lc.DISTINCT(K))
    phi0 = H.field((C,) + lat, F32, 45, scale=1.2)
    torch.manual_seed(35)
    gen = torch.cuda.default_generators[0]
    seed, off = gen.initial_seed(), gen.get_offset() // 4
    s.start(phi0)
    y = s.sample(4 * C, n_chains=C, n_md=n_md, dt=dt, exchange_every=1, cluster_every=2)
    coef = ladder.coef_table(lat, DEV)
    phi, rung = phi0.clone(), (torch.arange(C, device=DEV) % K).to(torch.int32)
    rows, sweeps = [], []
    for step in range(4):
        if step % 2 == 0:
            sweeps.append(_hip.phi4_cluster_ladder(phi, coef, rung, position=(seed, off))['stats'])
            off += 2
        r = _hip.phi4_hmc_ladder(phi, coef, rung, n_md, dt, n_traj=1, position=(seed, off))
        off += 2
        col = torch.arange(C, device=DEV) // K * K + rung.long()
        rows.append(torch.empty_like(phi).index_copy_(0, col, phi))
        _hip.ladder_exchange(_hip.lattice_measure(phi), coef, rung, step % 2, action=r['action'], position=(seed, off))
        off += 1
    assert torch.equal(y, torch.cat(rows)) and torch.equal(s.last['cluster'][..., :3], torch.stack(sweeps)[..., :3])
    assert torch.equal(s._ref['rung'], rung) and gen.get_offset() == 4 * off
    assert s.last['swapped'].sum().item() > 0


def test_bare_sweep_paths_agree():
    lat, K, C = (8, 8), 3, 6
    m, ladder, s = _sampler(lat, F64, Lc.DISTINCT(K))
    phi = _dev(Cc.field(lat, 'float64', C))
    before, rung = phi.clone(), Clc.rung(C, K, DEV)
    a, b, c = (s.cluster(phi, rung=rung, position=Cc.POS, path=p) for p in ('kernel', 'tiled', 'composed'))
    assert torch.equal(phi, before)
    for other in (b, c):
        assert np.array_equal(Cc.bits(a['phi']), Cc.bits(other['phi'])) and torch.equal(a['labels'], other['labels'])
        assert torch.equal(a['stats'][:, :3], other['stats'][:, :3]) and (other['stats'][:, 3] >= 1).all()
    d = s.cluster(phi, rung=rung, position=Cc.POS)
    assert torch.equal(d['stats'][:, :3], a['stats'][:, :3]) and torch.equal(d['labels'], a['labels'])
    ident = s.cluster(phi, position=Cc.POS)
    assert not torch.equal(ident['labels'], a['labels'])


# ---------------------------------------------------------------- exactness with both sweeps
def test_interacting_ladder_with_sweeps_and_exchanges_against_quadrature():
    """(4,), three rungs, 256 replica sets, a cluster sweep before and an exchange after every step: per rung <phi^2>
    within 5 standard errors (across the replica sets) of the quadrature, and <m> within 5 of 0."""
    K, R, steps, drop = 3, 256, 260, 30
    m, ladder, s = _sampler((4,), F32, Lc.INTERACTING_LADDER)
    torch.manual_seed(37)
    y = s.sample(K * R * steps, n_chains=K * R, n_md=4, dt=0.25, exchange_every=1, cluster_every=1)
    assert s.last['cluster'].shape == (steps, K * R, 4) and (s.last['cluster'][..., 3] >= 1).all()
    for k, yk in enumerate(s.split(y)):
        exact = Lc.quadrature_phi2(ladder.rung(k))
        mean, err = Lc.rung_stats(yk, R, drop=drop)
        per_set = yk.double().cpu().reshape(steps, R, -1)[drop:].mean(dim=(0, 2))
        mag, mag_err = per_set.mean().item(), per_set.std().item() / R ** 0.5
        print(f"(4,) ladder rung {k} with sweeps and exchanges: <phi^2> {mean:.5f} +- {err:.5f} "
              f"({(mean - exact) / err:+.2f} sigma of {exact:.6f}), <m> {mag:+.5f} +- {mag_err:.5f} ({mag / mag_err:+.2f} sigma)")
        assert abs(mean - exact) <= 5 * err
        assert abs(mag) <= 5 * mag_err
    print(f"exchange rates {s.history.exchange_rate[-1]}, accept rate {s.history.accept_rate[-1]:.3f}")
    assert all(0.0 < r < 1.0 for r in s.history.exchange_rate[-1])

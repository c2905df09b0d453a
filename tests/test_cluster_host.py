"""Cluster sweeps without a GPU: the exported symbols and the key domain, every NF_EINVAL of the four entry points, the
planner's table, the exact stationarity of the restated rule, `cluster_sweep` on CPU tensors against the restatement,
the tie guard on every case of the list, and `hmc.sample(cluster_every=E)` on CPU tensors."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from normflow__amd import _hip
from normflow__amd.mcmc.cluster import cluster_sweep

import hmc_cases as H
import cluster_cases as Cc

F32, F64 = torch.float32, torch.float64
CPU = torch.device("cpu")
NEW = ("nf_phi4_cluster_supported", "nf_phi4_cluster_plan", "nf_phi4_cluster", "nf_phi4_cluster_draws")
PTR = C.c_void_p(0x1000)


def test_symbols_are_declared_exported_and_prototyped():
    header = open(os.path.join(_hip._HERE, "..", "include", "normflow_hip.h")).read()
    declared = set(re.findall(r"\b(nf_[a-z0-9_]+)\s*\(", header))
    lib = _hip.load()
    for name in NEW:
        assert name in declared and hasattr(lib, name) and name in _hip.PROTOTYPES, name
    assert f"#define NF_PHILOX_CLUSTER_DOMAIN 0x{Cc.CLUSTER_DOMAIN:08x}u" in header
    domains = {k: int(v, 16) for k, v in re.findall(r"#define NF_PHILOX_(\w+)_DOMAIN (0x[0-9a-fA-F]+)u", header)}
    assert len(set(domains.values())) == len(domains) and domains["CLUSTER"] == Cc.CLUSTER_DOMAIN     # a key domain of its own


def _cluster(**over):
    """nf_phi4_cluster with valid arguments on a (4, 4) fp32 lattice except for `over`; the pointers are never followed,
    because every call here is refused before anything is launched."""
    a = dict(phi=PTR, stats=PTR, labels_out=None, C=6, lattice=_hip._lat4((4, 4)), w0=0.5, seed=1, offset=0,
             dtype=_hip.NF_F32, stream=None)
    assert set(over) <= set(a), over
    a.update(over)
    lib = _hip.load()
    return lib.nf_phi4_cluster(*a.values()), lib.nf_last_error_string().decode()


def _draws(**over):
    a = dict(u_out=PTR, flip_out=PTR, C=6, lattice=_hip._lat4((4, 4)), seed=1, offset=0, stream=None)
    assert set(over) <= set(a), over
    a.update(over)
    lib = _hip.load()
    return lib.nf_phi4_cluster_draws(*a.values()), lib.nf_last_error_string().decode()


CLUSTER_EINVAL = [
    ("phi", dict(phi=None), "NULL"), ("stats", dict(stats=None), "NULL"), ("lattice", dict(lattice=None), "NULL"),
    ("C=0", dict(C=0), "C (0)"), ("C=65536", dict(C=65536), "C (65536)"), ("fp16", dict(dtype=_hip.NF_F16), "dtype"),
    ("extent 0", dict(lattice=_hip._lat4((4, 0))), "extents"),
    ("32^3 fp32", dict(lattice=_hip._lat4((32, 32, 32))), "class"),
    ("24^3 fp64", dict(lattice=_hip._lat4((24, 24, 24)), dtype=_hip.NF_F64), "class"),
]
DRAWS_EINVAL = [
    ("u_out", dict(u_out=None), "NULL"), ("flip_out", dict(flip_out=None), "NULL"), ("lattice", dict(lattice=None), "NULL"),
    ("C=0", dict(C=0), "C (0)"), ("C=65536", dict(C=65536), "C (65536)"), ("extent 0", dict(lattice=_hip._lat4((0, 4))), "extents"),
    ("2^31 sites", dict(lattice=_hip._lat4((2 ** 16, 2 ** 15))), "2^31"),
]


@pytest.mark.parametrize("name,over,word", CLUSTER_EINVAL, ids=[e[0] for e in CLUSTER_EINVAL])
def test_cluster_argument_validation(name, over, word):
    rc, msg = _cluster(**over)
    assert rc == -1 and "nf_phi4_cluster" in msg and word in msg, (name, rc, msg)


@pytest.mark.parametrize("name,over,word", DRAWS_EINVAL, ids=[e[0] for e in DRAWS_EINVAL])
def test_cluster_draws_argument_validation(name, over, word):
    rc, msg = _draws(**over)
    assert rc == -1 and "nf_phi4_cluster_draws" in msg and word in msg, (name, rc, msg)


def test_plan_argument_validation():
    lib = _hip.load()
    plan = _hip.ClusterPlan()
    assert lib.nf_phi4_cluster_plan(_hip._lat4((4, 4)), _hip.NF_F32, None) == -1
    assert lib.nf_phi4_cluster_plan(None, _hip.NF_F32, C.byref(plan)) == -1
    assert lib.nf_phi4_cluster_plan(_hip._lat4((4, 4)), _hip.NF_F16, C.byref(plan)) == -1
    assert lib.nf_phi4_cluster_supported(None, _hip.NF_F32) == 0
    with pytest.raises(_hip.NormflowHipError, match="class"):
        _hip.cluster_plan((32, 32, 32), F32)


# (sites per lane, lanes, LDS bytes): nf_phi4_hmc's lane map; 256 B of flags and sums, 4 V of labels and V of bond bytes,
# the two arrays rounded up to 16 B
PLAN = {
    ((4,), F32): (1, 64, 288), ((8,), F64): (1, 64, 304), ((3, 5), F32): (1, 64, 336), ((2, 2, 2, 2), F64): (1, 64, 336),
    ((1, 8), F32): (1, 64, 304), ((16, 16), F32): (1, 256, 1536), ((16, 16), F64): (1, 256, 1536),
    ((64, 64), F32): (4, 1024, 20736), ((16, 16, 16), F64): (4, 1024, 20736), ((8, 8, 8, 8), F32): (4, 1024, 20736),
    ((24, 24, 24), F32): (16, 896, 69376),
    ((128, 128), F32): (16, 1024, 82176), ((64, 128), F64): (8, 1024, 41216),        # the largest of either dtype
}
REFUSED = [((129, 128), F32), ((65, 128), F64), ((24, 24, 24), F64), ((32, 32, 32), F32), ((16, 16, 16, 16), F32)]


def test_planner_table():
    for (lat, dt), want in PLAN.items():
        p = _hip.cluster_plan(lat, dt)
        assert (p['sites_per_lane'], p['lanes'], p['lds_bytes']) == want, (lat, dt, p)
        assert _hip.cluster_supported(lat, dt) and _hip.hmc_supported(lat, dt)
        h = _hip.hmc_plan(lat, dt)
        assert (p['sites_per_lane'], p['lanes']) == (h['sites_per_lane'], h['lanes'])
        assert p['lds_bytes'] <= 160 * 1024
    for lat, dt in REFUSED:
        assert not _hip.cluster_supported(lat, dt) and not _hip.hmc_supported(lat, dt), (lat, dt)
    for lat, dt, _ in Cc.CASES:
        assert _hip.cluster_supported(lat, getattr(torch, dt)), (lat, dt)
    assert not _hip.cluster_supported((4, 4), torch.float16)


# ---------------------------------------------------------------- the rule itself
RING4 = [(0, 1), (1, 2), (2, 3), (3, 0)]


@pytest.mark.parametrize("name,absphi,w0,links", [
    ("ring of 4, w0 > 0", [0.3, 1.2, 0.8, 2.0], 0.67, RING4), ("ring of 4, w0 < 0", [0.3, 1.2, 0.8, 2.0], -0.5, RING4),
    ("extent 2, double link", [0.7, 1.1], 0.67, [(0, 1), (1, 0)])], ids=["ring4", "ring4-negative", "double-link"])
def test_restated_rule_is_exactly_stationary(name, absphi, w0, links):
    """All sign states x all bond sets x all flip choices: the sweep maps the Boltzmann weights onto themselves."""
    dev = Cc.stationarity(absphi, w0, links)
    print(f"{name}: max deviation {dev:.3e}")
    assert dev <= 1e-14, (name, dev)


def test_restatement_on_hand_made_bonds():
    """The union-find against clusters read off by eye: (2, 3) lattice, u set by hand."""
    phi = np.array([[[1.0, 1.0, -1.0], [1.0, -1.0, -1.0]]])
    u = np.ones((1, 6, 4))                        # no bond
    for x, mu in [(0, 3), (0, 2), (4, 3), (2, 2)]:      # 0-1, 0-3 (down), 4-5, 2-5 (down)
        u[0, x, mu] = 1e-6
    u[0, 1, 3] = 1e-6                              # 1-2 have opposite signs: t < 0, no bond whatever u
    flip = np.array([[True, False, False, True, True, True]])
    new, labels, stats = Cc.sweep_with(phi, (2, 3), 2.0, u, flip)
    assert labels.tolist() == [[0, 0, 2, 0, 2, 2]]
    assert new.reshape(-1).tolist() == [-1.0, -1.0, -1.0, -1.0, -1.0, -1.0]
    assert stats.tolist() == [[2, 3, 3]]


@pytest.mark.parametrize("lat,dt,chains", Cc.CASES, ids=[f"{'x'.join(map(str, c[0]))}-{c[1]}" for c in Cc.CASES])
def test_every_case_is_clear_of_ties(lat, dt, chains):
    """Zero ties: no link of a case has its uniform within 1e-9 of its threshold, by the restatement alone."""
    assert Cc.case(lat, dt, chains)['clear']


SMALL = [c for c in Cc.CASES if int(np.prod(c[0])) <= 256]


@pytest.mark.parametrize("lat,dt,chains", SMALL, ids=[f"{'x'.join(map(str, c[0]))}-{c[1]}" for c in SMALL])
def test_cluster_sweep_on_cpu_tensors_equals_the_restatement(lat, dt, chains):
    ref = Cc.case(lat, dt, chains)
    Cn = 3
    u, flip = Cc.draws(Cn, lat, *Cc.POS)
    phi = torch.from_numpy(ref['phi'][:Cn].copy())
    before = phi.clone()
    new, labels, stats = cluster_sweep(phi, Cc.W0, torch.from_numpy(u), torch.from_numpy(flip))
    assert torch.equal(phi, before)
    assert labels.dtype == torch.int32 and labels.shape == phi.shape and stats.dtype == torch.int32
    assert np.array_equal(labels.reshape(Cn, -1).numpy(), ref['labels'][:Cn])
    assert np.array_equal(Cc.bits(new), Cc.bits(ref['new'][:Cn]))
    assert np.array_equal(stats[:, :3].numpy(), ref['stats'][:Cn])
    V = int(np.prod(lat))
    assert (stats[:, 3] >= 1).all() and (stats[:, 3] <= V).all()


def test_cluster_sweep_worst_cases_on_cpu():
    """|phi| = 4 at w0 = 2: p = 1 exactly.  One cluster around the ring of 256, and the serpentine of (32, 32)."""
    ring = torch.full((1, 256), 4.0, dtype=F64)
    u = torch.full((1, 256, 4), 1.0 - 2.0 ** -33, dtype=F64)
    new, labels, stats = cluster_sweep(ring, 2.0, u, torch.ones((1, 256), dtype=torch.bool))
    assert (labels == 0).all() and torch.equal(new, -ring) and stats[0, :3].tolist() == [1, 256, 256]
    assert 1 <= stats[0, 3] <= 256
    s = 4.0 * Cc.serpentine()
    phi = torch.from_numpy(s)[None]
    u = torch.full((1, 1024, 4), 1.0 - 2.0 ** -33, dtype=F64)
    flip = torch.zeros((1, 1024), dtype=torch.bool)
    new, labels, stats = cluster_sweep(phi, 2.0, u, flip)
    _, want, want_stats = Cc.sweep_with(s[None], (32, 32), 2.0, u.numpy(), flip.numpy())
    assert np.array_equal(labels.reshape(1, -1).numpy(), want) and stats[0, :3].tolist() == want_stats[0].tolist()
    assert want_stats[0, 0] == 2 and 480 <= (s > 0).sum() <= 520
    assert 1 <= stats[0, 3] <= 1024


# ---------------------------------------------------------------- the sampler on CPU tensors
def test_sampler_rows_and_sweep_count_on_cpu():
    m = H.model((4, 4), F64, CPU, **H.INTERACTING)
    torch.manual_seed(3)
    m.hmc.start(n_chains=3)
    y = m.hmc.sample(3 * 5, n_chains=3, n_md=4, cluster_every=2)
    assert y.shape == (15, 4, 4)
    assert torch.equal(y[12:], m.hmc._ref['sample'])                     # row r = step r // C of chain r % C; the call ends with HMC
    cl = m.hmc.last['cluster']
    assert cl.shape == (3, 3, 4) and cl.dtype == torch.int32             # sweeps before the steps 0, 2, 4
    assert (cl[..., 0] >= 1).all() and (cl[..., 2] <= 16).all() and (cl[..., 3] >= 1).all()
    assert m.hmc.last['dh'].shape == (5, 3) and m.hmc.last['accept'].shape == (5, 3)
    assert len(m.hmc.history.accept_rate) == 1
    m.hmc.sample(3 * 4, n_chains=3, n_md=4, cluster_every=2)             # steps 5 .. 8: sweeps before 6 and 8
    assert m.hmc.last['cluster'].shape == (2, 3, 4)
    m.hmc.sample(3, n_chains=3, n_md=4, cluster_every=2)                 # step 9: none
    assert m.hmc.last['cluster'].shape == (0, 3, 4)
    m.hmc.start(n_chains=3)                                              # the count starts again
    m.hmc.sample(3, n_chains=3, n_md=4, cluster_every=2)
    assert m.hmc.last['cluster'].shape == (1, 3, 4)
    assert tuple(type(m.hmc.history)._KEYS) == ('accept_rate', 'exp_mdh', 'dh_rms')
    with pytest.raises(ValueError, match="cluster_every"):
        m.hmc.sample(3, n_chains=3, cluster_every=-1)


def test_sweep_keeps_the_even_sums_and_flips_signs_on_cpu():
    m = H.model((4, 4), F64, CPU, **H.INTERACTING)
    torch.manual_seed(5)
    phi = 1.5 * torch.randn((6, 4, 4), dtype=F64)
    before = phi.clone()
    r = m.hmc.cluster(phi)
    assert torch.equal(phi, before)
    assert torch.equal(r['phi'].abs(), phi.abs())
    assert r['labels'].shape == phi.shape and r['stats'].shape == (6, 4)
    changed = (r['phi'] != phi).flatten(1).sum(1)
    assert torch.equal(changed.to(torch.int32), r['stats'][:, 1])
    lab = r['labels'].flatten(1).long()
    # the sites of a cluster have one sign where a bond joins them, and flip together
    flipped = (r['phi'] != phi).flatten(1)
    assert torch.equal(flipped, flipped.gather(1, lab))


def test_cluster_every_zero_is_the_call_without_the_argument_on_cpu():
    m = H.model((4, 4), F64, CPU, **H.INTERACTING)
    rows = []
    for kw in ({}, dict(cluster_every=0)):
        torch.manual_seed(11)
        m.hmc.start(n_chains=2)
        rows.append((m.hmc.sample(2 * 4, n_chains=2, n_md=3, **kw), dict(m.hmc.last)))
    assert torch.equal(rows[0][0], rows[1][0])
    assert torch.equal(rows[0][1]['dh'], rows[1][1]['dh']) and set(rows[1][1]) == {'dh', 'accept'}
    torch.manual_seed(11)
    m.hmc.start(n_chains=2)
    assert not torch.equal(m.hmc.sample(2 * 4, n_chains=2, n_md=3, cluster_every=1), rows[0][0])


def test_measure_is_measure_of_the_rows_on_cpu():
    m = H.model((4, 4), F64, CPU, **H.INTERACTING)
    torch.manual_seed(13)
    m.hmc.start(n_chains=2)
    y = m.hmc.sample(2 * 5, n_chains=2, n_md=3, cluster_every=2)
    torch.manual_seed(13)
    m.hmc.start(n_chains=2)
    got = m.hmc.measure(2 * 5, n_chains=2, n_md=3, cluster_every=2)
    want = m.measure(y)
    for key in ('sum_phi', 'sum_phi2', 'sum_phi4', 'links', 'action'):
        assert torch.equal(getattr(got, key), getattr(want, key)), key


def test_device_entry_points_refuse_cpu_tensors():
    with pytest.raises(_hip.NormflowHipError):
        _hip.phi4_cluster(torch.zeros((2, 4, 4)), 0.5)
    with pytest.raises(_hip.NormflowHipError):
        _hip.phi4_cluster_draws(2, (4, 4), CPU)

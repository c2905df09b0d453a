"""Coupling ladders without a GPU: the exported symbols, every NF_EINVAL case of the three entry points, ScalarPhi4Ladder
against ScalarPhi4Action rung by rung, and LadderHMCSampler's composed path on CPU tensors (layouts, measure against
measure of the split rows, the rungs staying permutations, K identical rungs against model.hmc.sample, the exchange rule
against its numpy restatement, and the free-field ladder against the lattice propagator)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from normflow__amd import _hip
from normflow__amd.action import ScalarPhi4Ladder
from normflow__amd.lib import observables as ob
from normflow__amd.lib.observables import Ensemble
from normflow__amd.mcmc.ladder import exchange_sweep, measure_rows

import hmc_cases as H
import ladder_cases as Lc

F64 = torch.float64
CPU = torch.device("cpu")
NEW = ("nf_phi4_hmc_ladder", "nf_phi4_hmc_tiled_ladder", "nf_phi4_ladder_exchange")


def test_symbols_are_declared_exported_and_prototyped():
    header = open(os.path.join(_hip._HERE, "..", "include", "normflow_hip.h")).read()
    declared = set(re.findall(r"\b(nf_[a-z0-9_]+)\s*\(", header))
    lib = _hip.load()
    for name in NEW:
        assert name in declared and hasattr(lib, name) and name in _hip.PROTOTYPES, name
    assert f"#define NF_PHILOX_EXCHANGE_DOMAIN 0x{Lc.EXCHANGE_DOMAIN:08x}u" in header
    assert Lc.EXCHANGE_DOMAIN not in (H.ACCEPT_DOMAIN, 0x6E66686B, 0x6E666368)      # a key domain of its own


PTR = C.c_void_p(0x1000)


def _hmc(entry, **over):
    """The fused or tiled ladder entry point with valid arguments on a (4, 4) fp32 lattice except for `over`; the pointers
    are never followed, because every call here is refused before anything is launched."""
    a = dict(phi=PTR, action_out=PTR, pi_in=None, pi_out=None, dh_out=PTR, accept_out=PTR, record=None)
    if entry == "nf_phi4_hmc_ladder":
        a.update(measure_out=None)
    a.update(record_every=1, C=6, lattice=_hip._lat4((4, 4)), coef=PTR, K=3, rung=PTR, n_md=3, dt=0.1, n_traj=1,
             force_accept=0, seed=1, offset=0)
    if entry == "nf_phi4_hmc_tiled_ladder":
        a.update(workspace=PTR, workspace_bytes=1 << 30)
    a.update(dtype=_hip.NF_F32, stream=None)
    assert set(over) <= set(a), over
    a.update(over)
    lib = _hip.load()
    rc = getattr(lib, entry)(*a.values())
    return rc, lib.nf_last_error_string().decode()


HMC_EINVAL = [
    ("coef", dict(coef=None), "NULL"), ("rung", dict(rung=None), "NULL"), ("K=0", dict(K=0), "K (0)"),
    ("K=-1", dict(K=-1), "K (-1)"), ("C % K", dict(C=7), "not a multiple"),
    # and what the entry points without the ladder refuse
    ("phi", dict(phi=None), "NULL"), ("dh_out", dict(dh_out=None), "NULL"), ("lattice", dict(lattice=None), "NULL"),
    ("C=0", dict(C=0), "C (0)"), ("n_md=0", dict(n_md=0), "n_md (0)"), ("record_every=0", dict(record_every=0), "record_every (0)"),
    ("pi_in with n_traj=2", dict(pi_in=PTR, n_traj=2), "pi_in"), ("fp16", dict(dtype=_hip.NF_F16), "dtype"),
]


@pytest.mark.parametrize("entry", NEW[:2])
@pytest.mark.parametrize("name,over,word", HMC_EINVAL, ids=[e[0] for e in HMC_EINVAL])
def test_hmc_ladder_argument_validation(entry, name, over, word):
    rc, msg = _hmc(entry, **over)
    assert rc == -1 and word in msg and entry in msg, (rc, msg)


def test_hmc_ladder_caps_are_the_kernels():
    rc, msg = _hmc("nf_phi4_hmc_ladder", n_md=1024, n_traj=8192)
    assert rc == -1 and "NF_HMC_MAX_WORK" in msg and "nf_phi4_hmc_ladder" in msg
    rc, msg = _hmc("nf_phi4_hmc_ladder", n_md=1024, n_traj=257)                  # nf_phi4_hmc's last accepted product is 256
    assert rc == -1 and "NF_HMC_MAX_WORK" in msg
    rc, msg = _hmc("nf_phi4_hmc_ladder", measure_out=PTR, n_md=1024, n_traj=256)  # with measure_out: the measuring cap
    assert rc == -1 and "NF_HMC_MEASURE_MD_STEPS" in msg
    rc, msg = _hmc("nf_phi4_hmc_ladder", lattice=_hip._lat4((32, 32, 32, 32)))
    assert rc == -1 and "does not fit" in msg
    rc, msg = _hmc("nf_phi4_hmc_tiled_ladder", n_md=14, n_traj=4097)
    assert rc == -1 and "NF_HMC_TILED_MAX_LAUNCHES" in msg
    rc, msg = _hmc("nf_phi4_hmc_tiled_ladder", workspace_bytes=16)
    assert rc == -1 and "workspace" in msg


def _exchange(**over):
    a = dict(rows=PTR, row_stride=7, coef=PTR, K=3, rung=PTR, action=None, swapped=PTR, C=6, parity=0, seed=1, offset=0,
             stream=None)
    assert set(over) <= set(a), over
    a.update(over)
    lib = _hip.load()
    rc = lib.nf_phi4_ladder_exchange(*a.values())
    return rc, lib.nf_last_error_string().decode()


EXCHANGE_EINVAL = [
    ("rows", dict(rows=None), "NULL"), ("coef", dict(coef=None), "NULL"), ("rung", dict(rung=None), "NULL"),
    ("swapped", dict(swapped=None), "NULL"), ("K=0", dict(K=0), "K (0)"), ("K=1025", dict(K=1025, C=1025), "K (1025)"),
    ("C % K", dict(C=7), "multiple"), ("C=0", dict(C=0), "C (0)"), ("row_stride=6", dict(row_stride=6), "row_stride (6)"),
    ("parity=2", dict(parity=2), "parity (2)"),
]


@pytest.mark.parametrize("name,over,word", EXCHANGE_EINVAL, ids=[e[0] for e in EXCHANGE_EINVAL])
def test_exchange_argument_validation(name, over, word):
    rc, msg = _exchange(**over)
    assert rc == -1 and word in msg and "nf_phi4_ladder_exchange" in msg, (rc, msg)


def test_wrappers_refuse_host_tensors_and_bad_ladders():
    phi = torch.zeros(6, 4, 4)
    coef, rung = torch.zeros(3, 3, dtype=F64), torch.zeros(6, dtype=torch.int32)
    with pytest.raises(_hip.NormflowHipError, match="no CPU fallback"):
        _hip.phi4_hmc_ladder(phi, coef, rung, 3, 0.1)
    with pytest.raises(_hip.NormflowHipError, match="no CPU fallback"):
        _hip.ladder_exchange(torch.zeros(6, 7, dtype=F64), coef, rung, 0)
    with pytest.raises(ValueError, match="share one length"):
        ScalarPhi4Ladder(m_sq=(1.0, 2.0), lambd=(0.1, 0.2, 0.3))


# ---------------------------------------------------------------- ScalarPhi4Ladder
@pytest.mark.parametrize("lattice", [(5,), (4, 6), (1, 7), (3, 1, 4), (2, 3, 4, 5)], ids=lambda v: "x".join(map(str, v)))
def test_ladder_action_is_the_rungs_action_row_by_row(lattice):
    K = 4
    ladder = ScalarPhi4Ladder(**Lc.DISTINCT(K))
    assert len(ladder) == K
    g = torch.Generator().manual_seed(3)
    cfgs = torch.randn((11,) + lattice, generator=g, dtype=F64)
    rung = torch.randint(0, K, (11,), generator=g)
    got = ladder.action(cfgs, rung)
    for b in range(11):
        want = ladder.rung(int(rung[b])).action(cfgs[b:b + 1])[0]
        assert abs(got[b] - want) <= 1e-13 * abs(want), (b, got[b].item(), want.item())
        assert abs(want - H.ref_action(cfgs[b:b + 1], ladder.rung(int(rung[b])))[0]) <= 1e-12 * abs(want)
    # differentiable: the force of row b is the force of its rung
    x = cfgs.clone().requires_grad_(True)
    (F,) = torch.autograd.grad(ladder.action(x, rung).sum(), x)
    for b in range(11):
        want = H.ref_force(cfgs[b:b + 1], ladder.rung(int(rung[b])))[0]
        assert (F[b] - want).abs().max() <= 1e-12 * want.abs().max()


@pytest.mark.parametrize("lattice", [(6, 6), (1, 7), (3, 1, 4), (16, 16, 16)], ids=lambda v: "x".join(map(str, v)))
def test_coef_table_is_the_samplers_coef_per_rung(lattice):
    K = 3
    ladder = ScalarPhi4Ladder(**Lc.DISTINCT(K))
    table = ladder.coef_table(lattice, CPU)
    assert table.shape == (K, 3) and table.dtype == F64
    for k in range(K):
        r = ladder.rung(k)
        m = H.model(lattice, F64, CPU, kappa=r.kappa, m_sq=r.m_sq, lambd=r.lambd)
        assert table[k].tolist() == list(m.hmc._coef(lattice))
    scalar = ScalarPhi4Ladder(m_sq=-1.0, lambd=0.5, kappa=0.6)
    assert len(scalar) == 1 and scalar.coef_table(lattice, CPU).shape == (1, 3)


# ---------------------------------------------------------------- the exchange rule
def _rows(C, seed):
    g = torch.Generator().manual_seed(seed)
    phi = torch.randn((C, 4, 6), generator=g, dtype=F64)
    return phi, measure_rows(phi)


@pytest.mark.parametrize("K,R", [(2, 1), (3, 5), (8, 40), (1, 3)], ids=lambda v: str(v))
@pytest.mark.parametrize("parity", [0, 1])
def test_cpu_exchange_is_the_restated_rule(K, R, parity):
    C = K * R
    ladder = ScalarPhi4Ladder(**Lc.DISTINCT(K))
    coef = ladder.coef_table((4, 6), CPU)
    phi, rows = _rows(C, 10 + K)
    rung = Lc.permuted_rung(R, K, 20 + K)
    logu = Lc.sweep_uniforms(77, 5, R, K)
    S0 = ladder.action(phi, rung)
    new_rung, S, swapped = exchange_sweep(rows, coef, rung, S0, parity, torch.from_numpy(logu.copy()))
    want_sw, want_rung, delta = Lc.ref_exchange(rows.numpy(), coef.numpy(), rung.numpy(), parity, logu)
    tried = ~np.isnan(delta)
    assert tried.sum() == R * len(range(parity, K - 1, 2))
    clear = Lc.clear_of_ties(delta, logu) & tried
    assert (tried & ~clear).sum() <= 0.01 * max(tried.sum(), 1)
    assert np.array_equal(swapped.numpy()[clear], want_sw[clear]) and not swapped.numpy()[~tried].any()
    if clear.sum() == tried.sum():
        assert np.array_equal(new_rung.numpy(), want_rung)
    if K >= 3:
        assert 0 < swapped.sum() < tried.sum()                # both outcomes occur
    # permutation kept, the actions are those of the new rungs
    assert torch.equal(new_rung.reshape(R, K).sort(dim=1).values, torch.arange(K, dtype=torch.int32).expand(R, K))
    want_S = ladder.action(phi, new_rung)
    assert ((S - want_S).abs() / want_S.abs().clamp_min(1.0)).max() <= 1e-12


def test_measure_rows_have_the_kernels_layout():
    phi = torch.randn(3, 1, 5, dtype=F64)
    rows = measure_rows(phi)
    assert rows.shape == (3, 7 + 1 + 1 + 1 + 5)
    assert torch.allclose(rows[:, 1], (phi ** 2).flatten(1).sum(1)) and bool((rows[:, 3:6] == 0).all())
    assert torch.allclose(rows[:, 6], (phi * phi.roll(1, dims=2)).flatten(1).sum(1))
    assert torch.equal(rows[:, 7], rows[:, 0]) and torch.equal(rows[:, 9], rows[:, 0])
    assert torch.allclose(rows[:, 10:], phi[:, 0])


# ---------------------------------------------------------------- LadderHMCSampler on CPU tensors
def _sampler(lattice=(4, 4), couplings=None, dtype=F64):
    m, ladder = Lc.model(lattice, dtype, CPU, **(couplings or Lc.DISTINCT(3)))
    return m, ladder, m.hmc.ladder(ladder)


def test_layouts_and_measure_of_the_split_rows():
    K, R, steps = 3, 4, 5                       # sweeps after steps 2 and 4: the last rows are ordered by the final rungs
    C = K * R
    m, ladder, s = _sampler()
    kw = dict(n_chains=C, n_md=3, dt=0.1, n_skip=1, exchange_every=2)
    torch.manual_seed(5)
    s.start(n_chains=C)
    state = torch.get_rng_state()
    y = s.sample(steps * C, **kw)
    assert y.shape == (steps * C, 4, 4) and s.last['dh'].shape == (2 * steps, C) and s.last['swapped'].shape == (2, R, K - 1)
    parts = s.split(y)
    assert parts.shape == (K, steps * R, 4, 4)
    rows = y.reshape(steps, R, K, 4, 4)
    for k in range(K):
        assert torch.equal(parts[k].reshape(steps, R, 4, 4), rows[:, :, k])
    # the last rows are the chains' states, by rung; _ref is indexed by chain
    rung = s._ref['rung'].long()
    col = (torch.arange(C) // K) * K + rung
    assert torch.equal(y[-C:][col], s._ref['sample'])
    assert torch.equal(rung.reshape(R, K).sort(dim=1).values, torch.arange(K).expand(R, K))
    want_S = ladder.action(s._ref['sample'], rung)
    assert ((s._ref['action'] - want_S).abs() / want_S.abs().clamp_min(1.0)).max() <= 1e-12
    hist = s.history
    assert len(hist.exchange_rate) == 1 and len(hist.exchange_rate[0]) == K - 1 and len(hist.accept_rate) == 1
    # measure from the same chain and generator state
    torch.manual_seed(5)
    s.start(n_chains=C)
    torch.set_rng_state(state)
    ms = s.measure(steps * C, **kw)
    assert len(ms) == K
    for k in range(K):
        want = ob.measure(parts[k], action=ladder.rung(k))
        assert torch.equal(ms[k].sum_phi2, want.sum_phi2) and torch.equal(ms[k].links, want.links)
        assert torch.equal(ms[k].sum_phi, want.sum_phi) and torch.equal(ms[k].sum_phi4, want.sum_phi4)
        assert all(torch.equal(a, b) for a, b in zip(ms[k].slices, want.slices))
        assert torch.equal(ms[k].action, want.action)
        assert torch.allclose(ms[k].action, ladder.rung(k).action(parts[k]), rtol=1e-12, atol=0)
        e = Ensemble(ms[k], n_chains=R)
        assert len(ms[k]) == steps * R and e is not None


def test_rungs_stay_permutations_and_parity_alternates_across_calls():
    K, R = 4, 6
    C = K * R
    m, ladder, s = _sampler(couplings=dict(kappa=0.5, lambd=0.4, m_sq=(-1.0, -0.9, -0.8, -0.7)))
    torch.manual_seed(6)
    s.start(n_chains=C)
    seen = []
    for call in range(5):
        s.sample(3 * C, n_chains=C, n_md=2, dt=0.15, exchange_every=1)
        sw = s.last['swapped']
        assert sw.shape == (3, R, K - 1)
        for i in range(3):
            parity = (3 * call + i) % 2                          # the count persists across calls
            assert not sw[i][:, [k for k in range(K - 1) if k % 2 != parity]].any()
            seen.append(int(sw[i].sum()))
        rung = s._ref['rung']
        assert rung.dtype == torch.int32
        assert torch.equal(rung.reshape(R, K).sort(dim=1).values, torch.arange(K, dtype=torch.int32).expand(R, K))
    assert sum(seen) > 0 and not torch.equal(s._ref['rung'], (torch.arange(C) % K).to(torch.int32))
    assert all(0.0 <= r <= 1.0 for r in s.history.exchange_rate[-1]) and len(s.history.exchange_rate) == 5
    s.start(n_chains=C)
    assert s._sweeps == 0 and torch.equal(s._ref['rung'], (torch.arange(C) % K).to(torch.int32))
    s.sample(C, n_chains=C, n_md=2, dt=0.15, exchange_every=0)
    assert s.last['swapped'].shape[0] == 0 and all(np.isnan(r) for r in s.history.exchange_rate[-1])


def test_identical_rungs_without_exchange_walk_the_plain_samplers_chain():
    K, C = 3, 6
    m, ladder, s = _sampler(couplings=dict(kappa=[H.INTERACTING['kappa']] * K, m_sq=H.INTERACTING['m_sq'],
                                           lambd=H.INTERACTING['lambd']))
    kw = dict(n_chains=C, n_md=4, dt=0.12, n_skip=1)
    torch.manual_seed(8)
    plain = m.hmc.sample(5 * C, **kw)
    torch.manual_seed(8)
    got = s.sample(5 * C, exchange_every=0, **kw)
    assert torch.equal(got, plain)
    assert torch.equal(s.last['dh'], m.hmc.last['dh']) and torch.equal(s.last['accept'], m.hmc.last['accept'])
    assert s.history.accept_rate == m.hmc.history.accept_rate


def test_argument_errors():
    m, ladder, s = _sampler()
    with pytest.raises(ValueError, match="multiple of the K = 3 rungs"):
        s.sample(8, n_chains=4)
    with pytest.raises(ValueError, match="multiple of n_chains"):
        s.sample(7, n_chains=6)
    with pytest.raises(ValueError, match="exchange_every"):
        s.sample(6, n_chains=6, exchange_every=-1)
    with pytest.raises(_hip.NormflowHipError, match="fused"):
        s.sample(6, n_chains=6, path='fused')


def test_free_field_ladder_with_exchanges():
    """The reference run of the device test (tests/test_hmc_ladder.py), composed in fp64 on the CPU: per rung the exact
    <phi^2> within 5 standard errors, and the error inside the 2 % cap the device test asserts."""
    K, R = 4, 64
    m, ladder, s = _sampler((16,), Lc.FREE_LADDER)
    torch.manual_seed(31)
    y = s.sample(K * R * 160, n_chains=K * R, n_md=3, dt=0.4, exchange_every=1)
    assert abs(Lc.free_phi2(1.5, 0.25) - H.FREE_PHI2) < 5e-5
    for k, yk in enumerate(s.split(y)):
        exact = Lc.free_phi2(Lc.FREE_LADDER['m_sq'][k], 0.25)
        mean, err = Lc.rung_stats(yk, R, drop=30)
        print(f"free ladder rung {k}: <phi^2> {mean:.5f} +- {err:.5f} ({(mean - exact) / err:+.2f} sigma of {exact:.5f})")
        assert abs(mean - exact) <= 5 * err and err <= 0.02 * exact
    assert all(0.0 < r < 1.0 for r in s.history.exchange_rate[-1])
    assert 0.7 < s.history.accept_rate[-1] < 0.97

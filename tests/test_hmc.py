"""nf_phi4_hmc (the LDS-resident HMC kernel) and HMCSampler on the device.

The fused kernel is held to the composed path (nf_normal_sample, the action's VJP, torch ops, nf_block_accept), which the
host tests hold to the fp64 restatement of tests/hmc_cases.py and to exact results.  fp64: both paths from the same
Philox position agree to 1e-11 of the largest entry in phi and pi and to 1e-9 in dH, and take the same decisions away
from ties (|log u + dH| <= 1e-6, u restated on the host).  fp32: momenta handed in; the reference is the composed path in
fp64 and the bound 4 x the error the composed path makes in fp32 on the same inputs (two independent roundings per
operation and the kernel's contracted multiply-adds), floor 1e-6 of the largest entry; dH: that multiple + 1e-4."""
import numpy as np
import pytest
import torch

from normflow__amd import _hip

import hmc_cases as H
from hmc_cases import DEV, field as _field, rel as _rel

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
LATTICES = [(5,), (1, 7), (2, 6), (16, 16), (17, 16), (5, 7, 9), (3, 4, 5), (2, 3, 4, 5), (16, 16, 16)]
CHAINS = [1, 3, 300]
N_MD, DT = 5, 0.1
# and the chains of more than 4096 sites: 8 and 16 sites per lane, and an LDS image above the default 64 KiB limit
CASES64 = [(lat, C) for lat in LATTICES for C in CHAINS] + [((8192,), 2)]
CASES32 = [(lat, C) for lat in LATTICES for C in CHAINS] + [((90, 90), 2), ((24, 24, 24), 2), ((128, 128), 2)]
_case = lambda v: f"{'x'.join(map(str, v[0]))}-C{v[1]}"
_name = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v).replace("torch.", "")


@pytest.mark.parametrize("case", CASES64, ids=_case)
def test_fused_matches_composed_fp64(case, parity_report):
    lattice, C = case
    m = H.model(lattice, F64, DEV, **H.INTERACTING)
    phi0 = _field((C,) + lattice, F64, 100 + C)
    pos = (0x1234567 + C, 40)
    run = lambda path, force: m.hmc.trajectory(phi0, N_MD, DT, force_accept=force, path=path, position=pos)
    f, c = run('fused', True), run('composed', True)
    assert bool(f['accept'].all()) and bool(c['accept'].all())
    case = f"hmc fp64 {_name(lattice)} C={C}"
    for key, bound in (('phi', 1e-11), ('pi', 1e-11)):
        err = _rel(f[key], c[key])
        parity_report(case, key, err, bound)
        assert err <= bound, (case, key, err)
    e_dh = (f['dh'] - c['dh']).abs().max().item()
    parity_report(case, 'dH (abs)', e_dh, 1e-9)
    assert e_dh <= 1e-9
    e_s = ((f['action'] - c['action']).abs() / c['action'].abs().clamp_min(1.0)).max().item()
    assert e_s <= 1e-12, e_s
    # the decision: the same flags away from ties, and they are the documented rule on the restated uniform
    f, c = run('fused', False), run('composed', False)
    logu = H.log_uniforms(pos[0], pos[1] + 1, C)
    dh = c['dh'].cpu().numpy()
    clear = np.abs(logu + dh) > 1e-6
    assert (~clear).sum() <= 0.02 * C
    fa, ca = f['accept'].cpu().numpy().astype(bool), c['accept'].cpu().numpy().astype(bool)
    assert np.array_equal(fa[clear], ca[clear]) and np.array_equal(fa[clear], (logu < -dh)[clear])
    keep = torch.as_tensor(~fa, device=DEV)
    assert torch.equal(f['phi'][keep], phi0[keep])            # rejected: the old bits


@pytest.mark.parametrize("case", CASES32, ids=_case)
def test_fused_fp32(case, parity_report):
    lattice, C = case
    m32, m64 = H.model(lattice, F32, DEV, **H.INTERACTING), H.model(lattice, F64, DEV, **H.INTERACTING)
    phi0, pi0 = _field((C,) + lattice, F32, 200 + C), _field((C,) + lattice, F32, 300 + C, scale=1.0)
    pos = (77, 8)
    ref = m64.hmc.trajectory(phi0.double(), N_MD, DT, pi=pi0.double(), force_accept=True, path='composed', position=pos)
    c32 = m32.hmc.trajectory(phi0, N_MD, DT, pi=pi0, force_accept=True, path='composed', position=pos)
    f32 = m32.hmc.trajectory(phi0, N_MD, DT, pi=pi0, force_accept=True, path='fused', position=pos)
    assert f32['phi'].dtype == F32 and f32['dh'].dtype == F64
    H.fp32_bounds(f"hmc fp32 {_name(lattice)} C={C}", f32, c32, ref, parity_report)


def test_fused_fp32_draws_the_momenta_of_normal_sample(parity_report):
    """fp32 with the momenta DRAWN, on a lattice whose last Philox group is ragged (315 sites, groups of 4): the kernel's
    draw and its transit through the LDS image against nf_normal_sample at the same position.  A momentum at the wrong
    site is an error of order 1; the bound is the fp32 parity bound above."""
    lattice, C = (5, 7, 9), 3
    m32, m64 = H.model(lattice, F32, DEV, **H.INTERACTING), H.model(lattice, F64, DEV, **H.INTERACTING)
    phi0 = _field((C,) + lattice, F32, 250)
    pos = (4242, 16)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(pos[0])
    gen.set_offset(4 * pos[1])
    pi0 = _hip.normal_sample(None, None, C, lattice, F32, DEV, generator=gen)[0]      # the documented stream, fp32
    ref = m64.hmc.trajectory(phi0.double(), N_MD, DT, pi=pi0.double(), force_accept=True, path='composed', position=pos)
    c32 = m32.hmc.trajectory(phi0, N_MD, DT, force_accept=True, path='composed', position=pos)
    f32 = m32.hmc.trajectory(phi0, N_MD, DT, force_accept=True, path='fused', position=pos)
    H.fp32_bounds("hmc fp32 drawn momenta 5x7x9 C=3", f32, c32, ref, parity_report)


def _launch(*args, **kw):
    return H.launch(_hip.phi4_hmc, *args, **kw)


@pytest.mark.parametrize("dtype", [F32, F64], ids=_name)
@pytest.mark.parametrize("lattice", [(6, 6), (16, 16, 16)], ids=_name)
def test_the_loop_inside_the_launch(lattice, dtype):
    """n_traj = 8, record_every = 2 in one launch == eight launches of one trajectory at offsets offset + 2 t, bitwise."""
    C = 6
    m = H.model(lattice, dtype, DEV, **H.INTERACTING)
    coef = m.hmc._coef(lattice)
    phi0 = _field((C,) + lattice, dtype, 400)
    seed, off = 99, 1000
    phi_a, a = _launch(phi0, coef, 8, (seed, off), record_every=2)
    phi_b, dh, acc, rec = phi0, [], [], []
    for t in range(8):
        phi_b, b = _launch(phi_b, coef, 1, (seed, off + 2 * t))
        dh.append(b['dh'][0]); acc.append(b['accept'][0])
        if t % 2 == 1:
            rec.append(phi_b)
    print(f"loop {_name(lattice)} {_name(dtype)}: accepted {int(a['accept'].sum())} of {a['accept'].numel()}")
    assert a['record'].shape == (4, C) + lattice
    assert torch.equal(phi_a, phi_b) and torch.equal(a['record'], torch.stack(rec))
    assert torch.equal(a['dh'], torch.stack(dh)) and torch.equal(a['accept'], torch.stack(acc))
    assert torch.equal(a['action'], b['action'])
    assert torch.equal(a['record'][-1], phi_a)


@pytest.mark.parametrize("dtype", [F32, F64], ids=_name)
def test_reject_and_restore(dtype):
    """dt = 1.5, n_md = 20: the integrator is unstable and dH enormous (or not a number); the rejected chains keep their
    bits and action_out is S of the start; force_accept takes the proposal whatever dH is."""
    lattice, C = (16, 16), 40
    m = H.model(lattice, dtype, DEV, **H.INTERACTING)
    coef = m.hmc._coef(lattice)
    phi0 = _field((C,) + lattice, dtype, 500, scale=0.05)
    phi, r = _launch(phi0, coef, 1, (5, 0), n_md=20, dt=1.5)
    rej = r['accept'][0] == 0
    assert int(rej.sum()) >= C // 2, "dt = 1.5 should reject nearly everything"
    assert torch.equal(phi[rej], phi0[rej])
    s0 = H.ref_action(phi0.double().cpu(), m.action)
    got = r['action'].cpu()
    assert ((got - s0).abs() / s0.abs().clamp_min(1.0))[rej.cpu()].max().item() <= 1e-12
    phi_f, rf = _launch(phi0, coef, 1, (5, 0), n_md=20, dt=1.5, force_accept=True, want_pi=True)
    assert bool(rf['accept'].all())
    assert bool((phi_f != phi0).flatten(1).any(1).all())                 # every chain moved
    assert torch.equal(rf['dh'].isnan(), r['dh'].isnan()) and torch.equal(rf['dh'].nan_to_num(), r['dh'].nan_to_num())
    acc = ~rej
    assert torch.equal(phi[acc].nan_to_num(), phi_f[acc].nan_to_num())   # an accepted chain holds that proposal


def test_reversibility_on_the_device(parity_report):
    lattice, C = (5, 7, 9), 4
    m = H.model(lattice, F64, DEV, **H.INTERACTING)
    phi0, pi0 = _field((C,) + lattice, F64, 600), _field((C,) + lattice, F64, 601, scale=1.0)
    a = m.hmc.trajectory(phi0, 10, 0.1, pi=pi0, force_accept=True, path='fused')
    b = m.hmc.trajectory(a['phi'], 10, 0.1, pi=-a['pi'], force_accept=True, path='fused')
    e_phi, e_pi = (b['phi'] - phi0).abs().max().item(), (b['pi'] + pi0).abs().max().item()
    parity_report("hmc reversibility 5x7x9 fp64", "|phi2 - phi0|", e_phi, 1e-11)
    parity_report("hmc reversibility 5x7x9 fp64", "|pi2 + pi0|", e_pi, 1e-11)
    assert e_phi <= 1e-11 and e_pi <= 1e-11
    # and the trajectory is the restatement's
    phi1, pi1, dh = H.ref_trajectory(phi0, pi0, m.action, 10, 0.1)
    assert (a['phi'].cpu() - phi1).abs().max().item() <= 1e-11 and (a['dh'].cpu() - dh).abs().max().item() <= 1e-9


def test_sampler_end_to_end():
    lattice, C = (6, 6), 8
    m = H.model(lattice, F64, DEV, **H.INTERACTING)
    phi0 = _field((C,) + lattice, F64, 700)
    kw = dict(n_chains=C, n_md=5, dt=0.15)

    def run(seed, calls, rows, path):
        torch.manual_seed(seed)
        m.hmc.start(phi0)
        return torch.cat([m.hmc.sample(rows * C, path=path, **kw) for _ in range(calls)])

    one = run(3, 1, 20, 'fused')
    assert one.shape == (20 * C,) + lattice
    assert torch.equal(one[-C:], m.hmc._ref['sample'])                   # the rows are the chains' states
    s_ref = H.ref_action(m.hmc._ref['sample'].cpu(), m.action)
    assert ((m.hmc._ref['action'].cpu() - s_ref).abs() / s_ref.abs().clamp_min(1.0)).max().item() <= 1e-12
    dh_f, acc_f = m.hmc.last['dh'].cpu().numpy(), m.hmc.last['accept'].cpu().numpy().astype(bool)
    assert 0 < acc_f.sum() < acc_f.size
    assert torch.equal(one, run(3, 1, 20, 'fused'))                      # torch.manual_seed governs the sampler
    assert not torch.equal(one, run(4, 1, 20, 'fused'))
    assert torch.equal(one, run(3, 2, 10, 'fused'))                      # two calls of k rows == one call of 2k rows
    assert torch.equal(one, run(3, 1, 20, None))                         # the default takes the fused kernel here
    # composed from the same seed: the same decisions away from ties, the same samples up to rounding
    torch.manual_seed(3)
    gen = torch.cuda.default_generators[0]
    seed, off = gen.initial_seed(), gen.get_offset() // 4
    comp = run(3, 1, 20, 'composed')
    acc_c = m.hmc.last['accept'].cpu().numpy().astype(bool)
    logu = np.stack([H.log_uniforms(seed, off + 2 * t + 1, C) for t in range(20)])
    assert (np.abs(logu + dh_f) > 1e-6).all(), "a tie within 1e-6 in 160 decisions: pick another seed"
    assert np.array_equal(acc_f, acc_c) and np.array_equal(acc_f, logu < -dh_f)
    assert (one - comp).abs().max().item() <= 1e-9
    y, logp = m.hmc.sample_(2 * C, **kw)
    assert logp.dtype == F64 and torch.allclose(logp, -m.action(y), rtol=0, atol=0)


def _count_launches(monkeypatch):
    calls, real = [], _hip.phi4_hmc

    def counted(*a, **k):
        calls.append(k.get('n_traj'))
        return real(*a, **k)
    monkeypatch.setattr(_hip, "phi4_hmc", counted)
    return calls


def test_free_field_distribution_fused_fp32(monkeypatch):
    calls = _count_launches(monkeypatch)
    torch.manual_seed(21)
    m = H.model((16,), F32, DEV, **H.FREE)
    y = m.hmc.sample(256 * 160, n_chains=256, n_md=3, dt=0.4, path='fused')
    assert calls == [160]                                                # one launch: 3 * 160 * 256 is far below the cap
    mean, err = H.chain_stats(y, 256, drop=30)
    rate = m.hmc.history.accept_rate[-1]
    print(f"free field, fused fp32: <phi^2> {mean:.5f} +- {err:.5f} ({(mean - H.FREE_PHI2) / err:+.2f} sigma), accept rate {rate:.3f}")
    assert abs(mean - H.FREE_PHI2) <= 5 * err
    assert 0.7 < rate < 0.97


def test_interacting_chain_against_quadrature_fused_fp32(monkeypatch):
    calls = _count_launches(monkeypatch)
    exact = H.quadrature_phi2()
    torch.manual_seed(22)
    m = H.model((4,), F32, DEV, **H.INTERACTING)
    y = m.hmc.sample(256 * 260, n_chains=256, n_md=4, dt=0.25, path='fused')
    assert calls == [260]
    mean, err = H.chain_stats(y, 256, drop=30)
    e = torch.exp(-m.hmc.last['dh'][30:]).flatten().cpu()
    e_mean, e_err = e.mean().item(), e.std().item() / e.numel() ** 0.5
    print(f"(4,) chain, fused fp32: <phi^2> {mean:.5f} +- {err:.5f} ({(mean - exact) / err:+.2f} sigma of {exact:.6f}), "
          f"<exp(-dH)> - 1 = {e_mean - 1:+.2e} +- {e_err:.2e}, accept rate {m.hmc.history.accept_rate[-1]:.3f}")
    assert abs(mean - exact) <= 5 * err
    assert abs(e_mean - 1.0) <= 5 * e_err


def test_long_runs_are_split_at_the_work_cap(monkeypatch):
    """A run above NF_HMC_MAX_WORK goes in several launches and equals the same run under a cap that needs none."""
    lattice, C = (6, 6), 3
    m = H.model(lattice, F32, DEV, **H.INTERACTING)
    phi0 = _field((C,) + lattice, F32, 800)
    torch.manual_seed(5)
    whole = m.hmc.start(phi0).sample(12 * C, n_chains=C, n_md=2, dt=0.1, n_skip=1)
    calls = _count_launches(monkeypatch)
    monkeypatch.setattr(_hip, "HMC_MAX_WORK", 2 * 256 * 10)             # ten trajectories per launch: five rows of two
    torch.manual_seed(5)
    split = m.hmc.start(phi0).sample(12 * C, n_chains=C, n_md=2, dt=0.1, n_skip=1)
    assert calls == [10, 10, 4] and torch.equal(whole, split)
    calls.clear()
    monkeypatch.setattr(_hip, "HMC_MAX_WORK", 2 * 256)                  # one trajectory per launch: a row needs two
    torch.manual_seed(5)
    assert torch.equal(whole, m.hmc.start(phi0).sample(12 * C, n_chains=C, n_md=2, dt=0.1, n_skip=1))
    assert calls == [1] * 24


def test_graph_capture():
    """The launch neither allocates nor synchronises: captured and replayed once it equals the eager call, bitwise."""
    lattice, C = (16, 16), 5
    m = H.model(lattice, F32, DEV, **H.INTERACTING)
    coef = m.hmc._coef(lattice)
    phi0 = _field((C,) + lattice, F32, 900)
    pos = (31, 64)
    phi_e, e = _launch(phi0, coef, 6, pos, record_every=3)
    static = phi0.clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        r = _hip.phi4_hmc(static, *coef, 4, 0.1, n_traj=6, record_every=3, position=pos)
    torch.cuda.synchronize()
    assert torch.equal(static, phi0)                                     # capture ran nothing
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(static, phi_e) and torch.equal(r['record'], e['record'])
    assert torch.equal(r['dh'], e['dh']) and torch.equal(r['accept'], e['accept']) and torch.equal(r['action'], e['action'])

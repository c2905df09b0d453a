"""nf_phi4_hmc_tiled (the HMC kernels for chains in HBM) and HMCSampler(path='tiled') on the device.

The tiled kernels are held to the composed path and to the resident kernel with the bounds of tests/test_hmc.py: fp64
from the same Philox position 1e-11 of the largest entry in phi and pi, 1e-9 in dH, 1e-12 relative in the action, the same
decisions away from ties (|log u + dH| <= 1e-6, u restated on the host); fp32 with the momenta handed in against the
composed path in fp64, bound 4 x the composed path's own fp32 error (floor 1e-6 of the largest entry; dH: + 1e-4).  The
cases and the regimes they reach are tests/hmc_tiled_cases.py's (checked on the host by tests/test_hmc_tiled_host.py)."""
import numpy as np
import pytest
import torch

from normflow__amd import _hip

import hmc_cases as H
import hmc_tiled_cases as TC
from hmc_cases import DEV, field as _field, fp32_bounds as _fp32_bounds, rel as _rel

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
N_MD, DT = 5, 0.1
_name = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v).replace("torch.", "")


@pytest.mark.parametrize("case", TC.cases(F64), ids=TC.case_id)
def test_tiled_matches_composed_fp64(case, parity_report):
    lattice, C = case
    m = H.model(lattice, F64, DEV, **H.INTERACTING)
    phi0 = _field((C,) + lattice, F64, 100 + C)
    pos = (0x1234567 + C, 40)
    run = lambda path, force: m.hmc.trajectory(phi0, N_MD, DT, force_accept=force, path=path, position=pos)
    f, c = run('tiled', True), run('composed', True)
    assert bool(f['accept'].all()) and bool(c['accept'].all())
    name = f"hmc tiled fp64 {_name(lattice)} C={C}"
    for key, bound in (('phi', 1e-11), ('pi', 1e-11)):
        err = _rel(f[key], c[key])
        parity_report(name, key, err, bound)
        assert err <= bound, (name, key, err)
    e_dh = (f['dh'] - c['dh']).abs().max().item()
    parity_report(name, 'dH (abs)', e_dh, 1e-9)
    assert e_dh <= 1e-9
    e_s = ((f['action'] - c['action']).abs() / c['action'].abs().clamp_min(1.0)).max().item()
    assert e_s <= 1e-12, e_s
    f, c = run('tiled', False), run('composed', False)
    logu = H.log_uniforms(pos[0], pos[1] + 1, C)
    dh = c['dh'].cpu().numpy()
    clear = np.abs(logu + dh) > 1e-6
    assert (~clear).sum() <= 0.02 * C
    fa, ca = f['accept'].cpu().numpy().astype(bool), c['accept'].cpu().numpy().astype(bool)
    assert np.array_equal(fa[clear], ca[clear]) and np.array_equal(fa[clear], (logu < -dh)[clear])
    keep = torch.as_tensor(~fa, device=DEV)
    assert torch.equal(f['phi'][keep], phi0[keep])            # rejected: the old bits


@pytest.mark.parametrize("case", TC.cases(F32), ids=TC.case_id)
def test_tiled_fp32(case, parity_report):
    lattice, C = case
    m32, m64 = H.model(lattice, F32, DEV, **H.INTERACTING), H.model(lattice, F64, DEV, **H.INTERACTING)
    phi0, pi0 = _field((C,) + lattice, F32, 200 + C), _field((C,) + lattice, F32, 300 + C, scale=1.0)
    pos = (77, 8)
    ref = m64.hmc.trajectory(phi0.double(), N_MD, DT, pi=pi0.double(), force_accept=True, path='composed', position=pos)
    c32 = m32.hmc.trajectory(phi0, N_MD, DT, pi=pi0, force_accept=True, path='composed', position=pos)
    f32 = m32.hmc.trajectory(phi0, N_MD, DT, pi=pi0, force_accept=True, path='tiled', position=pos)
    assert f32['phi'].dtype == F32 and f32['dh'].dtype == F64
    _fp32_bounds(f"hmc tiled fp32 {_name(lattice)} C={C}", f32, c32, ref, parity_report)


def test_tiled_fp32_draws_the_momenta_of_normal_sample(parity_report):
    """fp32 with the momenta DRAWN, (5, 7, 9): 315 sites, the last Philox group of four is cut and no row is a multiple of
    four sites, so every site draws its group for itself.  A momentum at the wrong site is an error of order 1."""
    lattice, C = (5, 7, 9), 3
    m32, m64 = H.model(lattice, F32, DEV, **H.INTERACTING), H.model(lattice, F64, DEV, **H.INTERACTING)
    phi0 = _field((C,) + lattice, F32, 250)
    pos = (4242, 16)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(pos[0])
    gen.set_offset(4 * pos[1])
    pi0 = _hip.normal_sample(None, None, C, lattice, F32, DEV, generator=gen)[0]
    ref = m64.hmc.trajectory(phi0.double(), N_MD, DT, pi=pi0.double(), force_accept=True, path='composed', position=pos)
    c32 = m32.hmc.trajectory(phi0, N_MD, DT, force_accept=True, path='composed', position=pos)
    f32 = m32.hmc.trajectory(phi0, N_MD, DT, force_accept=True, path='tiled', position=pos)
    _fp32_bounds("hmc tiled fp32 drawn momenta 5x7x9 C=3", f32, c32, ref, parity_report)


@pytest.mark.parametrize("lattice", [(16, 16), (5, 7, 9), (16, 16, 16)], ids=_name)
def test_tiled_matches_resident_fp64(lattice, parity_report):
    C = 300
    m = H.model(lattice, F64, DEV, **H.INTERACTING)
    phi0 = _field((C,) + lattice, F64, 150)
    pos = (991, 12)
    run = lambda path, force: m.hmc.trajectory(phi0, N_MD, DT, force_accept=force, path=path, position=pos)
    t, f = run('tiled', True), run('fused', True)
    name = f"hmc tiled vs resident fp64 {_name(lattice)}"
    for key in ('phi', 'pi'):
        err = _rel(t[key], f[key])
        parity_report(name, key, err, 1e-11)
        assert err <= 1e-11, (name, key, err)
    e_dh = (t['dh'] - f['dh']).abs().max().item()
    parity_report(name, 'dH (abs)', e_dh, 1e-9)
    assert e_dh <= 1e-9
    t, f = run('tiled', False), run('fused', False)
    logu = H.log_uniforms(pos[0], pos[1] + 1, C)
    clear = np.abs(logu + f['dh'].cpu().numpy()) > 1e-6
    assert (~clear).sum() <= 0.02 * C
    ta, fa = t['accept'].cpu().numpy().astype(bool), f['accept'].cpu().numpy().astype(bool)
    assert np.array_equal(ta[clear], fa[clear]) and 0 < ta.sum()


def _launch(*args, **kw):
    return H.launch(_hip.phi4_hmc_tiled, *args, **kw)


@pytest.mark.parametrize("dtype", [F32, F64], ids=_name)
@pytest.mark.parametrize("lattice", [(6, 6), (12, 12, 12, 12)], ids=_name)
def test_the_loop_inside_the_call(lattice, dtype):
    """n_traj = 8, record_every = 2 in one call == eight calls of one trajectory at offsets offset + 2 t, bitwise."""
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
def test_chain_independence(dtype):
    """The rows of chains run together equal, bitwise, the same chains run alone with the momenta handed in."""
    lattice, C = (2, 13, 13, 64), 5                      # several tiles per chain on every tiled axis
    assert _hip.hmc_tiled_plan(lattice, dtype)['tiles'] >= 3
    m = H.model(lattice, dtype, DEV, **H.INTERACTING)
    coef = m.hmc._coef(lattice)
    phi0, pi0 = _field((C,) + lattice, dtype, 450), _field((C,) + lattice, dtype, 451, scale=1.0)
    pos = (17, 4)
    phi_all, r_all = _launch(phi0, coef, 1, pos, pi_in=pi0, want_pi=True, force_accept=True)
    for c in (0, 3, 4):
        phi_c, r_c = _launch(phi0[c:c + 1], coef, 1, pos, pi_in=pi0[c:c + 1].contiguous(), want_pi=True, force_accept=True)
        assert torch.equal(phi_c[0], phi_all[c]) and torch.equal(r_c['pi'][0], r_all['pi'][c])
        assert torch.equal(r_c['dh'][0, 0], r_all['dh'][0, c]) and torch.equal(r_c['action'][0], r_all['action'][c])


@pytest.mark.parametrize("dtype", [F32, F64], ids=_name)
def test_workspace_contents_do_not_matter(dtype):
    lattice, C = (40, 40, 24), 2
    m = H.model(lattice, dtype, DEV, **H.INTERACTING)
    coef = m.hmc._coef(lattice)
    phi0 = _field((C,) + lattice, dtype, 460)
    need = _hip.load().nf_phi4_hmc_tiled_workspace(C, _hip._lat4(lattice), _hip._dtype_code(phi0))
    outs = []
    for fill in (float('nan'), 0.0, 0.0):
        ws = torch.full((need // 8 + 1,), fill, dtype=F64, device=DEV).view(torch.uint8)
        phi, r = _launch(phi0, coef, 3, (8, 8), record_every=1, want_pi=True, workspace=ws)
        outs.append((phi, r['record'], r['pi'], r['dh'], r['accept'], r['action']))
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert torch.equal(a, b)
    assert not outs[0][3].isnan().any()


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
    lattice, C = (2, 13, 13, 64), 2
    m = H.model(lattice, F64, DEV, **H.INTERACTING)
    phi0, pi0 = _field((C,) + lattice, F64, 600), _field((C,) + lattice, F64, 601, scale=1.0)
    a = m.hmc.trajectory(phi0, 10, 0.1, pi=pi0, force_accept=True, path='tiled')
    b = m.hmc.trajectory(a['phi'], 10, 0.1, pi=-a['pi'], force_accept=True, path='tiled')
    e_phi, e_pi = (b['phi'] - phi0).abs().max().item(), (b['pi'] + pi0).abs().max().item()
    parity_report("hmc tiled reversibility 2x13x13x64 fp64", "|phi2 - phi0|", e_phi, 1e-11)
    parity_report("hmc tiled reversibility 2x13x13x64 fp64", "|pi2 + pi0|", e_pi, 1e-11)
    assert e_phi <= 1e-11 and e_pi <= 1e-11
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

    one = run(3, 1, 20, 'tiled')
    assert one.shape == (20 * C,) + lattice
    assert torch.equal(one[-C:], m.hmc._ref['sample'])                   # the rows are the chains' states
    s_ref = H.ref_action(m.hmc._ref['sample'].cpu(), m.action)
    assert ((m.hmc._ref['action'].cpu() - s_ref).abs() / s_ref.abs().clamp_min(1.0)).max().item() <= 1e-12
    dh_t, acc_t = m.hmc.last['dh'].cpu().numpy(), m.hmc.last['accept'].cpu().numpy().astype(bool)
    assert 0 < acc_t.sum() < acc_t.size
    assert torch.equal(one, run(3, 1, 20, 'tiled'))                      # torch.manual_seed governs the sampler
    assert not torch.equal(one, run(4, 1, 20, 'tiled'))
    assert torch.equal(one, run(3, 2, 10, 'tiled'))                      # two calls of k rows == one call of 2k rows
    torch.manual_seed(3)
    gen = torch.cuda.default_generators[0]
    seed, off = gen.initial_seed(), gen.get_offset() // 4
    comp = run(3, 1, 20, 'composed')
    acc_c = m.hmc.last['accept'].cpu().numpy().astype(bool)
    logu = np.stack([H.log_uniforms(seed, off + 2 * t + 1, C) for t in range(20)])
    assert (np.abs(logu + dh_t) > 1e-6).all(), "a tie within 1e-6 in 160 decisions: pick another seed"
    assert np.array_equal(acc_t, acc_c) and np.array_equal(acc_t, logu < -dh_t)
    assert (one - comp).abs().max().item() <= 1e-9
    # a lattice beyond the resident kernel: the default takes the tiled kernels there
    big = H.model((24, 24, 24), F64, DEV, **H.INTERACTING)
    start = _field((2, 24, 24, 24), F64, 701)
    torch.manual_seed(9)
    y_none = big.hmc.start(start).sample(4, n_chains=2, n_md=3, dt=0.05)
    torch.manual_seed(9)
    assert torch.equal(y_none, big.hmc.start(start).sample(4, n_chains=2, n_md=3, dt=0.05, path='tiled'))


def test_free_field_distribution_tiled_fp32():
    torch.manual_seed(21)
    m = H.model((16,), F32, DEV, **H.FREE)
    y = m.hmc.sample(256 * 160, n_chains=256, n_md=3, dt=0.4, path='tiled')
    mean, err = H.chain_stats(y, 256, drop=30)
    rate = m.hmc.history.accept_rate[-1]
    print(f"free field, tiled fp32: <phi^2> {mean:.5f} +- {err:.5f} ({(mean - H.FREE_PHI2) / err:+.2f} sigma), accept rate {rate:.3f}")
    assert abs(mean - H.FREE_PHI2) <= 5 * err
    assert 0.7 < rate < 0.97


def test_interacting_chain_against_quadrature_tiled_fp32():
    exact = H.quadrature_phi2()
    torch.manual_seed(22)
    m = H.model((4,), F32, DEV, **H.INTERACTING)
    y = m.hmc.sample(256 * 260, n_chains=256, n_md=4, dt=0.25, path='tiled')
    mean, err = H.chain_stats(y, 256, drop=30)
    e = torch.exp(-m.hmc.last['dh'][30:]).flatten().cpu()
    e_mean, e_err = e.mean().item(), e.std().item() / e.numel() ** 0.5
    print(f"(4,) chain, tiled fp32: <phi^2> {mean:.5f} +- {err:.5f} ({(mean - exact) / err:+.2f} sigma of {exact:.6f}), "
          f"<exp(-dH)> - 1 = {e_mean - 1:+.2e} +- {e_err:.2e}, accept rate {m.hmc.history.accept_rate[-1]:.3f}")
    assert abs(mean - exact) <= 5 * err
    assert abs(e_mean - 1.0) <= 5 * e_err


def test_graph_capture():
    """The call neither allocates nor synchronises: captured and replayed once it equals the eager call, bitwise."""
    lattice, C = (12, 12, 12, 12), 3
    m = H.model(lattice, F32, DEV, **H.INTERACTING)
    coef = m.hmc._coef(lattice)
    phi0 = _field((C,) + lattice, F32, 900)
    pos = (31, 64)
    phi_e, e = _launch(phi0, coef, 6, pos, record_every=3)
    static = phi0.clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        r = _hip.phi4_hmc_tiled(static, *coef, 4, 0.1, n_traj=6, record_every=3, position=pos)
    torch.cuda.synchronize()
    assert torch.equal(static, phi0)                                     # capture ran nothing
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(static, phi_e) and torch.equal(r['record'], e['record'])
    assert torch.equal(r['dh'], e['dh']) and torch.equal(r['accept'], e['accept']) and torch.equal(r['action'], e['action'])

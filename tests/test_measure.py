"""nf_lattice_measure and `measure` / `Model.measure` / `Ensemble` on the device.

The kernel is held to the numpy reference of tests/measure_cases.py, evaluated on the up-cast input, within the worst-case
bound of a double sum, (terms + 4) 2^-53 sum |terms| per quantity and row; the cases and the regimes they reach are
tests/measure_cases.py's (checked on the host by tests/test_measure_host.py).  Its bits depend on a row's values and the
plan alone: the same row gives the same bits whatever the batch, its position in it, or the pointer's alignment (the wide
and the narrow loads fill the same LDS image, and every sum is read from the image)."""
import functools

import numpy as np
import pytest
import torch

from normflow__amd import _hip
from normflow__amd.lib import observables as OB

import hmc_cases as H
import measure_cases as MC

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F32, F64 = torch.float32, torch.float64
_name = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v).replace("torch.", "")
ALL = [(lat, N, dt) for dt in (F32, F64) for lat, N in MC.cases(dt)]
_id = lambda c: f"{MC.case_id(c[:2])}-{_name(c[2])}"
# one case per regime of the plan, and the lattices with axes of extent 1
SOME = [((5,), 5), ((1, 7), 5), ((16, 16), 67), ((5, 7, 9), 5), ((1, 3, 4, 5), 5), ((16, 16, 16), 5), ((53, 101), 2),
        ((12, 12, 12, 12), 3), ((3, 50, 70), 2)]
BITWISE = [((16, 16), 67), ((5, 7, 9), 67), ((16, 16, 16), 67), ((12, 12, 12, 12), 3), ((130, 130), 3), ((20012,), 3)]


@functools.lru_cache(maxsize=None)
def _case(lattice, N, dtype):
    """(rows on the CPU, the reference of the up-cast rows): computed once, shared, never written."""
    x = MC.draw(lattice, N, dtype)
    return x, MC.ref_measure(x.numpy())


def _check(got, ref, name, report=None):
    res = MC.worst(got, ref)
    if report is not None:
        q = max(res, key=lambda k: res[k][0] / max(res[k][1], 1e-300))
        report(name, q, *res[q])
    for q, (err, bound) in res.items():
        assert err <= bound, (name, q, err, bound)


@pytest.mark.parametrize("case", ALL, ids=_id)
def test_kernel_against_the_reference(case, parity_report):
    lattice, N, dtype = case
    x0, ref = _case(lattice, N, dtype)
    x = x0.to(DEV)
    out = _hip.lattice_measure(x)
    assert out.dtype == F64 and torch.equal(x.cpu(), x0)                     # the input is unchanged
    _check(MC.unpack(out, lattice), ref, f"measure {_name(dtype)} {_name(lattice)} N={N}", parity_report)
    # `measure` hands out the same numbers, and every axis' slices add up to sum phi within the two bounds
    m = OB.measure(x)
    assert OB.kernel_applies(x) and torch.equal(m.sum_phi, out[:, 0]) and torch.equal(m.sum_phi4, out[:, 2])
    got = MC.fields(m)
    assert np.array_equal(got['links'], MC.unpack(out, lattice)['links'])
    for mu, L in enumerate(lattice):
        assert np.array_equal(got[f'slices_{mu}'], MC.unpack(out, lattice)[f'slices_{mu}'])
        sb = ref[f'slices_{mu}'][1].sum(axis=1) + (L + 4) * MC.U * np.abs(ref[f'slices_{mu}'][0]).sum(axis=1)
        assert (np.abs(got[f'slices_{mu}'].sum(axis=1) - got['sum_phi']) <= sb + ref['sum_phi'][1]).all()


@pytest.mark.parametrize("dtype", [F32, F64], ids=_name)
@pytest.mark.parametrize("case", BITWISE, ids=MC.case_id)
def test_a_row_depends_on_nothing_but_itself(case, dtype):
    lattice, N = case
    x = MC.draw(lattice, N, dtype, seed=7).to(DEV)
    full = _hip.lattice_measure(x)
    assert torch.equal(_hip.lattice_measure(x), full)                            # the same input, the same bits
    g = torch.Generator(device='cpu').manual_seed(3)
    perm = torch.randperm(N, generator=g, device='cpu').to(DEV)
    assert torch.equal(_hip.lattice_measure(x[perm].contiguous()), full[perm])   # a permutation of the rows permutes the output
    for k in {0, N // 2, N - 1}:
        assert torch.equal(_hip.lattice_measure(x[k:k + 1]), full[k:k + 1])      # a row alone
    assert torch.equal(_hip.lattice_measure(x[::2].contiguous()), full[::2])     # every other row


@pytest.mark.parametrize("dtype", [F32, F64], ids=_name)
@pytest.mark.parametrize("case", [((16, 16), 5), ((16, 16, 16), 3), ((12, 12, 12, 12), 2), ((17, 16), 5),
                                  ((20012,), 2), ((12290,), 2)], ids=MC.case_id)
def test_a_misaligned_tensor_gives_the_aligned_copys_bits(case, dtype):
    """One element off a 16-byte boundary the rows are loaded site by site instead of 16 bytes at a time -- into the same
    LDS image, which every sum is read from: the bits are equal, not merely within the bound."""
    lattice, N = case
    x = MC.draw(lattice, N, dtype, seed=11).to(DEV)
    buf = torch.empty(x.numel() + 1, dtype=dtype, device=DEV)
    off = buf[1:].view(x.shape)
    off.copy_(x)
    assert x.data_ptr() % 16 == 0 and off.data_ptr() % 16 != 0 and off.is_contiguous()
    assert torch.equal(_hip.lattice_measure(off), _hip.lattice_measure(x))


@pytest.mark.parametrize("dtype", [F32, F64], ids=_name)
def test_a_view_that_is_not_contiguous(dtype):
    x = MC.draw((9, 16, 12), 5, dtype, seed=13).to(DEV)
    view = x.transpose(1, 3)                                                     # (5, 12, 16, 9)
    keep = x.clone()
    m = OB.measure(view)
    assert not view.is_contiguous() and torch.equal(x, keep) and m.lattice == (12, 16, 9)
    assert torch.equal(m.links, OB.measure(view.contiguous()).links)
    _check(MC.fields(m), MC.ref_measure(view.cpu().numpy()), "transposed view")
    # the statistics of the transposed lattice are those of the lattice with the axes exchanged
    m0 = OB.measure(x)
    assert torch.allclose(m.slices[0], m0.slices[2], rtol=1e-12, atol=1e-12)
    assert torch.allclose(m.links[:, 2], m0.links[:, 0], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("case", [((16, 16, 16), 5, F32), ((16, 16), 67, F64), ((12, 12, 12, 12), 3, F32),
                                  ((24, 24, 24), 2, F64)], ids=_id)
def test_graph_capture(case):
    """The call neither allocates nor synchronises: captured and replayed once it equals the eager call, bitwise."""
    lattice, N, dtype = case
    x = MC.draw(lattice, N, dtype, seed=17).to(DEV)
    eager = _hip.lattice_measure(x)
    static = torch.zeros_like(x)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = _hip.lattice_measure(static)
    torch.cuda.synchronize()
    static.copy_(x)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


@pytest.mark.parametrize("dtype", [F32, F64], ids=_name)
@pytest.mark.parametrize("case", SOME, ids=MC.case_id)
def test_kernel_and_composed_path_agree(case, dtype):
    lattice, N = case
    x0, ref = _case(lattice, N, dtype)
    x = x0.to(DEV)
    k, c = MC.fields(OB.measure(x, path='kernel')), MC.fields(OB.measure(x, path='composed'))
    for name, (_, bound) in ref.items():                                         # each is within the bound of the exact value
        assert (np.abs(k[name] - c[name]) <= 2 * bound).all(), name


@pytest.mark.parametrize("dtype", [F32, F64], ids=_name)
@pytest.mark.parametrize("lattice", MC.SMALL + [(12, 12, 12, 12)], ids=_name)
def test_action_of_a_measurement(lattice, dtype):
    """Measurement.action against the nf_phi4_action kernel: 1e-12 in fp64; in fp32 the action kernel's own tolerance
    against the reference's values (2e-6 of the largest action, tests/test_gpu_parity.py)."""
    model = H.model(lattice, dtype, DEV, **H.INTERACTING)
    y = MC.draw(lattice, 5, dtype, seed=19).to(DEV)
    m = model.measure(y)
    want = model.action(y).double()
    tol = 1e-12 if dtype == F64 else 2e-6
    assert m.action.dtype == F64 and ((m.action - want).abs().max() <= tol * want.abs().max()).item(), (m.action, want)


def test_free_field_hmc_end_to_end():
    """model.hmc rows -> Model.measure -> Ensemble on the free 16^2 lattice, with the run of the free-field <phi^2> test
    of tests/test_hmc.py (256 chains, n_md = 3, dt = 0.4, 160 steps, the first 30 dropped): the time-slice correlator at
    t = 0 .. 8 and <phi^2> within 5 sigma of the exact values, errors from the chain jackknife.  The composed path on CPU
    tensors passes the same statement from the same seed (largest deviation 1.1 sigma; here 0.9 sigma was measured)."""
    torch.manual_seed(21)
    m = H.model((16, 16), F32, DEV, **H.FREE)
    y = m.hmc.sample(256 * 160, n_chains=256, n_md=3, dt=0.4)
    e = OB.Ensemble(m.measure(y), n_chains=256, drop=30)
    G, _, phi2 = MC.free_exact(16)
    val, err = e.correlator(0)
    dev = MC.sigmas(val[:9], err[:9], G[:9])
    p2, p2e = e.mean('phi2')
    tau, tau_err, W = e.tau_int('magnetization')
    print(f"free 16^2 HMC: G(t) deviations {np.round(dev, 2).tolist()} sigma; <phi^2> {p2:.5f} +- {p2e:.5f} "
          f"({(p2 - phi2) / p2e:+.2f} sigma of {phi2:.5f}); accept rate {m.hmc.history.accept_rate[-1]:.3f}; "
          f"tau_int(m) {tau:.2f} +- {tau_err:.2f} (W = {W})")
    assert (dev <= 5).all(), dev
    assert abs(p2 - phi2) <= 5 * p2e

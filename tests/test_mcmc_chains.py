"""MCMCSampler(n_chains=) on an MI355X: nf_metropolis_chains against a restatement of its documented random stream
(include/normflow_hip.h) and a numpy scan in double, nf_metropolis_select against torch.index_select, the sampler end to
end against replayed proposals, the stationary distribution of a free field, and the absence of host traffic."""
import math

import numpy as np
import pytest
import torch

import normflow__amd as nf
from normflow__amd import _hip
from normflow__amd.mask import EvenOddMask
from normflow__amd.nn import AffineCoupling_, ConvAct, ModuleList_
from normflow__amd.prior import NormalPrior
from normflow__amd.action import ScalarPhi4Action
from oracle import nf_oracle as O

from mcmc_cases import position as _position, log_uniforms as _log_uniforms, scan as _scan, run_chains as _run_chains

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
CHAIN_DOMAIN = 0x6E666368          # NF_PHILOX_CHAIN_DOMAIN
NP_DTYPE = {torch.float32: np.float32, torch.float64: np.float64}


@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


@pytest.mark.parametrize("fresh", [False, True])
@pytest.mark.parametrize("S,C", [(1, 300), (1000, 1), (37, 7), (16, 256)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_metropolis_chains_teacher_forced(dtype, S, C, fresh):
    # inputs from numpy's generator and the Philox position from torch.manual_seed: the case is the same on every machine,
    # and on this seed no decision of any case is within 1e-9 of a tie (asserted below)
    seed = 1000 + 7 * S + C
    rng = np.random.default_rng(seed)
    npdt = NP_DTYPE[dtype]
    B = S * C
    logq, logp = (rng.normal(size=B) * 2).astype(npdt), (rng.normal(size=B) * 2).astype(npdt)
    ref_lq, ref_lp = (rng.normal(size=C) * 2).astype(npdt), (rng.normal(size=C) * 2).astype(npdt)
    ref = ref_lq.astype(np.float64) - ref_lp.astype(np.float64)
    torch.manual_seed(seed)
    got, (pseed, off) = _run_chains(logq, logp, ref, ref_lq, ref_lp, C, fresh, dtype)
    logu = _log_uniforms(pseed, off, B)
    want = _scan(logq, logp, ref, ref_lq, ref_lp, logu, S, C, fresh)
    print(f"chains {dtype} S={S} C={C} fresh={fresh}: smallest |margin| {want[-1]:.3e}, accept {want[0].mean():.3f}")
    assert want[-1] > 1e-9                                        # every flag below is decided
    assert set(np.unique(got[0])) <= {0, 1}
    if B > C or not fresh:
        assert want[0].any() and not want[0].all()
    np.testing.assert_array_equal(got[0].astype(bool), want[0])
    np.testing.assert_array_equal(got[1], want[1])
    r = np.arange(B)
    assert (got[1] <= r).all() and (got[1] % C == r % C).all()
    for g, w in zip(got[2:], want[2:7]):                           # selected values and the final state: exact, bitwise
        assert g.dtype == w.dtype and np.array_equal(g.view(np.uint8), w.view(np.uint8))

    if fresh:
        return
    # logqp_ref = -inf: nothing is ever accepted; +inf: every chain accepts its first proposal, then the rule goes on
    for val in (-math.inf, math.inf):
        inf_ref = np.full(C, val)
        got, (pseed, off) = _run_chains(logq, logp, inf_ref, ref_lq, ref_lp, C, False, dtype)
        want = _scan(logq, logp, inf_ref, ref_lq, ref_lp, _log_uniforms(pseed, off, B), S, C, False)
        assert want[-1] > 1e-9
        np.testing.assert_array_equal(got[0].astype(bool), want[0])
        np.testing.assert_array_equal(got[1], want[1])
        if val < 0:
            assert not got[0].any() and (got[1] == r % C).all() and np.array_equal(got[4], inf_ref)
            assert np.array_equal(got[2], np.tile(ref_lq, S)) and np.array_equal(got[3], np.tile(ref_lp, S))
        else:
            assert got[0][:C].all() and (S > 1 or got[0].all())


def _select_case(S, C, rng):
    """Flags and keep of C chains over S steps: chain 0 never accepts, chain 1 rejects its first steps, chain 2 accepts
    its first; the rest at random."""
    flags = rng.random((S, C)) < 0.6
    flags[:, 0] = False
    if C > 2 and S > 2:
        flags[:2, 1], flags[2, 1] = False, True
        flags[0, 2] = True
    keep = np.empty((S, C), dtype=np.int64)
    last = np.arange(C)
    for s in range(S):
        last = np.where(flags[s], s * C + np.arange(C), last)
        keep[s] = last
    return flags.ravel(), keep.ravel()


@pytest.mark.parametrize("V", [30, 4096])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32, torch.float64])
def test_metropolis_select_is_index_select(dtype, V):
    rng = np.random.default_rng(5)
    for S, C in ((9, 7), (3, 1), (1, 70)):
        B = S * C
        flags, keep = _select_case(S, C, rng)
        assert not flags.all() and (S * C < 10 or flags.any())
        torch.manual_seed(S + C)
        shape = (5, 6) if V == 30 else (V,)
        y = torch.randn((B, *shape), device=DEV).to(dtype)
        ref = torch.randn((C, *shape), device=DEV).to(dtype)
        y0 = y.clone()
        # the equivalent gather on cat([ref_sample, y]): the kept row if it was accepted, else the chain's stored sample
        idx = np.where(flags[keep], keep + C, np.arange(B) % C)
        want = torch.index_select(torch.cat([ref, y0]), 0, torch.as_tensor(idx, device=DEV))
        _hip.metropolis_select(y, ref, torch.as_tensor(flags.astype(np.uint8), device=DEV),
                               torch.as_tensor(keep, device=DEV), C)
        torch.cuda.synchronize()
        assert torch.equal(y.view(torch.uint8), want.view(torch.uint8))            # bitwise
        acc = torch.as_tensor(flags, device=DEV)
        assert torch.equal(y[acc].view(torch.uint8), y0[acc].view(torch.uint8))    # accepted rows untouched
        assert not torch.equal(y, y0)

    # fresh chains: every first row accepted, no stored sample to read
    S, C = 6, 5
    flags, keep = _select_case(S, C, rng)
    flags[:C] = True
    flags, keep = flags.reshape(S, C), keep.reshape(S, C)
    last = np.arange(C)
    for s in range(S):
        last = np.where(flags[s], s * C + np.arange(C), last)
        keep[s] = last
    flags, keep = flags.ravel(), keep.ravel()
    y = torch.randn((S * C, V), device=DEV).to(dtype)
    want = torch.index_select(y, 0, torch.as_tensor(keep, device=DEV))
    _hip.metropolis_select(y, None, torch.as_tensor(flags.astype(np.uint8), device=DEV), torch.as_tensor(keep, device=DEV), C)
    torch.cuda.synchronize()
    assert torch.equal(y.view(torch.uint8), want.view(torch.uint8))


def _affine_model(shape, dtype, seed=0, kappa=0.5, m_sq=-1.0, lambd=0.5):
    torch.manual_seed(seed)
    mask = EvenOddMask(shape=shape)
    nets = [ConvAct(1, 2, 3, conv_dim=len(shape), hidden_sizes=[4], acts=['tanh', None]) for _ in range(2)]
    with torch.no_grad():
        for net in nets:
            for p in net.parameters():
                p.mul_(0.5)
    net_ = ModuleList_([AffineCoupling_(nets, mask=mask)])
    net_.to(device=DEV, dtype=dtype)
    prior = NormalPrior(loc=torch.zeros(shape, dtype=dtype, device=DEV), scale=torch.ones(shape, dtype=dtype, device=DEV))
    return nf.Model(net_=net_, prior=prior, action=ScalarPhi4Action(kappa=kappa, m_sq=m_sq, lambd=lambd))


def _two_calls(shape, dtype, C, B, graphed=False):
    model = _affine_model(shape, dtype, seed=1)
    model.posterior.graphed = graphed
    s = model.mcmc
    out = []
    for seed in (5, 6):
        torch.manual_seed(seed)
        y, lq, lp = s.sample__(batch_size=B, bookkeeping=True, n_chains=C)
        out.append((y.clone(), lq.clone(), lp.clone(), s.history.accept_seq[-1], s.history.accept_ind[-1],
                    {k: v.clone() for k, v in s._ref.items()}))
    return model, out


@pytest.mark.parametrize("C", [1, 32])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_sampler_end_to_end_against_replayed_proposals(dtype, C):
    shape, B = (8, 16), 4 * 32
    S = B // C
    model, first = _two_calls(shape, dtype, C, B)
    _, again = _two_calls(shape, dtype, C, B)
    _, graphed = _two_calls(shape, dtype, C, B, graphed=True)
    for other in (again, graphed):                                 # same seeds, same output; a HIP-graph flow changes nothing
        for a, b in zip(first, other):
            for u, v in zip(a[:3], b[:3]):
                assert torch.equal(u, v)
            np.testing.assert_array_equal(a[3], b[3])
            np.testing.assert_array_equal(a[4], b[4])

    stored, decided, total = None, 0, 0
    for (y, lq, lp, acc, ind, ref), seed in zip(first, (5, 6)):
        acc, ind = acc.ravel(), ind.ravel()
        assert acc.shape == (B,) and acc.dtype == bool and ind.dtype == np.int64
        torch.manual_seed(seed)
        py, plq, plp = model.posterior.sample__(B)                 # the proposals of that call, replayed
        pseed, off = _position()                                   # where the sampler's launch drew its uniforms
        # the decisions, restated from the replayed log q / log p and the state the previous call left
        npdt = NP_DTYPE[dtype]
        if stored is None:
            z = np.zeros(C)
            want = _scan(plq.cpu().numpy(), plp.cpu().numpy(), z, z.astype(npdt), z.astype(npdt),
                         _log_uniforms(pseed, off, B), S, C, True)
        else:
            want = _scan(plq.cpu().numpy(), plp.cpu().numpy(), stored['logqp'].reshape(C).cpu().numpy(),
                         stored['logq'].reshape(C).cpu().numpy(), stored['logp'].reshape(C).cpu().numpy(),
                         _log_uniforms(pseed, off, B), S, C, False)
        assert want[-1] > 1e-9
        np.testing.assert_array_equal(acc, want[0])
        np.testing.assert_array_equal(ind, want[1])
        r = np.arange(B)
        assert (ind <= r).all() and (ind % C == r % C).all()
        # every returned row: bitwise the proposal row it points at, or the chain's stored sample
        from_prop = torch.as_tensor(acc[ind], device=DEV)
        ind_t = torch.as_tensor(ind, device=DEV)
        if stored is None:
            assert bool(from_prop.all())
            want_y, want_q, want_p = py[ind_t], plq[ind_t], plp[ind_t]
        else:
            chain = torch.as_tensor(r % C, device=DEV)
            pick = lambda prop, st: torch.where(from_prop.reshape(-1, *[1] * (prop.dim() - 1)), prop[ind_t],
                                                st.reshape(C, *prop.shape[1:])[chain])
            want_y, want_q, want_p = pick(py, stored['sample']), pick(plq, stored['logq']), pick(plp, stored['logp'])
            total += int((~from_prop).sum())
        assert torch.equal(y, want_y) and torch.equal(lq, want_q) and torch.equal(lp, want_p)
        # the stored state: a copy of the last C rows, in the reference's shapes for one chain
        assert torch.equal(ref['sample'].reshape(C, *shape), y[-C:]) and torch.equal(ref['logq'].reshape(C), lq[-C:])
        assert torch.equal(ref['logp'].reshape(C), lp[-C:])
        assert ref['logqp'].dtype == torch.float64
        assert torch.equal(ref['logqp'].reshape(C), lq[-C:].double() - lp[-C:].double())
        assert ref['sample'].shape == (shape if C == 1 else (C, *shape)) and ref['logqp'].shape == (() if C == 1 else (C,))
        decided += int(acc.sum())
        stored = ref
    assert 0 < decided < 2 * B
    if C > 1:
        assert total > 0                                           # some chain held its stored sample into the second call


def test_default_path_continues_a_device_chain_and_back():
    """n_chains=None after a device call with n_chains=1 continues that chain (and the other way round)."""
    shape = (8, 16)
    model = _affine_model(shape, torch.float64, seed=2)
    s = model.mcmc
    torch.manual_seed(3)
    np.random.seed(3)
    s.sample__(batch_size=16, n_chains=1)
    left = {k: v.clone() for k, v in s._ref.items()}
    s.sample__(batch_size=16, bookkeeping=True)                    # the reference's host code
    acc, lq, lp = s.history.accept_seq[-1], s.history.raw_logq[-1], s.history.raw_logp[-1]
    np.random.seed(3)
    d = lq - lp
    logu = np.log(np.random.rand(16))
    ref, want = left['logqp'].item(), []
    for i in range(16):
        want.append(logu[i] < ref - d[i])
        ref = d[i] if want[-1] else ref
    np.testing.assert_array_equal(acc, want)
    assert isinstance(s._ref['logqp'], float)
    y = s.sample(batch_size=8, n_chains=1)                         # and the device path takes the floats back
    assert y.shape == (8, *shape) and torch.is_tensor(s._ref['logqp']) and s._ref['logqp'].is_cuda


def test_free_field_distribution():
    """<phi^2> of a free field on 16 sites from 256 independent chains matches trace(K^-1) / V within 5 standard errors
    (across chains), after a burn-in chosen from the run's own acceptance rate.

    The field's parameters: an independence sampler converges geometrically, at a rate its acceptance rate describes,
    only if p / q is bounded, i.e. if the proposal covers the target's tails.  The proposal is a mild flow of the unit
    normal, so the target is chosen with every mode narrower than that: K has the eigenvalues m^2 + 2 kappa (1 - cos k),
    with kappa = 0.25 and m^2 = 1.5 mode variances from 0.4 to 0.67 (tr K^-1 / V = 0.516, against about 1 for the
    proposals themselves: a sampler that accepted everything would miss by hundreds of standard errors).  With the blocked
    test's kappa = 1, m^2 = 0.5 the zero mode has variance 2, wider than the proposal's: unbounded weights, and a chain of
    a few hundred steps is visibly biased whatever the burn-in."""
    L, C, S = 16, 256, 400
    model = _affine_model((L,), torch.float32, seed=3, kappa=0.25, m_sq=1.5, lambd=0.0)
    w0, w2, _ = model.action.get_coef(1)
    T = np.roll(np.eye(L), 1, axis=0)
    K = 2 * w2 * np.eye(L) - w0 * (T + T.T)            # S = phi^T K phi / 2
    exact = np.trace(np.linalg.inv(K)) / L
    torch.manual_seed(17)
    y = model.mcmc.sample(batch_size=S * C, n_chains=C)
    rate = model.mcmc.history.accept_rate[-1]
    assert 0.05 < rate < 0.99
    burn = int(math.ceil(math.log(1e-3) / math.log(1.0 - rate))) + 1
    assert (1.0 - rate) ** burn < 1e-3 and burn < S // 2
    phi2 = (y.double() ** 2).mean(dim=1).reshape(S, C)[burn:].cpu().numpy()
    per_chain = phi2.mean(axis=0)
    mean, se = per_chain.mean(), per_chain.std(ddof=1) / math.sqrt(C)
    print(f"free field: <phi^2> {mean:.5f} exact {exact:.5f} se {se:.5f} rate {rate:.3f} burn-in {burn}")
    assert abs(mean - exact) < 5 * se, (mean, exact, se, rate)


def test_one_chain_device_call_moves_nothing_but_the_flags():
    """With `_ref` holding device tensors, the device step of an n_chains=1 call (both launches, the `_ref` update) runs
    with torch's synchronisation debug mode set to "error": no host-to-device copy, no device-to-host read, no
    synchronisation.  The flags are read afterwards, once, by `sample__`."""
    shape, B = (8, 16), 64
    model = _affine_model(shape, torch.float32, seed=4)
    s = model.mcmc
    torch.manual_seed(8)
    s.sample__(batch_size=B, n_chains=1)
    assert all(torch.is_tensor(v) and v.is_cuda for v in s._ref.values())
    assert s._ref['sample'].shape == shape and s._ref['logqp'].shape == () and s._ref['logqp'].dtype == torch.float64
    y, lq, lp = model.posterior.sample__(B)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        assert s._stored_chains(1)
        y2, lq2, lp2, flags, keep = s._chains_device(y, lq, lp, 1, True)
        assert all(torch.is_tensor(v) and v.is_cuda for v in s._ref.values())
        with pytest.raises(RuntimeError):
            flags.cpu()                                            # the mode is live: the one read would be caught here
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    acc = flags.cpu().numpy()
    assert set(np.unique(acc)) <= {0, 1} and y2.shape == (B, *shape)
    s.sample__(batch_size=B, bookkeeping=True, n_chains=1)         # and the whole call goes through
    assert len(s.history.accept_rate) == 2 and s.history.accept_ind[-1].shape == (B,)

#!/usr/bin/env python3
"""Generate tests/golden/mcmc.npz by RUNNING THE REFERENCE's independence Metropolis sampler.

Container-only, like make_golden_blocked.py (same invocation, with this file's name).

The file holds data only: the net's weights and the reference's outputs.  Case: that of make_golden_blocked.py (CPU, fp64,
the unit normal prior on a 1-D lattice of 8 sites, one AffineCoupling_ block with weights x 0.5, phi^4).  After
torch.manual_seed / np.random.seed, three calls of model.mcmc.sample__(batch_size=8, bookkeeping=True): the second and
third continue the chain.  The seed is chosen so that the fixture holds both decisions, a continued call whose first
proposal is accepted and one whose first proposal is rejected (asserted below).  tests/test_mcmc_chains_host.py replays it.
"""
import os
import warnings

import numpy as np

warnings.filterwarnings("ignore")
if not hasattr(np, "product"):
    np.product = np.prod          # NumPy-1 alias the reference's Prior.nvar relies on (as in make_golden_psd.py)
HERE = os.path.dirname(os.path.abspath(__file__))

import torch  # noqa: E402
import normflow  # noqa: E402  (the REFERENCE; sets default dtype fp64)
from normflow.mask import EvenOddMask  # noqa: E402
from normflow.nn import AffineCoupling_, ConvAct, ModuleList_  # noqa: E402
from normflow.action import ScalarPhi4Action  # noqa: E402
from normflow.prior import NormalPrior  # noqa: E402
from normflow import Model  # noqa: E402

torch.set_default_device('cpu')
assert torch.get_default_dtype() == torch.float64

L, SEED, KAPPA, M_SQ, LAMBD, BATCH, CALLS = 8, 6, 0.5, -0.5, 0.8, 8, 3


def main():
    torch.manual_seed(11)
    nets = [ConvAct(1, 2, 3, conv_dim=1, hidden_sizes=[4], acts=['tanh', None]) for _ in range(2)]
    with torch.no_grad():       # a mild flow: acceptances and rejections both occur
        for net in nets:
            for p in net.parameters():
                p.mul_(0.5)
    net_ = ModuleList_([AffineCoupling_(nets, mask=EvenOddMask(shape=(L,)))])
    prior = NormalPrior(loc=torch.zeros(L), scale=torch.ones(L))
    action = ScalarPhi4Action(kappa=KAPPA, m_sq=M_SQ, lambd=LAMBD)
    model = Model(net_=net_, prior=prior, action=action)

    out = dict(L=np.int64(L), seed=np.int64(SEED), kappa=np.float64(KAPPA), m_sq=np.float64(M_SQ),
               lambd=np.float64(LAMBD))
    for k, net in enumerate(nets):
        for j, conv in enumerate(m for m in net if hasattr(m, 'weight')):
            out[f"w{k}{j}"] = conv.weight.detach().numpy()
            out[f"b{k}{j}"] = conv.bias.detach().numpy()

    torch.manual_seed(SEED)
    np.random.seed(SEED)
    for call in range(CALLS):
        cfgs, logq, logp = model.mcmc.sample__(batch_size=BATCH, bookkeeping=True)
        out[f"cfgs{call}"] = cfgs.numpy()
        out[f"logq{call}"] = logq.numpy()
        out[f"logp{call}"] = logp.numpy()
        out[f"accept_seq{call}"] = np.asarray(model.mcmc.history.accept_seq[-1], dtype=bool)
        out[f"accept_ind{call}"] = np.asarray(model.mcmc.history.accept_ind[-1], dtype=np.int64)
    out["accept_rate"] = np.array(model.mcmc.history.accept_rate)

    seqs = [out[f"accept_seq{call}"] for call in range(CALLS)]
    flat = np.concatenate(seqs)
    assert flat.any() and not flat.all(), "the fixture needs both decisions"
    firsts = [bool(s[0]) for s in seqs[1:]]
    assert any(firsts), "the fixture needs a continued call whose first proposal is accepted"
    assert not all(firsts), "the fixture needs a continued call whose first proposal is rejected"

    path = os.path.join(HERE, "mcmc.npz")
    np.savez_compressed(path, **out)
    print(f"mcmc: {os.path.getsize(path) / 1024:.1f} KiB, flags " +
          " / ".join("".join(str(int(v)) for v in s) for s in seqs))


if __name__ == "__main__":
    main()

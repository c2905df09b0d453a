#!/usr/bin/env python3
"""Generate tests/golden/blocked.npz by RUNNING THE REFERENCE's blocked Metropolis sampler.

Container-only, like make_golden.py (same invocation, with this file's name):

    mkdir -p /tmp/nf_oracle && ln -sfn /root/reference/src /tmp/nf_oracle/normflow
    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=/tmp/nf_oracle python3 tests/golden/make_golden_blocked.py

The file holds data only: the net's weights and the reference's outputs.  Case: CPU, fp64, the unit normal prior on a 1-D
lattice of 8 sites, one AffineCoupling_ block (two ConvAct nets 1 -> 4 -> 2, kernel 3, tanh), phi^4 with lambda > 0.
After torch.manual_seed / np.random.seed, two calls of model.blocked_mcmc.sample__(batch_size=6, n_blocks=4,
bookkeeping=True): the second continues the first's chain.  tests/test_blocked_mcmc_host.py replays it.
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

L, SEED, KAPPA, M_SQ, LAMBD = 8, 1234, 0.5, -0.5, 0.8


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
    for call in range(2):
        cfgs, logq, logp = model.blocked_mcmc.sample__(batch_size=6, n_blocks=4, bookkeeping=True)
        out[f"cfgs{call}"] = cfgs.numpy()
        out[f"logq{call}"] = logq.numpy()
        out[f"logp{call}"] = logp.numpy()
        out[f"accept_seq{call}"] = model.blocked_mcmc.history.accept_seq[-1]
    out["accept_rate"] = np.array(model.blocked_mcmc.history.accept_rate)
    path = os.path.join(HERE, "blocked.npz")
    np.savez_compressed(path, **out)
    print(f"blocked: {os.path.getsize(path) / 1024:.1f} KiB, accept {out['accept_seq0'].mean():.2f} "
          f"{out['accept_seq1'].mean():.2f}")


if __name__ == "__main__":
    main()

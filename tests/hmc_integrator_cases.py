"""Shared by tests/test_hmc_integrators_host.py and tests/test_hmc_integrators.py: the integration schemes typed again
from their definition (include/normflow_hip.h, "integration schemes"), and the fp64 torch restatement of a trajectory of
a scheme, written from that definition with torch.roll (the force and the action of tests/hmc_cases.py) and none of the
package's code."""
import torch

import hmc_cases as H

LAMBDA = 0.1931833275037836
R1, R2, R3, R4 = 0.08398315262876693, 0.2539785108410595, 0.6822365335719091, -0.03230286765269967
W1 = 1.0 / (2.0 - 2.0 ** (1.0 / 3.0))
W0 = 1.0 - 2.0 * W1
SCHEMES = {
    'leapfrog': ((1.0,), (1.0,)),
    'omelyan': ((0.5, 0.5), (1.0 - 2.0 * LAMBDA, 2.0 * LAMBDA)),
    'omf4': ((R2, R4, 1.0 - 2.0 * (R2 + R4), R4, R2), (R3, 0.5 - R1 - R3, 0.5 - R1 - R3, R3, 2.0 * R1)),
}
YOSHIDA = ((W1, W0, W1), ((W1 + W0) / 2, (W1 + W0) / 2, W1))      # a custom scheme: Yoshida's fourth-order triple
# what the tests hand to `integrator=` / `scheme=`, and the weights of each
INTEGRATORS = {'leapfrog': 'leapfrog', 'omelyan': 'omelyan', 'omf4': 'omf4', 'yoshida': YOSHIDA}
WEIGHTS = dict(SCHEMES, yoshida=YOSHIDA)
ORDER = {'leapfrog': 2, 'omelyan': 2, 'omf4': 4, 'yoshida': 4}


def ref_trajectory(phi, pi, action, n_md, dt, weights):
    """(phi1, pi1, dH) of one trajectory of the scheme `weights` = (a, b) in fp64 on the CPU."""
    a, b = weights
    s = len(a)
    phi, pi = phi.detach().double().cpu(), pi.detach().double().cpu()
    H0 = 0.5 * (pi ** 2).flatten(1).sum(1) + H.ref_action(phi, action)
    pi = pi - (0.5 * b[s - 1] * dt) * H.ref_force(phi, action)
    for k in range(1, n_md + 1):
        for j in range(s):
            phi = phi + (a[j] * dt) * pi
            last = k == n_md and j == s - 1
            pi = pi - ((0.5 * b[j] if last else b[j]) * dt) * H.ref_force(phi, action)
    H1 = 0.5 * (pi ** 2).flatten(1).sum(1) + H.ref_action(phi, action)
    return phi, pi, H1 - H0


def starts(shape, seed, scale=0.7):
    """(phi0, pi0) fp64 on the CPU: phi0 = scale randn, pi0 = randn."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    phi = scale * torch.randn(shape, generator=g, dtype=torch.float64, device="cpu")
    return phi, torch.randn(shape, generator=g, dtype=torch.float64, device="cpu")

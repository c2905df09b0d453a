"""Shared by tests/test_hmc_fa_host.py and tests/test_hmc_fa.py: the lattices of the Fourier-accelerated HMC suites and the
numpy restatement of one accelerated trajectory, written from include/normflow_hip.h ("Fourier-accelerated hybrid Monte
Carlo") with an explicit dense Hartley matrix per axis -- no FFT and none of the package's code.

Each shape is the smallest one that reaches a particular piece of code:
    (4, 4)         16 sites, one partial tile
    (5, 6)         odd and unequal extents, two matrices
    (2, 3, 4, 4)   four axes, extent 2 where the neighbour counts twice, a shared matrix
    (1, 8, 8)      as a user lattice with an axis of extent 1
    (24, 8)        two output tiles
    (48, 4)        three output tiles
    (64, 4)        four output tiles
    (64,)          one axis
    (16, 16)       a BASELINE shape
    (16, 16, 16)   several sites per lane; the only case above a few thousand sites"""
import math

import numpy as np
import torch

CASES = [(4, 4), (5, 6), (2, 3, 4, 4), (1, 8, 8), (24, 8), (48, 4), (64, 4), (64,), (16, 16), (16, 16, 16)]
SMALL = CASES[:5]                       # "every case up to (24, 8)": what the dense CPU comparisons run
CHAINS = (1, 3, 5)
REFUSED = [((128, 128), torch.float32, "axis of 128 sites"), ((65, 4), torch.float32, "axis of 65 sites"),
           ((64, 128), torch.float64, "axis of 128 sites"), ((16, 16), torch.float16, "dtype"),
           ((8, 64, 64), torch.float32, "LDS image"), ((2, 64, 64), torch.float64, "exceed")]
COUPLINGS = dict(kappa=0.67, m_sq=-2.68, lambd=0.5)      # tests/hmc_cases.py INTERACTING
MASS_SQ = 0.5
LEAPFROG = ((1.0,), (1.0,))
_LAMBDA = 0.1931833275037836
OMELYAN = ((0.5, 0.5), (1.0 - 2.0 * _LAMBDA, 2.0 * _LAMBDA))
SCHEMES = dict(leapfrog=LEAPFROG, omelyan=OMELYAN)
PI_LD = np.longdouble("3.14159265358979323846264338327950288")
name = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def chains_for(lattice):
    """One C of {1, 3, 5} per case, every value used."""
    return CHAINS[CASES.index(lattice) % 3]


def shat(L):
    """4 sin^2(pi k / L), k = 0 .. L - 1, in long double, rounded once; nothing for an axis of extent 1."""
    if L == 1:
        return np.zeros(1)
    k = np.arange(L, dtype=np.longdouble)
    return np.asarray(4.0 * np.sin(PI_LD * k / L) ** 2, dtype=np.float64)


def denominator(lattice, w0, mass_sq):
    """w0 sum_mu shat_mu(k_mu) + M^2 on the momentum lattice, the axes summed left to right."""
    d = len(lattice)
    s = None
    for mu, L in enumerate(lattice):
        term = shat(L).reshape((1,) * mu + (L,) + (1,) * (d - 1 - mu))
        s = term if s is None else s + term
    return w0 * np.broadcast_to(s, lattice) + mass_sq


def hartley(N):
    """H_N[k, n] = (cos(2 pi k n / N) + sin(2 pi k n / N)) / sqrt(N), the angle reduced exactly."""
    kn = np.outer(np.arange(N), np.arange(N)) % N
    ang = 2.0 * np.pi * kn / N
    return (np.cos(ang) + np.sin(ang)) / np.sqrt(N)


def transform(x, lattice):
    """T x for x (C, *L): one dense matrix product per axis."""
    for mu, L in enumerate(lattice):
        if L > 1:
            x = np.moveaxis(np.tensordot(hartley(L), x, axes=([1], [mu + 1])), 0, mu + 1)
    return x


def coef(lattice, kappa, m_sq, lambd):
    """(w0, w2, w4) of ScalarPhi4Action at a = 1, typed again."""
    d = len(lattice)
    return kappa, (m_sq + 2 * d * kappa) / 2, lambd


def action(phi, lattice, w0, w2, w4):
    """S, every axis rolled (an axis of extent 1 onto itself, as ScalarPhi4Action does)."""
    S = (w2 * phi ** 2 + w4 * phi ** 4).reshape(phi.shape[0], -1).sum(1)
    for mu in range(len(lattice)):
        S = S - w0 * (phi * np.roll(phi, 1, axis=mu + 1)).reshape(phi.shape[0], -1).sum(1)
    return S


def force(phi, lattice, w0, w2, w4):
    F = 2 * w2 * phi + 4 * w4 * phi ** 3
    for mu in range(len(lattice)):
        F = F - w0 * (np.roll(phi, 1, axis=mu + 1) + np.roll(phi, -1, axis=mu + 1))
    return F


def ref_trajectory(phi, pi, lattice, couplings, n_md, dt, mass_sq, scheme=LEAPFROG):
    """One accelerated trajectory from given pi (steps 2 to 5 of the header) in fp64: dict(phi, pi, dh, h0, h1)."""
    phi = np.asarray(phi.detach().double().cpu().numpy() if torch.is_tensor(phi) else phi, dtype=np.float64)
    pi = np.asarray(pi.detach().double().cpu().numpy() if torch.is_tensor(pi) else pi, dtype=np.float64)
    w = coef(lattice, **couplings)
    a = 1.0 / denominator(lattice, w[0], mass_sq)
    A = lambda p: transform(a * transform(p, lattice), lattice)
    H = lambda ph, p: 0.5 * (p * A(p)).reshape(p.shape[0], -1).sum(1) + action(ph, lattice, *w)
    wa, wb = scheme
    s, half = len(wa), 0.5 * wb[-1] * dt
    h0 = H(phi, pi)
    pi = pi - half * force(phi, lattice, *w)
    for k in range(1, n_md + 1):
        for j in range(s):
            phi = phi + (wa[j] * dt) * A(pi)
            pi = pi - (half if k == n_md and j == s - 1 else wb[j] * dt) * force(phi, lattice, *w)
    h1 = H(phi, pi)
    return dict(phi=torch.from_numpy(phi), pi=torch.from_numpy(pi), dh=torch.from_numpy(h1 - h0),
                h0=torch.from_numpy(h0), h1=torch.from_numpy(h1))


def refresh(eta, lattice, w0, mass_sq):
    """pi = A^(-1/2) eta (step 1)."""
    eta = np.asarray(eta.detach().double().cpu().numpy(), dtype=np.float64)
    return torch.from_numpy(transform(np.sqrt(denominator(lattice, w0, mass_sq)) * transform(eta, lattice), lattice))


def starts(shape, seed, scale=0.7):
    """(phi0, pi0) fp64 on the CPU."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (scale * torch.randn(shape, generator=g, dtype=torch.float64, device="cpu"),
            torch.randn(shape, generator=g, dtype=torch.float64, device="cpu"))


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


def free_phi2(lattice, kappa, m_sq):
    """sum_k 1 / (kappa khat^2 + m^2) / V: <phi^2> of the free field (S = phi^T (kappa khat^2 + m^2) phi / 2)."""
    return float((1.0 / denominator(lattice, kappa, m_sq)).mean())


def lag1(x):
    """The lag-1 autocorrelation of the series x (T, C) of C equivalent chains, around the mean over chains and time
    (a chain's own mean of a short series would bias it by -1 / T)."""
    x = x.double() - x.double().mean()
    return ((x[1:] * x[:-1]).mean() / x.square().mean()).item()


FREE = dict(kappa=1.0, m_sq=1.0, lambd=0.0)


def _chain_stats(y):
    """(mean, standard error across chains) of <phi^2> from y (T, C, V)."""
    per_chain = y.square().mean(dim=(0, 2))
    return per_chain.mean().item(), per_chain.std().item() / y.shape[1] ** 0.5


def free_field_run(m, Cn, path, fa_mass_sq, seed=17):
    """24 trajectories of Cn chains from the prior, the first 4 dropped: (<phi^2>, its chain-to-chain standard error,
    acceptance, lag-1 autocorrelation of V m^2)."""
    torch.manual_seed(seed)
    lattice = tuple(m.prior.sample(1).shape[1:])
    kw = {} if fa_mass_sq is None else dict(fa_mass_sq=fa_mass_sq)
    y = m.hmc.start(n_chains=Cn).sample(24 * Cn, n_chains=Cn, n_md=8, dt=math.pi / 16, path=path, **kw)
    V = math.prod(lattice)
    y = y.double().cpu().reshape(24, Cn, V)[4:]
    mean, err = _chain_stats(y)
    mag2 = y.mean(dim=2).square() * V
    return mean, err, m.hmc.last['accept'].double().mean().item(), lag1(mag2)

"""Shared by tests/test_cluster_ladder_host.py and tests/test_cluster_ladder.py: the hopping coefficients of the rungs, the
coefficient tables, the fields and the case lists of the ladder cluster kernels.  The host test asserts the tie guard of
tests/cluster_cases.py on every (lattice, dtype, rung) listed here; the GPU test compares them bit for bit."""
import numpy as np
import torch

import cluster_cases as Cc
import ladder_cases as Lc

# the w0 of the rungs: three around cluster_cases.W0 (K = 3), and W0 itself (K = 1)
W0S = {1: (Cc.W0,), 3: (0.57, Cc.W0, 0.77)}
CHAINS = 6
DTYPES = ('float32', 'float64')
FUSED_LATTICES = [lat for lat in Cc.LATTICES if lat != (64, 64)]
TILED_LATTICES = [(8, 8), (4, 4, 4), (2, 2, 2, 2)]
TILES = (16, 64, 0)
BIG = ((32, 32, 32), 'float32', 3, 3)              # (lattice, dtype, chains, K): beyond nf_phi4_cluster's class
# (lattice, dtype name, chains, K) of every comparison on the device
FUSED = [(lat, dt, CHAINS, K) for lat in FUSED_LATTICES for dt in DTYPES for K in (1, 3)]
TILED = [(lat, dt, CHAINS, K) for lat in TILED_LATTICES for dt in DTYPES for K in (1, 3)]
ALL = FUSED + TILED + [BIG]


def case_id(case):
    lat, dt, chains, K = case
    return f"{'x'.join(map(str, lat))}-{dt}-K{K}"


def coef_table(K, device=None):
    """(K, 3) float64: (w0_k, w2, w4) with w2 and w4 that no sweep may read (NaN would show in a bond)."""
    return torch.tensor([[w0, float('nan'), float('nan')] for w0 in W0S[K]], dtype=torch.float64, device=device)


def rung(chains, K, device=None):
    """(chains) int32: per replica set a permutation of the rungs that is not the identity."""
    return Lc.permuted_rung(chains // K, K, seed=17 + chains + K, device=device)


def field(case):
    lat, dt, chains, _ = case
    return Cc.field(lat, dt, chains)


def rows_of(r, K):
    """The rung-ordered stats row of every chain: (c // K) K + rung[c]."""
    r = np.asarray(r, dtype=np.int64)
    return np.arange(r.shape[0]) // K * K + r

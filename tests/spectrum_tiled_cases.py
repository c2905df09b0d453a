"""Shared by tests/test_cluster_spectrum_tiled_host.py and tests/test_cluster_spectrum_tiled.py: the case lists of
nf_cluster_spectrum_tiled and its planner's table, written out from the formulas of include/normflow_hip.h.  The numpy
restatement, the comparison and the bound (V + 8) 2^-53 sum |terms| are those of tests/spectrum_cases.py, unchanged: the
bound holds for a double sum of the V terms in ANY order, so it covers the blocked order of the tiled kernel.  The fields
and the synthetic labels are those of tests/improved_cases.py, the colliding keys those of
tests/cluster_moments_tiled_cases.py."""
import numpy as np

import improved_cases as Ic
from cluster_moments_tiled_cases import KINDS, collide_labels                   # noqa: F401
from spectrum_cases import check_against, column, kmax_of, restate, select, tile           # noqa: F401

DTYPES = Ic.DTYPES
DEFAULT_BLOCK = 4096
TABLE = 512                       # H: labels k, k + H, k + 2 H share an entry
LANES = 256
MAX_PASS = 16                     # quantities per pass
MAX_Q = 1024
# odd extents, Nyquist on extents 2 and 6, an axis of extent 1; (1, 2, 16) at 'all' has Q = 17 and crosses a pass of 16;
# (6, 6, 6, 6) has V = 1296 > H, so labels collide in the table
LATTICES = [(8,), (3, 5), (16, 16), (5, 7, 3), (1, 2, 16), (2, 2, 2, 2), (6, 6, 6, 6)]
CASES = [(lat, dt) for lat in LATTICES for dt in DTYPES]
MOMENTA = (1, 3, 'all')
CHAINS = (1, 3, 300)
PER_PASS = (None, 1, 2, 5, 16)    # the last clipped to Q
LARGE = [((32, 32, 32), 'float32', 'all', 2), ((16, 16, 16, 16), 'float64', 3, 1)]


def case_id(case):
    return Ic.case_id(case)


def volume(lat):
    return Ic.volume(lat)


def blocks_of(lat):
    """block_sites in {1, 7, 64, 256, 257, 1000, V, V + 1, 0}."""
    V = volume(lat)
    return [1, 7, 64, 256, 257, 1000, V, V + 1, 0]


def quantities(lat, momenta):
    """Q = 1 + sum_mu (2 K_mu - [2 K_mu = L_mu])."""
    return 1 + sum(2 * K - (1 if K and 2 * K == n else 0) for K, n in zip(kmax_of(lat, momenta), lat))


def columns(lat, momenta):
    return 2 + sum(kmax_of(lat, momenta))


def per_pass_of(pp, lat, momenta):
    """A value of PER_PASS as the wrapper takes it: None stays, the others are clipped to min(Q, 16)."""
    return None if pp is None else min(pp, quantities(lat, momenta), MAX_PASS)


def pairing(lat):
    """Nine (block_sites, per_pass, momenta, C): every value of every list meets the lattice at least once, instead of the
    full product.  block_sites goes through its list, per_pass and momenta go round theirs, C changes every third."""
    return [(bs, per_pass_of(PER_PASS[n % 5], lat, MOMENTA[n % 3]), MOMENTA[n % 3], CHAINS[(n // 3) % 3])
            for n, bs in enumerate(blocks_of(lat))]


def lds(per_pass):
    """The scatter kernel's table: int32 keys and per_pass arrays of int64 sums."""
    return TABLE * (4 + 8 * per_pass)


def workspace(C, lat, momenta, block_sites, per_pass):
    """The header's formula: 4 C bytes of flags rounded up to 16, per_pass C V 8 of slots, C (Q + 1) blocks doubles."""
    V, Q = volume(lat), quantities(lat, momenta)
    bs = min(block_sites or DEFAULT_BLOCK, V)
    blocks = -(-V // bs)
    pp = per_pass or min(Q, MAX_PASS)
    return (4 * C + 15) // 16 * 16 + pp * C * V * 8 + C * (Q + 1) * blocks * 8


# (lattice, momenta, block_sites, per_pass) -> (blocks, block_sites in force, Q, columns, per_pass in force, passes,
# launches): blocks = ceil(V / block_sites in force), Q and columns from the formulas above, per_pass 0 = min(Q, 16),
# passes = ceil(Q / per_pass), launches = 2 + 2 passes
PLAN = {
    ((32, 32, 32), 'all', 0, 0): (8, 4096, 94, 50, 16, 6, 14),          # Q = 1 + 3 (2 x 16 - 1), columns = 2 + 3 x 16
    ((16, 16, 16, 16), 'all', 0, 0): (16, 4096, 61, 34, 16, 4, 10),     # Q = 1 + 4 (2 x 8 - 1)
    ((32, 32, 32, 32), 'all', 0, 7): (256, 4096, 125, 66, 7, 18, 38),   # Q = 1 + 4 x 31, ceil(125 / 7) = 18
    ((48, 48, 48, 48), 'all', 0, 6): (1296, 4096, 189, 98, 6, 32, 66),  # Q = 1 + 4 x 47, ceil(189 / 6) = 32
    ((32, 32, 32), 1, 0, 0): (8, 4096, 7, 5, 7, 1, 4),
    ((1, 2, 16), 'all', 0, 0): (1, 32, 17, 11, 16, 2, 6),               # Q = 1 + 1 + 15, columns = 2 + 1 + 8
    ((6, 6, 6, 6), 'all', 0, 0): (1, 1296, 21, 14, 16, 2, 6),           # Q = 1 + 4 (2 x 3 - 1)
    ((2, 2, 2, 2), 'all', 0, 0): (1, 16, 5, 6, 5, 1, 4),
    ((5, 7, 3), 'all', 0, 0): (1, 105, 13, 8, 13, 1, 4),                # Q = 1 + 4 + 6 + 2, columns = 2 + 2 + 3 + 1
    ((64,), 'all', 0, 0): (1, 64, 64, 34, 16, 4, 10),                   # Q = 1 + 63
    ((6, 6, 6, 6), 3, 257, 5): (6, 257, 21, 14, 5, 5, 12),
    ((16, 16), 'all', 64, 1): (4, 64, 31, 18, 1, 31, 64),
    ((16, 16), 2, 257, 0): (1, 256, 9, 6, 9, 1, 4),
    ((48, 48, 48, 48), 4, 8192, 16): (648, 8192, 33, 18, 16, 3, 8),
    ((1,), 'all', 0, 0): (1, 1, 1, 2, 1, 1, 4),
}
# (chains, lattice) at 'all' -> the per_pass that per_pass=None takes under the default footprint of 1 GiB: the largest
# p <= min(Q, 16) with flags + p C V 8 + C (Q + 1) blocks 8 <= 2^30.  (256, 32^3): C V 8 = 64 MiB, the partials 1.5 MiB:
# 15.  (64, 16^4): C V 8 = 32 MiB: 16.  (16, 32^4): 128 MiB and 3.9 MiB of partials: 7.  (4, 48^4): 162 MiB and 7.5 MiB: 6.
DEFAULT_PER_PASS = {(256, (32, 32, 32)): 15, (64, (16, 16, 16, 16)): 16, (16, (32, 32, 32, 32)): 7, (4, (48, 48, 48, 48)): 6,
                    (300, (6, 6, 6, 6)): 16, (64, (48, 48, 48, 48)): 1}


def synthetic(kind, chains, V):
    """Labels of the kinds that need no sweep, 'collide' included."""
    return collide_labels(chains, V) if kind == 'collide' else Ic.synthetic_labels(kind, chains, V)


def fields(lat, dt, chains):
    """(chains, V): chain i of kind i % 7; the chains of kind 0 (a sweep at kappa = 0.67) are ordered fields."""
    phi = Ic.field(lat, dt, chains)
    phi[0::len(KINDS)] = Ic.field(lat, dt, chains, ordered=True)[0::len(KINDS)]
    return phi


assert all(np.prod(lat) >= 1 for lat in LATTICES)

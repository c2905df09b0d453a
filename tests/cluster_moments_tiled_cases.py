"""Shared by tests/test_cluster_moments_tiled_host.py and tests/test_cluster_moments_tiled.py: the case lists of
nf_cluster_moments_tiled.  The numpy restatement, the comparison, the fields, the synthetic labels and the bound
(V + 8) 2^-53 sum |terms| are those of tests/improved_cases.py, unchanged: the bound holds for a double sum of the V terms in
ANY order, so it covers the blocked order of the tiled kernel as it covers the one-workgroup order."""
import numpy as np

from improved_cases import (DTYPES, case_id, check_against, columns, field, lat4, limit, restate, synthetic_labels,  # noqa: F401
                            twiddles, volume)

DEFAULT_BLOCK = 4096
TABLE = 512                       # H: labels k, k + H, k + 2 H share an entry
LANES = 256
LDS = TABLE * (4 + 8 * 9)         # the scatter kernel's table: int32 keys and 9 arrays of int64 sums
LATTICES = [(8,), (3, 5), (16, 16), (5, 7, 3), (1, 2, 16), (2, 2, 2, 2), (6, 6, 6, 6)]
CASES = [(lat, dt) for lat in LATTICES for dt in DTYPES]
CHAINS = (1, 3, 300)
PER_PASS = (None, 1, 2)
KINDS = ('sweep67', 'sweep25', 'zero', 'arange', 'alternate', 'random', 'collide')
LARGE = [((32, 32, 32), 'float32', 2), ((16, 16, 16, 16), 'float64', 1)]


def blocks_of(lat):
    """block_sites in {1, 7, 64, 256, 257, 1000, V, V + 1, 0}."""
    V = volume(lat)
    return [1, 7, 64, 256, 257, 1000, V, V + 1, 0]


def quantities(lat):
    return 1 + 2 * sum(1 for n in lat if n > 1)


def collide_labels(chains, V, seed=0):
    """Keys k, k + H, k + 2 H, ... that share ONE entry of the table, site by site at random (all of them where V <= H:
    then there is one key).  Neighbouring lanes race for the entry, the losers go straight to HBM."""
    rng = np.random.default_rng(seed + 3 * V)
    k = 5 % V
    keys = np.arange(k, V, TABLE)
    return keys[rng.integers(0, len(keys), size=(chains, V))].astype(np.int32)


def workspace(C, lat, block_sites, per_pass):
    """The header's formula: 4 C bytes of flags rounded up to 16, per_pass C V 8 of slots, C blocks 10 doubles."""
    V = volume(lat)
    bs = min(block_sites or DEFAULT_BLOCK, V)
    blocks = -(-V // bs)
    pp = per_pass or quantities(lat)
    return (4 * C + 15) // 16 * 16 + pp * C * V * 8 + C * blocks * 10 * 8


# (lattice, block_sites, per_pass) -> (blocks, block_sites in force, quantities, per_pass in force, passes, launches)
PLAN = {
    ((32, 32, 32), 0, 0): (8, 4096, 7, 7, 1, 4), ((16, 16, 16, 16), 0, 0): (16, 4096, 9, 9, 1, 4),
    ((32, 32, 32, 32), 0, 7): (256, 4096, 9, 7, 2, 6), ((48, 48, 48, 48), 0, 6): (1296, 4096, 9, 6, 2, 6),
    ((48, 48, 48, 48), 8192, 1): (648, 8192, 9, 1, 9, 20), ((32, 32, 32), 2048, 2): (16, 2048, 7, 2, 4, 10),
    ((8,), 1, 0): (8, 1, 3, 3, 1, 4), ((3, 5), 7, 1): (3, 7, 5, 1, 5, 12), ((16, 16), 257, 2): (1, 256, 5, 2, 3, 8),
    ((16, 16), 255, 5): (2, 255, 5, 5, 1, 4), ((5, 7, 3), 257, 3): (1, 105, 7, 3, 3, 8), ((5, 7, 3), 106, 0): (1, 105, 7, 7, 1, 4),
    ((1, 2, 16), 7, 4): (5, 7, 5, 4, 2, 6), ((2, 2, 2, 2), 1, 9): (16, 1, 9, 9, 1, 4), ((6, 6, 6, 6), 257, 0): (6, 257, 9, 9, 1, 4),
    ((1,), 0, 0): (1, 1, 1, 1, 1, 4), ((1, 1, 1, 7), 0, 3): (1, 7, 3, 3, 1, 4),
}
# (chains, lattice) -> the per_pass that per_pass=None takes under the default footprint of 1 GiB, and the passes
DEFAULT_PER_PASS = {(256, (32, 32, 32)): (7, 1), (64, (16, 16, 16, 16)): (9, 1), (16, (32, 32, 32, 32)): (7, 2),
                    (4, (48, 48, 48, 48)): (6, 2), (64, (48, 48, 48, 48)): (1, 9), (300, (6, 6, 6, 6)): (9, 1)}

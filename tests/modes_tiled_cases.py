"""Shared by tests/test_cluster_modes_tiled_host.py and tests/test_cluster_modes_tiled.py: the case lists of
nf_cluster_modes_tiled and its planner's table, written out from the formulas of include/normflow_hip.h ("cluster modes with
the chains, the labels and the int64 slots in HBM").  The numpy restatement, the comparison and the bound
(V + 8) 2^-53 sum |terms| are those of tests/modes_cases.py, unchanged: the bound holds for a double sum of the V terms in
ANY order, so it covers the blocked order of the tiled kernel.  (The restatement forms the phase in int64: the exact
integer.)  The fields and the synthetic labels are those of tests/improved_cases.py, the label kinds and the colliding keys
those of tests/cluster_moments_tiled_cases.py."""
import numpy as np

import improved_cases as Ic
from cluster_moments_tiled_cases import KINDS, collide_labels                   # noqa: F401
from modes_cases import (POW2_RATIO, check_against, lcm, mode_lists, quantities, reduce, restate, self_conjugate,   # noqa: F401
                         table, tile, twiddles)

DTYPES = Ic.DTYPES
DEFAULT_BLOCK = 4096
TABLE = 512                       # H: labels k, k + H, k + 2 H share an entry
LANES = 256
MAX_PASS = 16                     # quantities per pass
MAX_Q = 1025
# (3, 5) has N = 15 and (5, 7, 3) has N = 105: N / L is no power of two; (6, 6, 6, 6) has V = 1296 > H, so labels collide in
# the table; (65536, 4) has V = 262144 and N = 65536: an extent at the cap
BIG = (65536, 4)
# m = (65535, 49152) for the first momentum: at x = (65535, 3) sum m x = 65535 x 65535 + 49152 x 3 = 4294983681 > 2^32,
# the smallest case where the phase sum leaves 32 bits.  (There N = 2^16 divides 2^32 and a wrapped sum keeps its residue;
# on WRAP = (65535, 15), N = 65535, it does not: m = (65534, 61166) at x = (65534, 14) gives 4295561480, whose residue is
# 4370 and whose low 32 bits have the residue 4369.)
BIG_LIST = [(-1, -1), (1, 0), (0, 1)]
WRAP = (65535, 15)
LATTICES = [(8,), (3, 5), (16, 16), (5, 7, 3), (1, 2, 16), (2, 2, 2, 2), (6, 6, 6, 6), BIG]
CASES = [(lat, dt) for lat in LATTICES for dt in DTYPES]
CHAINS = (1, 3, 300)
PER_PASS = (None, 1, 2, 5, 16)    # the last clipped to Q; 1 and 5 put pass boundaries between an R and its I
LARGE = [((32, 32, 32), 'float32', 2), ((16, 16, 16, 16), 'float64', 1)]

assert 65535 * 65535 + 49152 * 3 == 4294983681 > 2 ** 32


def case_id(case):
    return Ic.case_id(case)


def volume(lat):
    return Ic.volume(lat)


def lists_of(lat):
    """name -> momentum list: `modes_cases.mode_lists`, and on (65536, 4) the one list the case is there for."""
    return {'wrap': BIG_LIST} if tuple(lat) == BIG else mode_lists(lat)


def blocks_of(lat):
    """block_sites in {1, 7, 64, 256, 257, 1000, V, V + 1, 0}."""
    V = volume(lat)
    return [1, 7, 64, 256, 257, 1000, V, V + 1, 0]


def columns(modes):
    return 2 + len(modes)


def per_pass_of(pp, lat, modes):
    """A value of PER_PASS as the wrapper takes it: None stays, the others are clipped to min(Q, 16)."""
    return None if pp is None else min(pp, quantities(lat, modes), MAX_PASS)


def pairing(lat):
    """Nine (block_sites, per_pass, name of the list, C): every value of every list meets the lattice at least once,
    instead of the full product, as `spectrum_tiled_cases.pairing` does it.  block_sites goes through its list, per_pass
    and the momentum lists go round theirs, C changes every third."""
    names = list(lists_of(lat))
    out = []
    for n, bs in enumerate(blocks_of(lat)):
        name = names[n % len(names)]
        out.append((bs, per_pass_of(PER_PASS[n % 5], lat, lists_of(lat)[name]), name, CHAINS[(n // 3) % 3]))
    return out


def lds(per_pass):
    """The scatter kernel's table: int32 keys and per_pass arrays of int64 sums."""
    return TABLE * (4 + 8 * per_pass)


def workspace(C, lat, Q, block_sites, per_pass):
    """The header's formula: 4 C bytes of flags rounded up to 16, per_pass C V 8 of slots, C (Q + 1) blocks doubles."""
    V = volume(lat)
    bs = min(block_sites or DEFAULT_BLOCK, V)
    blocks = -(-V // bs)
    pp = per_pass or min(Q, MAX_PASS)
    return (4 * C + 15) // 16 * 16 + pp * C * V * 8 + C * (Q + 1) * blocks * 8


def correlator_list(lat, axis, spatial):
    """The L momenta (k along `axis`, `spatial` elsewhere) of the time-slice correlator at a spatial momentum."""
    return [tuple(spatial[:axis]) + (k,) + tuple(spatial[axis:]) for k in range(lat[axis])]


GENERAL3 = ((1, 1, 0), (1, 2, 3), (0, 1, -1))
CORR16 = tuple(correlator_list((16, 16, 16, 16), 0, (1, 0, 0)))
TWENTY = tuple((1 + k % 5, k % 3, 1, k) for k in range(20))           # general on 48^4: component 2 is 1, never 0 or 24
# (lattice, momenta, block_sites, per_pass) -> (blocks, block_sites in force, N, columns, Q, per_pass in force, passes,
# launches, LDS bytes): blocks = ceil(V / block_sites in force), N = lcm of the extents, columns = 2 + P,
# Q = 1 + sum (2 - [self-conjugate]), per_pass 0 = min(Q, 16), passes = ceil(Q / per_pass), launches = 2 + 2 passes,
# LDS = 512 (4 + 8 per_pass)
PLAN = {
    ((32, 32, 32), GENERAL3, 0, 0): (8, 4096, 32, 5, 7, 7, 1, 4, 512 * (4 + 56)),             # 30720
    ((16, 16, 16, 16), CORR16, 0, 0): (16, 4096, 16, 18, 33, 16, 3, 8, 512 * (4 + 128)),      # Q = 1 + 2 x 16
    (BIG, tuple(BIG_LIST), 0, 0): (64, 4096, 65536, 5, 7, 7, 1, 4, 30720),
    ((6, 6, 6, 6), ((0, 0, 0, 0), (3, 3, 3, 3), (1, 0, 0, 0)), 257, 2): (6, 257, 6, 5, 5, 2, 3, 8, 512 * 20),   # two R alone
    ((3, 5), ((1, 1),), 0, 0): (1, 15, 15, 3, 3, 3, 1, 4, 512 * 28),
    ((5, 7, 3), ((1, 1, 1), (2, 3, 1)), 1000, 1): (1, 105, 105, 4, 5, 1, 5, 12, 512 * 12),
    ((48, 48, 48, 48), TWENTY, 8192, 16): (648, 8192, 48, 22, 41, 16, 3, 8, 512 * 132),
    ((1, 2, 16), ((0, 1, 8), (0, 0, 1)), 0, 0): (1, 32, 16, 4, 4, 4, 1, 4, 512 * 36),         # (0, 1, 8) is a Nyquist corner
    ((16, 16), ((1, 2),), 64, 1): (4, 64, 16, 3, 3, 1, 3, 8, 512 * 12),
}
# (chains, lattice, Q) -> the per_pass that per_pass=None takes under the default footprint of 1 GiB: the largest
# p <= min(Q, 16) with flags + p C V 8 + C (Q + 1) blocks 8 <= 2^30.  (256, 32^3): C V 8 = 64 MiB and 0.5 MiB of partials:
# 15.  (64, 16^4): 32 MiB: 16.  (16, 32^4): 128 MiB and 1.1 MiB: 7.  (4, 48^4): 162 MiB and 1.3 MiB: 6.  (64, 48^4): 2.5 GiB: 1.
DEFAULT_PER_PASS = {(256, (32, 32, 32), 33): 15, (64, (16, 16, 16, 16), 33): 16, (16, (32, 32, 32, 32), 33): 7,
                    (4, (48, 48, 48, 48), 33): 6, (64, (48, 48, 48, 48), 7): 1, (300, (6, 6, 6, 6), 5): 5,
                    (16, (32, 32, 32, 32), 5): 5}


def synthetic(kind, chains, V):
    """Labels of the kinds that need no sweep, 'collide' included."""
    return collide_labels(chains, V) if kind == 'collide' else Ic.synthetic_labels(kind, chains, V)


def fields(lat, dt, chains):
    """(chains, V): chain i of kind i % 7; the chains of kind 0 (a sweep at kappa = 0.67) are ordered fields."""
    phi = Ic.field(lat, dt, chains)
    phi[0::len(KINDS)] = Ic.field(lat, dt, chains, ordered=True)[0::len(KINDS)]
    return phi


def host_labels(lat, chains):
    """(chains, V) labels without a sweep, for the host tests: chain i of the synthetic kind i % 5."""
    kinds = [k for k in KINDS if not k.startswith('sweep')]
    V = volume(lat)
    lab = np.zeros((chains, V), dtype=np.int32)
    for i, kind in enumerate(kinds):
        n = len(range(i, chains, len(kinds)))
        if n:
            lab[i::len(kinds)] = synthetic(kind, n, V)
    return lab


assert all(np.prod(lat) >= 1 for lat in LATTICES)

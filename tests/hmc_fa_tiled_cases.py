"""Shared by tests/test_hmc_fa_tiled_host.py and tests/test_hmc_fa_tiled.py: the lattices of the suites of
nf_phi4_hmc_fa_tiled (the Fourier-accelerated HMC with the chains in HBM) and the planner of include/normflow_hip.h ("the
same with the chains in HBM") typed again in Python.  The numpy restatement of the trajectory is tests/hmc_fa_cases.py's.

Each small shape is the smallest one that reaches a particular piece of code:
    (4, 4)                       the smallest case
    (5, 6, 7)                    odd, unequal extents; three matrices; line counts that are no multiple of 16
    (2, 3, 4, 4)                 four axes; extent 2; a shared matrix; eight cuts
    (1, 8, 8)                    a user axis of extent 1
    (24, 8), (48, 4), (64, 4)    2 / 3 / 4 output tiles per line, with the boundary between the two axes
    (64,)                        one axis
    (9, 3, 4)                    two marched segments in the step, the second shorter
Under the planner's 32 KiB panels every group of those has ONE panel per chain, so three more carry the panels that the
large lattices have -- several per chain, the last one shorter -- at the smallest sizes that give them under a cut:
    (6, 45, 51)    cut 1: the group (0,) in runs of 1148 + 1147 (fp32) / 3 x 574 + 573 (fp64) sites that are no multiple of
                   16 bytes, from rows of 2295: single-site accesses
    (6, 50, 50)    cut 1: the same group in runs of 1252 + 1248 / 3 x 626 + 622 sites: 16-byte accesses, a shorter last run
    (22, 30, 30)   cut 1: the group (1, 2) in panels of 8 + 8 + 6 / 5 x 4 + 2 values of the index in front of it"""
import math

import torch

import hmc_fa_cases as FA

F32, F64 = torch.float32, torch.float64
SMALL = [(4, 4), (5, 6, 7), (2, 3, 4, 4), (1, 8, 8), (24, 8), (48, 4), (64, 4), (64,), (9, 3, 4)]
RAGGED = [(6, 45, 51), (6, 50, 50), (22, 30, 30)]
BOTH = [(16, 16), (16, 16, 16)]                     # nf_phi4_hmc_fa takes them too
BEYOND = [((32, 32, 32), F32), ((32, 32, 32), F64), ((16, 16, 16, 16), F32)]      # beyond one CU: g >= 2
TABLE = [(32, 32, 32), (16, 16, 16, 16), (32, 32, 32, 32), (48, 48, 48, 48), (64, 64, 64)]      # the README's plan table
CHAINS = (1, 3, 5)
LDS_MAX, LDS_TARGET, PANEL, RUN_BYTES, MAX_AXIS = 160 * 1024, 80 * 1024, 32 * 1024, 64, 64
MAX_LAUNCHES = 65536
name = FA.name
dt_name = lambda v: str(v).replace("torch.", "")


def chains_for(lattice):
    """One C of {1, 3, 5} per small case, every value used."""
    return CHAINS[(SMALL + RAGGED).index(lattice) % 3]


def legal_cuts(lattice):
    """The masks (bit mu: a boundary between the axes mu and mu + 1 of `lattice`) with no boundary at an axis of extent 1."""
    d = len(lattice)
    return [m for m in range(1 << (d - 1))
            if all(not (m >> mu & 1) or (lattice[mu] > 1 and lattice[mu + 1] > 1) for mu in range(d - 1))]


def groups_of(lattice, cut):
    """[(first axis, last axis)] of the groups of the mask `cut`, the slowest first."""
    out, lo = [], 0
    for mu in range(len(lattice)):
        if mu == len(lattice) - 1 or cut >> mu & 1:
            out.append((lo, mu))
            lo = mu + 1
    return out


def matrix_elements(extents):
    """The Hartley matrices of nf_spectral.hip for these extents: per distinct extent > 1 the rows padded to the 16-tile
    and a row stride of that padding, plus 16 where the padding is a multiple of 32."""
    total = 0
    for n in set(n for n in extents if n > 1):
        pad16 = (n + 15) // 16 * 16
        total += pad16 * (pad16 if pad16 % 32 == 16 else pad16 + 16)
    return total


def group_plan(lattice, lo, hi, size):
    """The header's sizing rule for the group of the axes lo .. hi: None where its one line of sites and its matrices
    exceed the LDS, else dict(run, run_inner, panels, panel_sites, lanes, lds_bytes, matrix_bytes, eligible, stretch)."""
    G, O, I = math.prod(lattice[lo:hi + 1]), math.prod(lattice[:lo]), math.prod(lattice[hi + 1:])
    hb, unit, vec = matrix_elements(lattice[lo:hi + 1]) * size, G * size, 16 // size
    if unit + hb > LDS_MAX:
        return None
    budget = (LDS_TARGET if unit + hb <= LDS_TARGET else LDS_MAX) - hb
    rmin = min(I, RUN_BYTES // size) if I > 1 else 1
    cap = min(max(PANEL, unit * rmin), budget) // unit
    ri = 1
    if I > 1:
        rmax = min(cap, I)
        ri = -(-I // -(-I // rmax))
        up = -(-ri // vec) * vec
        ri = up if up <= rmax else ri
    ro = 1
    if ri == I:
        omax = max(1, min(O, cap // I))
        ro = -(-O // -(-O // omax))
    sites = ro * G * ri
    return dict(axes=tuple(range(lo, hi + 1)), run=ro * ri, run_inner=ri, panels=-(-O // ro) * -(-I // ri), panel_sites=sites,
                lanes=min(512, -(-(-(-sites // 8)) // 64) * 64), lds_bytes=-(-sites // vec) * vec * size + hb, matrix_bytes=hb,
                eligible=unit * rmin + hb <= LDS_TARGET, stretch=(sites if ri == I else ri) * size)


def plan(lattice, dtype, cut=None):
    """(the mask, the groups' dicts) as the header states the planner; None where no cut fits (or `cut` does not)."""
    size = 4 if dtype == F32 else 8
    if cut is not None:
        gs = [group_plan(lattice, lo, hi, size) for lo, hi in groups_of(lattice, cut)]
        return None if None in gs else (cut, gs)
    best = None
    for m in legal_cuts(lattice):
        got = plan(lattice, dtype, m)
        if got is None:
            continue
        key = (not all(g['eligible'] for g in got[1]), len(got[1]), -min(g['stretch'] for g in got[1]), m)
        if best is None or key < best[0]:
            best = (key, got)
    return None if best is None else best[1]


def launches(groups, evals):
    """draw, refresh filter, H0 filter, begin, per force evaluation a filter and a step, H1 filter, the partials of the
    end, commit -- a filter being 2 g - 1 passes."""
    passes = 2 * groups - 1
    return 1 + passes + passes + 1 + evals * (passes + 1) + passes + 1 + 1

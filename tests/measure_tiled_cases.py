"""Shared by tests/test_measure_tiled_host.py and tests/test_measure_tiled.py: the (lattice, brick cap) cases of the
brick-tiled measure kernel, nf_lattice_measure_tiled, and the regimes of the kernel that a case exercises, derived from
nf_lattice_measure_tiled_plan (pure host code), not from knowledge of the planner.  The rows, the numpy reference, the
unpacking of an output row and the worst-case bound (terms + 4) 2^-53 sum |terms| are tests/measure_cases.py's, by import.

A case is (lattice, cap): cap = the brick_bytes handed to the kernel, None for the library's default.  The forced caps
are a few dozen bytes so that lattices of a few hundred sites are cut the way 48^4 is cut by 32 KiB.

Regimes, from the plan and the case (a0 / a1: the plan's cut axes; pieces: the lengths of the bricks along an axis):
    cut0_only        a0 is cut, a1 (if there is one) is not: bricks of whole planes
    planes           ... of more than one plane (e0 > 1);  planes_ragged: the last brick has fewer planes
    cut1             a1 is cut (n1 >= 2; then e0 = 1): both halos come from HBM
    cut1_even, cut1_ragged, cut1_last_one    its pieces are equal / the last is shorter / the last is one sub-plane
    cut01            n0 >= 3 and n1 >= 3: a brick with a brick before and behind it along either axis
    L0_2, L1_2       L_a0 = 2, L_a1 = 2: the halo is the brick's only other neighbour
    L1_2_cut         L_a1 = 2 and cut: each sub-plane's halo is the other sub-plane
    lead1, mid1      a lattice axis of extent 1 before a0 / between a0 and a1
    fast_wide        a1 is the fastest axis and cut into pieces of whole 16-byte units (vec > 1)
    fast_narrow      a1 is the fastest axis, of odd extent, and cut (vec = 1)
    chain            one axis of extent > 1, cut along it
    over_cap         a brick of one sub-plane that is larger than the cap: taken all the same
    lanes_ragged     the sites of some brick are no multiple of the lanes
    sub_wave         a brick of fewer than 64 sites
    wide_team        512 lanes (a brick above 4096 sites)
    lds_raised       the image needs more than the 64 KiB of LDS a launch gets without asking
    default_cap      the case runs with brick_bytes = None"""
import math

import torch

from normflow__amd import _hip

from measure_cases import draw, ref_measure, unpack, worst, U  # noqa: F401  (the tests take them from here)

F32, F64 = torch.float32, torch.float64

FORCED = [((3, 5, 4, 8), 256), ((3, 5, 4, 8), 512), ((4, 6, 8), 64), ((2, 37), 64), ((2, 40), 64), ((5, 2, 6), 48),
          ((5, 2, 6), 24), ((2, 3, 4, 5), 64), ((1, 3, 4, 5), 64), ((3, 1, 4, 8), 64), ((5, 4, 8), 512), ((20012,), 4096)]
FORCED_ROWS = [1, 3]
# one brick of 96 000 B: beyond the 64 KiB of LDS a launch gets without asking
RAISED = [((3, 150, 160), 96 * 1024)]
DEFAULT32 = [(2, 160, 160), (12, 12, 12, 12)]
DEFAULT64 = [(24, 24, 24), (12, 12, 12, 12)]


def cases(dtype):
    """[(lattice, cap, N)]"""
    default = DEFAULT32 if dtype == F32 else DEFAULT64
    return ([(lat, cap, N) for lat, cap in FORCED for N in FORCED_ROWS] + [(lat, cap, 1) for lat, cap in RAISED] +
            [(lat, None, 2) for lat in default])


def case_id(v):
    return f"{'x'.join(map(str, v[0]))}-cap{v[1]}-N{v[2]}"


def pieces(L, e):
    return [min(e, L - s) for s in range(0, L, e)]


def regimes(lattice, cap, dtype):
    """The set of regime names (module docstring) that the case exercises, from the library's plan."""
    p = _hip.measure_tiled_plan(lattice, dtype, cap)
    elem = 4 if dtype == F32 else 8
    a0, a1 = p['axis0'], p['axis1']
    out = set()
    p0 = pieces(lattice[a0], p['e0'])
    p1 = pieces(lattice[a1], p['e1']) if a1 is not None else [1]
    sub = math.prod(lattice) // lattice[a0] // (lattice[a1] if a1 is not None else 1)
    if a1 is None:
        out.add('chain')
    if p['n0'] > 1 and p['n1'] == 1:
        out.add('cut0_only')
        if p['e0'] > 1: out.add('planes')
        if p['e0'] > 1 and p0[-1] < p['e0']: out.add('planes_ragged')
    if p['n1'] >= 2:
        out.add('cut1')
        out.add('cut1_even' if p1[-1] == p['e1'] else 'cut1_ragged')
        if p1[-1] == 1: out.add('cut1_last_one')
        if lattice[a1] == 2: out.add('L1_2_cut')
        if a1 == len(lattice) - 1:
            if p['vec'] > 1: out.add('fast_wide')
            elif lattice[a1] % 2: out.add('fast_narrow')
        if p['e1'] == 1 and sub * elem > (cap if cap is not None else 1 << 62): out.add('over_cap')
    if p['n0'] >= 3 and p['n1'] >= 3: out.add('cut01')
    if lattice[a0] == 2: out.add('L0_2')
    if a1 is not None and lattice[a1] == 2: out.add('L1_2')
    if 1 in lattice[:a0]: out.add('lead1')
    if a1 is not None and 1 in lattice[a0 + 1:a1]: out.add('mid1')
    sites = [n0 * n1 * sub for n0 in p0 for n1 in p1]
    if any(s % p['lanes'] for s in sites): out.add('lanes_ragged')
    if min(sites) < 64: out.add('sub_wave')
    if p['lanes'] == 512: out.add('wide_team')
    if p['lds_bytes'] > 64 * 1024: out.add('lds_raised')
    if cap is None: out.add('default_cap')
    return out


ALL_REGIMES = {'cut0_only', 'planes', 'planes_ragged', 'cut1', 'cut1_even', 'cut1_ragged', 'cut1_last_one', 'cut01', 'L0_2',
               'L1_2', 'L1_2_cut', 'lead1', 'mid1', 'fast_wide', 'fast_narrow', 'chain', 'over_cap', 'lanes_ragged',
               'sub_wave', 'wide_team', 'lds_raised', 'default_cap'}

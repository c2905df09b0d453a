"""Shared by tests/test_cluster_modes_host.py and tests/test_cluster_modes.py: the numpy restatement of the cluster modes,
written from the rule in include/normflow_hip.h ("cluster modes", which extends "cluster-improved estimators") with
np.rint, np.add.at on int64 and a long-double reference of the sums of squares -- none of the package's code -- and the
case lists.  The fixed point, the fields, the label kinds and the bound are those of tests/improved_cases.py:
(V + 8) 2^-53 sum |terms| covers every column (a column of two sums of squares is a sum of at most 2 V terms taken as two
sums of V and one more addition)."""
import math

import numpy as np

import improved_cases as Ic

DTYPES = Ic.DTYPES
CHAINS = (1, 3, 300)
HOST_LATTICES = [(8,), (3, 5), (5, 7, 3), (16, 16), (1, 2, 16), (2, 2, 2, 2), (8, 8, 8, 8)]
# lattice -> what it is there for (the issue's table); (24, 24, 24) runs in fp32 only
GPU_LATTICES = [(8,), (3, 5), (5, 7, 3), (16, 16), (1, 2, 16), (2, 2, 2, 2), (16, 16, 16), (8, 8, 8, 8)]
F32_ONLY = [(24, 24, 24)]
POW2_RATIO = [(8,), (16, 16), (1, 2, 16), (2, 2, 2, 2), (16, 16, 16), (8, 8, 8, 8), (24, 24, 24)]     # N / L_mu a power of two


def lcm(lat):
    """N: the lcm of the extents > 1 (1 if there is none)."""
    N = 1
    for n in lat:
        N = N * n // math.gcd(N, n)
    return N


def twiddles(lat):
    """(N, 2): (cos, sin)(2 pi j / N), as the header describes the table."""
    N = lcm(lat)
    return np.array([(math.cos(2.0 * math.pi * j / N), math.sin(2.0 * math.pi * j / N)) for j in range(N)], dtype=np.float64)


def reduce(lat, modes):
    return tuple(tuple(int(n) % L for n, L in zip(m, lat)) for m in modes)


def self_conjugate(lat, m):
    return all((2 * n) % L == 0 for n, L in zip(m, lat))


def quantities(lat, modes):
    """Q = 1 + sum_n (2 - [n self-conjugate])."""
    return 1 + sum(1 if self_conjugate(lat, m) else 2 for m in reduce(lat, modes))


def table(lat, modes):
    """The quantity table of the rule, enumerated: one row per quantity, (m_0 .. m_3 padded, component, column, R without
    I, place in the list); row 0 is zero but for the row length 2 + P."""
    N, pad = lcm(lat), 4 - len(lat)
    rows = [[0] * 7 + [2 + len(modes)]]
    for p, m in enumerate(reduce(lat, modes)):
        ms = [0] * pad + [n * (N // L) for n, L in zip(m, lat)]
        sc = self_conjugate(lat, m)
        rows.append(ms + [0, 2 + p, int(sc), p])
        if not sc:
            rows.append(ms + [1, 2 + p, 0, p])
    return np.array(rows, dtype=np.int32)


def per_pass(lat, modes):
    return min(quantities(lat, modes), 16, (160 * 1024 - 4096) // (8 * Ic.volume(lat)))


def r_ends_a_pass(lat, modes):
    """True if some R whose I follows is the last quantity of a pass: the carry slot is used."""
    t, pp = table(lat, modes), per_pass(lat, modes)
    return any(q % pp == pp - 1 and t[q, 4] == 0 and t[q, 6] == 0 for q in range(1, len(t)))


def mode_lists(lat):
    """name -> momentum list: every column-writing branch of the kernel (the host test holds each list to its purpose).
      zero_first   starts with the zero momentum (an R without I right after A)
      corner_mid   a Nyquist corner in the middle, which shifts the R / I parity of what follows
      negative     negative components (reduced mod L)
      mixed        on-axis and generic off-axis entries, with a repeated momentum
      carry        a length at which an R is the last quantity of a pass"""
    d = len(lat)
    axes = [a for a in range(d) if lat[a] > 1]
    unit = lambda a, k=1: tuple(k if b == a else 0 for b in range(d))
    diag = tuple(1 if lat[b] > 1 else 0 for b in range(d))
    skew = tuple(((b + 2) % lat[b]) if lat[b] > 1 else 0 for b in range(d))
    corner = tuple(lat[b] // 2 if lat[b] % 2 == 0 and lat[b] > 1 else 0 for b in range(d))
    neg = tuple(-(b + 1) if lat[b] > 1 else 0 for b in range(d))
    lists = {
        'zero_first': [(0,) * d, diag, unit(axes[0])],
        'corner_mid': [diag, corner, skew, unit(axes[-1])],
        'negative': [neg, tuple(-n for n in diag), tuple(n - L if L > 1 else 0 for n, L in zip(diag, lat))],
        'mixed': [unit(a) for a in axes] + [diag, skew, unit(axes[0], 2), diag],
    }
    # an R at the end of a pass: general momenta until the quantity at a pass boundary is an R with an I to come
    pp = min(16, (160 * 1024 - 4096) // (8 * Ic.volume(lat)))
    general = [m for m in (diag, skew, unit(axes[-1]), neg) if not self_conjugate(lat, reduce(lat, [m])[0])]
    if general:
        carry = []
        while not (len(carry) >= 2 and r_ends_a_pass(lat, carry)) and len(carry) < 2 * pp + 2:
            carry.append(general[len(carry) % len(general)])
        if r_ends_a_pass(lat, carry):
            lists['carry'] = carry
    return lists


def restate(phi, labels, lat, tw, modes):
    """phi (C, V) float32 / float64, labels (C, V) integers, tw (N, 2) from `twiddles`, modes a list of integer vectors ->
    dict(status (C) int32, out (C, 2 + P) long double, bound (same shape) float64, slots: per momentum (R, I or None)
    int64 arrays, modes reduced).  A refused chain: status 1 and a NaN row."""
    C, V = phi.shape
    N = lcm(lat)
    assert V == Ic.volume(lat) and labels.shape == phi.shape and tw.shape == (N, 2)
    red = reduce(lat, modes)
    x = phi.astype(np.float64)
    lab = labels.astype(np.int64)
    with np.errstate(invalid='ignore'):
        bad = (~(np.abs(x) < Ic.limit(V))).any(axis=1) | (lab < 0).any(axis=1) | (lab >= V).any(axis=1)
    x = np.where(bad[:, None], 0.0, x)
    lab = np.where(bad[:, None], 0, lab)
    rows = np.repeat(np.arange(C), V)

    def slots_of(w):
        s = np.zeros((C, V), dtype=np.int64)
        np.add.at(s, (rows, lab.reshape(-1)), Ic.fixed(w).reshape(-1))
        return s

    A = slots_of(x)
    a2, terms = Ic.sums_of_squares(A)
    t4 = terms * terms
    out, mag = [a2, t4.sum(axis=1)], [np.abs(terms).sum(axis=1), t4.sum(axis=1)]
    coords = np.stack(np.unravel_index(np.arange(V), lat), axis=0).astype(np.int64)          # (d, V)
    slots = []
    for m in red:
        j = np.zeros(V, dtype=np.int64)
        for a, (n, L) in enumerate(zip(m, lat)):
            j += (n * (N // L)) * coords[a]
        t = tw[j % N]
        R = slots_of(x * t[None, :, 0])
        r2, tr = Ic.sums_of_squares(R)
        if self_conjugate(lat, m):                       # the sine quantity is left out
            out.append(r2)
            mag.append(tr.sum(axis=1))
            slots.append((R, None))
        else:
            I = slots_of(x * t[None, :, 1])
            i2, ti = Ic.sums_of_squares(I)
            out.append(r2 + i2)
            mag.append(tr.sum(axis=1) + ti.sum(axis=1))
            slots.append((R, I))
    out = np.stack(out, axis=1)
    out[bad] = np.nan
    bound = ((V + 8) * 2.0 ** -53 * np.stack(mag, axis=1)).astype(np.float64)
    return dict(status=bad.astype(np.int32), out=out, bound=bound, slots=slots, A=A, modes=red)


def check_against(name, got_out, got_status, ref, report=None):
    """A wrapper's out and status against `restate`: status bit for bit, the doubles within the bound."""
    assert np.array_equal(got_status, ref['status']), (name, got_status, ref['status'])
    assert got_out.shape == ref['out'].shape, (name, got_out.shape, ref['out'].shape)
    good = ref['status'] == 0
    assert np.isnan(got_out[~good]).all(), name
    if not good.any():
        return 0.0
    err = np.abs(got_out[good].astype(np.longdouble) - ref['out'][good]).astype(np.float64)
    bound = ref['bound'][good]
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print(f"{name}: max error / bound = {ratio:.3f}")
    if report is not None:
        k = np.unravel_index(np.argmax(err / np.maximum(bound, 1e-300)), err.shape)
        report(name, 'cluster modes', err[k], bound[k])
    assert (err <= bound).all(), (name, ratio)
    return ratio


def tile(ref, chains):
    """The restatement of `chains` rows that repeat the rows of `ref` in a cycle."""
    idx = np.arange(chains) % ref['out'].shape[0]
    return dict(status=ref['status'][idx], out=ref['out'][idx], bound=ref['bound'][idx], modes=ref['modes'])


def host_labels(lat, dt, chains, sweep, seed=0):
    """(phi, labels) (chains, V): chain i gets the label kind i % 6 of `improved_cases.KINDS`; the two sweep kinds are
    `sweep`'s (mcmc.cluster.cluster_sweep) on CPU tensors from torch's generator, at kappa = 0.67 and 0.25."""
    import spectrum_cases as Sc
    return Sc.host_labels(lat, dt, chains, sweep, seed)


def direct_mode_correlator(phi, labels, lat, axis, spatial):
    """(C, L): (L / V^2) sum_C sum_s Re(A~_C(s)^* A~_C(s + t)) in double, A~_C(s) = sum over the sites of C in slice s of
    phi e^{i p x} over the other axes: a scatter over (label, slice), the definition the cosine sum is held against, in
    `Measurement.correlator`'s normalisation."""
    C, V = phi.shape
    L = lat[axis]
    coords = np.stack(np.unravel_index(np.arange(V), lat), axis=0)
    others = [a for a in range(len(lat)) if a != axis]
    phase = np.zeros(V)
    for a, n in zip(others, spatial):
        phase += 2.0 * np.pi * n * coords[a] / lat[a]
    w = phi.astype(np.float64) * np.exp(1j * phase)[None, :]
    A = np.zeros((C, V, L), dtype=np.complex128)
    np.add.at(A, (np.repeat(np.arange(C), V), labels.reshape(-1).astype(np.int64), np.tile(coords[axis], C)), w.reshape(-1))
    return np.stack([(np.conj(A) * np.roll(A, -t, axis=2)).sum(axis=(1, 2)).real for t in range(L)], axis=1) * (L / float(V) ** 2)

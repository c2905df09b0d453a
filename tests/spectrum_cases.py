"""Shared by tests/test_cluster_spectrum_host.py and tests/test_cluster_spectrum.py: the numpy restatement of the cluster
spectrum, written from the rule in include/normflow_hip.h ("cluster spectrum", which extends "cluster-improved
estimators") with np.rint, np.add.at on int64 and a long-double reference of the sums of squares -- none of the package's
code -- and the case lists.  The fixed point, the twiddle table, the fields and the label kinds are those of
tests/improved_cases.py, and so is the bound: (V + 8) 2^-53 sum |terms| covers every column (a column of two sums of
squares is a sum of at most 2 V terms taken as two sums of V and one more addition)."""
import numpy as np

import improved_cases as Ic

DTYPES = Ic.DTYPES
HOST_LATTICES = [(8,), (3, 5), (16, 16), (5, 7, 3), (1, 2, 16), (2, 2, 2, 2), (8, 8, 8, 8)]
GPU_LATTICES = [(8,), (3, 5), (16, 16), (5, 7, 3), (1, 2, 16), (2, 2, 2, 2), (16, 16, 16), (8, 8, 8, 8)]
MOMENTA = (1, 3, 'all')
CHAINS = (1, 3, 300)
CAPS = [((24, 24, 24), 'float32'), ((128, 128), 'float32'), ((64, 128), 'float64')]         # momenta = 2, C = 3
# (lattice, dtype, momenta) -> (Q, per_pass, passes) of nf_cluster_spectrum_plan: per_pass = min(Q, 16, (160 KiB - 4 KiB)
# // 8 V), passes = ceil(Q / per_pass).  (16, 16) has Q = 31 and 156 KiB / 2 KiB = 78 arrays fit, so the formula gives
# 16 per pass and 2 passes
PLAN = {
    ((16, 16), 'float32', 'all'): (31, 16, 2), ((16, 16, 16), 'float32', 'all'): (46, 4, 12),
    ((8, 8, 8, 8), 'float32', 'all'): (29, 4, 8), ((3, 5), 'float64', 'all'): (7, 7, 1),
    ((2, 2, 2, 2), 'float64', 'all'): (5, 5, 1), ((64,), 'float32', 'all'): (64, 16, 4),
    ((64, 128), 'float64', 2): (9, 2, 5), ((24, 24, 24), 'float32', 2): (13, 1, 13), ((128, 128), 'float32', 2): (9, 1, 9),
}


def momenta_id(m):
    return f"k{m}"


def kmax_of(lat, momenta):
    """K_mu of the axes of `lat`: 0 for an axis of extent 1, else floor(L / 2) ('all') or min(momenta, floor(L / 2))."""
    return tuple(0 if n == 1 else (n // 2 if momenta == 'all' else min(int(momenta), n // 2)) for n in lat)


def quantities(lat, momenta):
    return 1 + sum(2 * K - (1 if K and 2 * K == n else 0) for K, n in zip(kmax_of(lat, momenta), lat))


def column(lat, momenta, axis, k):
    """The column of (axis, k) in the (C, 2 + sum K_mu) row."""
    K = kmax_of(lat, momenta)
    assert 1 <= k <= K[axis]
    return 2 + sum(K[:axis]) + k - 1


def restate(phi, labels, lat, tw, momenta):
    """phi (C, V) float32 / float64, labels (C, V) integers, tw from `improved_cases.twiddles` -> dict(status (C) int32,
    out (C, 2 + sum K_mu) long double, bound (same shape) float64, momenta).  A refused chain: status 1 and a NaN row."""
    C, V = phi.shape
    assert V == Ic.volume(lat) and labels.shape == phi.shape
    K = kmax_of(lat, momenta)
    x = phi.astype(np.float64)
    lab = labels.astype(np.int64)
    with np.errstate(invalid='ignore'):
        bad = (~(np.abs(x) < Ic.limit(V))).any(axis=1) | (lab < 0).any(axis=1) | (lab >= V).any(axis=1)
    x = np.where(bad[:, None], 0.0, x)
    lab = np.where(bad[:, None], 0, lab)
    rows = np.repeat(np.arange(C), V)

    def squares_of(w):
        s = np.zeros((C, V), dtype=np.int64)
        np.add.at(s, (rows, lab.reshape(-1)), Ic.fixed(w).reshape(-1))
        total, terms = Ic.sums_of_squares(s)
        return total, terms

    a2, terms = squares_of(x)
    t4 = terms * terms
    out, mag = [a2, t4.sum(axis=1)], [np.abs(terms).sum(axis=1), t4.sum(axis=1)]
    site = np.arange(V)
    off, stride = 4 - len(lat), V
    for n, Kmu in zip(lat, K):
        stride //= n
        xm = (site // stride) % n
        for k in range(1, Kmu + 1):
            t = tw[off + (k * xm) % n]
            r2, tr = squares_of(x * t[None, :, 0])
            if 2 * k == n:                                # Nyquist: the sine quantity is left out
                out.append(r2)
                mag.append(tr.sum(axis=1))
            else:
                i2, ti = squares_of(x * t[None, :, 1])
                out.append(r2 + i2)
                mag.append(tr.sum(axis=1) + ti.sum(axis=1))
        off += n
    out = np.stack(out, axis=1)
    out[bad] = np.nan
    bound = ((V + 8) * 2.0 ** -53 * np.stack(mag, axis=1)).astype(np.float64)
    return dict(status=bad.astype(np.int32), out=out, bound=bound, momenta=K)


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
        report(name, 'cluster spectrum', err[k], bound[k])
    assert (err <= bound).all(), (name, ratio)
    return ratio


def direct_correlator(phi, labels, lat, axis):
    """(C, L): (L / V^2) sum_C sum_s A_C(s) A_C(s + t) in double from a scatter over (label, slice): the definition the
    spectrum's cosine sum is held against, in `Measurement.correlator`'s normalisation (G = (1 / L) sum_s pbar pbar with
    pbar = S L / V, so the slice sums carry L / V^2; with every site alone it is (L / V^2) sum phi^2 at t = 0)."""
    C, V = phi.shape
    L = lat[axis]
    stride = int(np.prod(lat[axis + 1:], dtype=np.int64))
    xm = (np.arange(V) // stride) % L
    A = np.zeros((C, V, L))
    np.add.at(A, (np.repeat(np.arange(C), V), labels.reshape(-1).astype(np.int64), np.tile(xm, C)),
              phi.astype(np.float64).reshape(-1))
    return np.stack([(A * np.roll(A, -t, axis=2)).sum(axis=(1, 2)) for t in range(L)], axis=1) * (L / float(V) ** 2)


def host_labels(lat, dt, chains, sweep, seed=0):
    """(phi, labels) (chains, V): chain i gets the label kind i % 6 of `improved_cases.KINDS`; the two sweep kinds are
    `sweep`'s (mcmc.cluster.cluster_sweep) on CPU tensors from torch's generator, at kappa = 0.67 and 0.25."""
    import torch
    V = Ic.volume(lat)
    phi = Ic.field(lat, dt, chains, seed=seed)
    phi[0::6] = Ic.field(lat, dt, chains, ordered=True, seed=seed)[0::6]
    labels = np.zeros((chains, V), dtype=np.int32)
    gen = torch.Generator().manual_seed(V + seed)
    for i, kind in enumerate(Ic.KINDS):
        n = len(range(i, chains, 6))
        if n == 0:
            continue
        if kind.startswith('sweep'):
            p = torch.from_numpy(phi[i::6]).reshape((n,) + tuple(lat))
            u = torch.rand((n, V, 4), dtype=torch.float64, generator=gen)
            flip = torch.rand((n, V), dtype=torch.float64, generator=gen) < 0.5
            _, lab, st = sweep(p, 2 * (0.67 if kind == 'sweep67' else 0.25), u, flip)
            assert (st[:, 3] >= 1).all()
            labels[i::6] = lab.reshape(n, V).numpy()
        else:
            labels[i::6] = Ic.synthetic_labels(kind, n, V)
    return phi, labels


def select(ref, lat, momenta):
    """The restatement at `momenta` from the one at 'all': its columns are a subset (a Nyquist column is one either way)."""
    K = kmax_of(lat, momenta)
    cols = [0, 1] + [column(lat, 'all', a, k) for a in range(len(lat)) for k in range(1, K[a] + 1)]
    return dict(status=ref['status'], out=ref['out'][:, cols], bound=ref['bound'][:, cols], momenta=K)


def tile(ref, chains):
    """The restatement of `chains` rows that repeat the rows of `ref` in a cycle."""
    idx = np.arange(chains) % ref['out'].shape[0]
    return dict(status=ref['status'][idx], out=ref['out'][idx], bound=ref['bound'][idx], momenta=ref['momenta'])

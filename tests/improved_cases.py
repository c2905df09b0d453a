"""Shared by tests/test_cluster_improved_host.py and tests/test_cluster_improved.py: the numpy restatement of the
cluster-improved estimators, written from the rule in include/normflow_hip.h ("cluster-improved estimators") with
np.rint, np.add.at on int64 and a long-double reference of the sums of squares -- none of the package's code -- and the
case lists.

The bound: a double sum of n <= V terms, in any order, differs from the exact sum by at most (n - 1) 2^-53 sum |terms|;
the terms themselves carry up to four roundings each (the int64 -> double conversion, a a, and for a^4 the square of
that, the fma's own) and the long-double reference its 2^-64 per operation: (n + 8) 2^-53 sum |terms| with n = V covers
every column.  It is the worst-case bound of tests/test_measure_host.py, widened by the squarings."""
import math

import numpy as np

DTYPES = ('float32', 'float64')
# where the lane map and the pass count change: 1 to 16 sites per lane, 1 to 7 passes, 3 to 9 quantities
LATTICES = [(8,), (3, 5), (16, 16), (5, 7, 3), (1, 2, 16), (2, 2, 2, 2), (16, 16, 16), (8, 8, 8, 8)]
F32_ONLY = [(24, 24, 24), (128, 128)]           # the caps of fp32: 16 sites per lane; (128, 128) is the 128 KiB slot array
F64_ONLY = [(64, 128)]                          # the cap of fp64: 8 sites per lane, two quantities per pass
CASES = ([(lat, dt) for lat in LATTICES for dt in DTYPES] + [(lat, 'float32') for lat in F32_ONLY]
         + [(lat, 'float64') for lat in F64_ONLY])
CHAINS = (1, 3, 300)
KINDS = ('sweep67', 'sweep25', 'zero', 'arange', 'alternate', 'random')
# (sites per lane, lanes, quantities, passes, per pass, LDS bytes) of nf_cluster_moments_plan: 2 KiB of reduction slots and
# per_pass x 8 V bytes of slots, per_pass = min(quantities, (160 KiB - 2 KiB) // 8 V)
PLAN = {
    ((8,), 'float32'): (1, 64, 3, 1, 3, 2048 + 3 * 64), ((3, 5), 'float64'): (1, 64, 5, 1, 5, 2048 + 5 * 120),
    ((16, 16), 'float32'): (1, 256, 5, 1, 5, 2048 + 5 * 2048), ((1, 2, 16), 'float32'): (1, 64, 5, 1, 5, 2048 + 5 * 256),
    ((2, 2, 2, 2), 'float64'): (1, 64, 9, 1, 9, 2048 + 9 * 128), ((4, 4, 8, 16), 'float32'): (2, 1024, 9, 1, 9, 2048 + 9 * 16384),
    ((16, 16, 16), 'float32'): (4, 1024, 7, 2, 4, 2048 + 4 * 32768), ((16, 16, 16), 'float64'): (4, 1024, 7, 2, 4, 2048 + 4 * 32768),
    ((8, 8, 8, 8), 'float32'): (4, 1024, 9, 3, 4, 2048 + 4 * 32768), ((64, 128), 'float64'): (8, 1024, 5, 3, 2, 2048 + 2 * 65536),
    ((24, 24, 24), 'float32'): (16, 896, 7, 7, 1, 2048 + 110592), ((128, 128), 'float32'): (16, 1024, 5, 5, 1, 2048 + 131072),
}
REFUSED = [((129, 128), 'float32'), ((65, 128), 'float64'), ((24, 24, 24), 'float64'), ((32, 32, 32), 'float32')]


def case_id(case):
    return 'x'.join(map(str, case[0])) + '-' + case[1]


def volume(lat):
    return int(np.prod(lat))


def lat4(lat):
    return (1,) * (4 - len(lat)) + tuple(lat)


def limit(V):
    """A site is in range iff |phi| < 2^min(16, 30 - ceil(log2 V))."""
    return 2.0 ** min(16, 30 - math.ceil(math.log2(V)))


def twiddles(lat):
    """(sum of the padded extents, 2): (cos, sin)(2 pi t / L_mu), offsets in axis order, as the header describes the table."""
    return np.array([(math.cos(2.0 * math.pi * t / n), math.sin(2.0 * math.pi * t / n)) for n in lat4(lat) for t in range(n)],
                    dtype=np.float64)


def fixed(w):
    """q(w) = llrint(w 2^32), round half to even."""
    return np.rint(w * 2.0 ** 32).astype(np.int64)


def sums_of_squares(slots):
    """(sum, sum of |terms|) of (slot 2^-32)^2 over the last axis, in long double from the exact integers."""
    a = slots.astype(np.longdouble) * np.longdouble(2.0) ** -32
    t = a * a
    return t.sum(axis=-1), t


def restate(phi, labels, lat, tw):
    """phi (C, V) float32 / float64, labels (C, V) integers, tw from `twiddles` (or the package's table: the kernel uses
    whatever numbers it is given) -> dict(moments (C, V) int64, status (C) int32, out (C, 6) long double, bound (C, 6)
    float64, slots: the list of the per-quantity int64 arrays).  A refused chain: status 1, a NaN row, zero moments."""
    C, V = phi.shape
    L4 = lat4(lat)
    assert V == volume(lat) and labels.shape == phi.shape
    x = phi.astype(np.float64)
    lab = labels.astype(np.int64)
    with np.errstate(invalid='ignore'):
        bad = (~(np.abs(x) < limit(V))).any(axis=1) | (lab < 0).any(axis=1) | (lab >= V).any(axis=1)
    x = np.where(bad[:, None], 0.0, x)
    lab = np.where(bad[:, None], 0, lab)
    rows = np.repeat(np.arange(C), V)

    def slots_of(w):
        s = np.zeros((C, V), dtype=np.int64)
        np.add.at(s, (rows, lab.reshape(-1)), fixed(w).reshape(-1))
        return s

    A = slots_of(x)
    a2, terms = sums_of_squares(A)
    t4 = terms * terms
    out = np.full((C, 6), np.nan, dtype=np.longdouble)
    mag = np.zeros((C, 6), dtype=np.longdouble)
    out[:, 0], mag[:, 0] = a2, np.abs(terms).sum(axis=1)
    out[:, 1], mag[:, 1] = t4.sum(axis=1), t4.sum(axis=1)
    site = np.arange(V)
    off, stride, slots = 0, V, [A]
    for mu, n in enumerate(L4):
        stride //= n
        if n == 1:
            out[:, 2 + mu], mag[:, 2 + mu] = out[:, 0], mag[:, 0]
        else:
            t = tw[off + (site // stride) % n]
            R, I = slots_of(x * t[None, :, 0]), slots_of(x * t[None, :, 1])
            (r2, tr), (i2, ti) = sums_of_squares(R), sums_of_squares(I)
            out[:, 2 + mu], mag[:, 2 + mu] = r2 + i2, tr.sum(axis=1) + ti.sum(axis=1)
            slots += [R, I]
        off += n
    out[bad] = np.nan
    bound = ((V + 8) * 2.0 ** -53 * mag).astype(np.float64)
    return dict(moments=A, status=bad.astype(np.int32), out=out, bound=bound, slots=slots)


def columns(lat):
    """The columns of the (C, 6) row that the wrappers return for the lattice `lat`: (C, 2 + d)."""
    return [0, 1] + [2 + 4 - len(lat) + a for a in range(len(lat))]


def field(lat, dtype, chains, ordered=False, seed=0):
    """(chains, V): Gaussian fields of scale 1.2; `ordered`: around +1, so that a sweep finds one giant cluster."""
    rng = np.random.default_rng(1000 * seed + 7 * volume(lat) + len(lat))
    x = rng.standard_normal((chains, volume(lat)))
    x = 1.0 + 0.3 * x if ordered else 1.2 * x
    return x.astype(dtype)


def synthetic_labels(kind, chains, V, seed=0):
    """(chains, V) int32 of the kinds that need no sweep."""
    if kind == 'zero':
        lab = np.zeros((chains, V))
    elif kind == 'arange':
        lab = np.tile(np.arange(V), (chains, 1))
    elif kind == 'alternate':                     # two keys site by site: the two heaviest slots a chain can have
        lab = np.tile(np.where(np.arange(V) % 2 == 0, V - 1, V // 3), (chains, 1))
    elif kind == 'random':                        # keys that are no roots of anything
        lab = np.random.default_rng(seed + V).integers(0, V, size=(chains, V))
    else:
        raise ValueError(kind)
    return lab.astype(np.int32)


def check_against(name, got_out, got_status, got_moments, ref, lat, report=None):
    """The wrappers' dict against `restate`: status and moments bit for bit, the doubles within the bound."""
    cols = columns(lat)
    assert np.array_equal(got_status, ref['status']), (name, got_status, ref['status'])
    if got_moments is not None:
        assert np.array_equal(got_moments.reshape(ref['moments'].shape), ref['moments']), name
    want, bound = ref['out'][:, cols], ref['bound'][:, cols]
    good = ref['status'] == 0
    assert np.isnan(got_out[~good]).all(), name
    err = np.abs(got_out[good].astype(np.longdouble) - want[good]).astype(np.float64)
    ratio = float((err / np.maximum(bound[good], 1e-300)).max()) if good.any() else 0.0
    print(f"{name}: max error / bound = {ratio:.3f}")
    if report is not None and good.any():
        k = np.unravel_index(np.argmax(err / np.maximum(bound[good], 1e-300)), err.shape)
        report(name, 'improved sums', err[k], bound[good][k])
    assert (err <= bound[good]).all(), (name, ratio)
    return ratio


def sign_average(phi, labels, lat):
    """Brute force: the averages of (sum phi)^2, (sum phi)^4 and |phi~(p_min)|^2 per axis over all 2^Nc sign assignments
    of the clusters of ONE chain phi (V), labels (V), in double.  Returns (m2, m4, [prop per axis of lat])."""
    keys = np.unique(labels)
    assert len(keys) <= 14
    x = phi.astype(np.float64)
    V = x.size
    member = np.stack([(labels == k) for k in keys]).astype(np.float64)           # (Nc, V)
    coords = np.stack(np.unravel_index(np.arange(V), lat), axis=0)               # (d, V)
    phases = [np.exp(2j * np.pi * coords[a] / lat[a]) for a in range(len(lat))]
    M = member @ x                                                               # (Nc)
    Mt = [member @ (x * ph) for ph in phases]
    signs = np.array([[1.0 if (n >> k) & 1 else -1.0 for k in range(len(keys))] for n in range(2 ** len(keys))])
    tot = signs @ M
    return (tot ** 2).mean(), (tot ** 4).mean(), [(np.abs(signs @ m) ** 2).mean() for m in Mt]

"""One Swendsen-Wang sweep of the embedded Ising signs of phi^4 chains (Brower-Tamayo), composed from torch ops: the rule
of include/normflow_hip.h (section "cluster updates") on any device.  `HMCSampler(cluster_every=E)` uses it for CPU
tensors and for the device lattices that neither nf_phi4_cluster nor, by TILED_CLASSES, nf_phi4_cluster_tiled is routed
to; on the device its `u` and `flip` come from nf_phi4_cluster_draws at the positions the kernels would use, so that it
walks the kernels' chain.  `cluster_moments` is the composed path of the cluster-improved estimators (nf_cluster_moments),
`cluster_spectrum` and `cluster_modes` those of nf_cluster_spectrum and nf_cluster_modes."""
import torch

PATHS = (None, 'kernel', 'tiled', 'composed')
# (dtype, axes of extent > 1, least sites of a chain): the classes beyond nf_phi4_cluster on which tools/cluster_bench.py
# --tiled measured nf_phi4_cluster_tiled faster than the composed sweep below by more than its margin on an MI355X: 32^3
# (3 axes) and 16^4, 32^4, 48^4 (4 axes) in both dtypes, 15 to 59 times (README, "Cluster updates").  A class is the
# number of axes and everything from its smallest measured lattice up: the share of links that cross tiles, which is
# what the merge costs, depends on both.  `HMCSampler._sweep_path` sends only these to the tiled kernel; lattices of 1
# or 2 axes and smaller ones of 3 or 4 were not measured and stay composed
TILED_CLASSES = ((torch.float32, 3, 32 ** 3), (torch.float64, 3, 32 ** 3),
                 (torch.float32, 4, 16 ** 4), (torch.float64, 4, 16 ** 4))


def cluster_sweep(phi, w0, u, flip):
    """(new phi, labels (C, *L) int32, stats (C, 4) int32) of one sweep of the chains phi (C, *L), which are left alone.
      u     (C, V, 4) float64 in (0, 1): word mu of site x decides the link (x, mu), mu counted on the lattice padded
            with leading extents 1 to four axes;
      flip  (C, V) bool or uint8: entry rho decides the cluster whose label -- its smallest site index -- is rho.
      w0    a float, or a (C,) float64 tensor with the hopping coefficient of every chain (a coupling ladder);
    Bonds: t = (w0 phi(x)) phi(x + mu) in double, active iff t > 0 and u < -expm1(-2 t); an axis of extent 1 has no link.
    Labels: labels = min(labels, where(bond, rolled labels)) in both directions of every axis, then labels[labels]
    (pointer jumping: it lowers a label to another label of the same cluster), until a round changes nothing; at most V
    rounds, as in the kernel, and a chain set that has not settled by then is returned untouched with rounds = -1.
    stats: clusters, sites flipped, size of the largest cluster, rounds (of the whole call: the chains are labelled
    together).  The loop reads ONE flag per round from the device: the composed sweep synchronises with the host as
    often as it has rounds."""
    C, lat = phi.shape[0], tuple(phi.shape[1:])
    if not 1 <= len(lat) <= 4:
        raise ValueError(f"cluster_sweep: lattices of 1 to 4 axes, got {lat}")
    V = 1
    for n in lat:
        V *= n
    dev = phi.device
    u = u.reshape((C,) + lat + (4,))
    f = phi.double()
    if isinstance(w0, torch.Tensor):
        if w0.dtype != torch.float64 or tuple(w0.shape) != (C,):
            raise ValueError(f"cluster_sweep: a tensor w0 is ({C},) float64, one per chain, got {tuple(w0.shape)} {w0.dtype}")
        w0 = w0.reshape((C,) + (1,) * len(lat))
    labels = torch.arange(V, dtype=torch.int64, device=dev).reshape(lat).expand((C,) + lat).contiguous()
    own = labels.clone()
    bonds = []
    for a, n in enumerate(lat):
        if n == 1:
            continue
        t = (w0 * f) * torch.roll(f, -1, dims=a + 1)
        fw = (t > 0) & (u[..., 4 - len(lat) + a] < -torch.expm1(-2.0 * t))
        bonds.append((a + 1, fw, torch.roll(fw, 1, dims=a + 1)))
    rounds, settled = 0, False
    for _ in range(V):
        new = labels
        for dim, fw, bw in bonds:
            new = torch.minimum(new, torch.where(fw, torch.roll(labels, -1, dims=dim), labels))
            new = torch.minimum(new, torch.where(bw, torch.roll(labels, 1, dims=dim), labels))
        new = new.reshape(C, V)
        new = new.gather(1, new).reshape(labels.shape)
        rounds += 1
        same = bool(torch.equal(new, labels))           # the one read of the round
        labels = new
        if same:
            settled = True
            break
    flat = labels.reshape(C, V)
    if not settled:
        stats = torch.zeros((C, 4), dtype=torch.int32, device=dev)
        stats[:, 3] = -1
        return phi.clone(), labels.to(torch.int32), stats
    flips = flip.reshape(C, V).bool().gather(1, flat)
    out = torch.where(flips.reshape(phi.shape), -phi, phi)
    sizes = torch.zeros((C, V), dtype=torch.int64, device=dev).scatter_add_(1, flat, torch.ones_like(flat))
    stats = torch.stack([(labels == own).reshape(C, V).sum(dim=1), flips.sum(dim=1), sizes.max(dim=1).values,
                         torch.full((C,), rounds, dtype=torch.int64, device=dev)], dim=1).to(torch.int32)
    return out, labels.to(torch.int32), stats


def cluster_moments(phi, labels, want_moments=False):
    """The rule of nf_cluster_moments (include/normflow_hip.h, "cluster-improved estimators") from torch ops, on any
    device and any lattice of 1 to 4 axes with V < 2^31, fp32 / fp64: the dict of `_hip.cluster_moments`, out (C, 2 + d)
    float64, status (C) int32, moments (C, *L) int64 or None.
      q(w) = torch.round(w 2^32) (half to even) as int64; the clusters' sums by scatter_add_ on int64, which is exact on
      every device, so the moments are the kernel's bit for bit; the sums of squares by `sum` in double, which agree with
      the kernel's within rounding.
    A chain with a site out of range (|phi| >= 2^min(16, 30 - ceil(log2 V)), NaN, inf) or a label outside 0 .. V - 1 is
    refused: status 1, a NaN row, a zero moments row; its values never reach an index.  Nothing is read back from the
    device."""
    from .. import _hip
    C, lat = phi.shape[0], tuple(phi.shape[1:])
    if not 1 <= len(lat) <= 4:
        raise ValueError(f"cluster_moments: lattices of 1 to 4 axes, got {lat}")
    if labels.shape != phi.shape:
        raise ValueError(f"cluster_moments: labels {tuple(labels.shape)} do not match phi {tuple(phi.shape)}")
    V = 1
    for n in lat:
        V *= n
    dev = phi.device
    x = phi.double().reshape(C, V)
    lab = labels.reshape(C, V).long()
    bad = (~(x.abs() < _hip.cluster_moments_limit(V)) | (lab < 0) | (lab >= V)).any(dim=1)
    x = torch.where(bad.unsqueeze(1), torch.zeros_like(x), x)
    lab = torch.where(bad.unsqueeze(1), torch.zeros_like(lab), lab)
    q = lambda w: torch.round(w * 2.0 ** 32).to(torch.int64)
    slots = lambda w: torch.zeros((C, V), dtype=torch.int64, device=dev).scatter_add_(1, lab, q(w))
    squares = lambda s: (s.double() * 2.0 ** -32).square().sum(dim=1)
    A = slots(x)
    a2 = (A.double() * 2.0 ** -32).square()
    cols = [a2.sum(dim=1), a2.square().sum(dim=1)]
    tw = _hip.twiddle_table(lat, dev)
    site = torch.arange(V, device=dev)
    off, stride = 4 - len(lat), V
    for n in lat:
        stride //= n
        if n == 1:
            cols.append(cols[0])
        else:
            t = tw[off + (site // stride) % n]              # (V, 2)
            cols.append(squares(slots(x * t[:, 0])) + squares(slots(x * t[:, 1])))
        off += n
    out = torch.stack(cols, dim=1)
    out = torch.where(bad.unsqueeze(1), torch.full_like(out, float('nan')), out)
    moments = A.reshape((C,) + lat) if want_moments else None
    return dict(out=out, status=bad.to(torch.int32), moments=moments)


def cluster_spectrum(phi, labels, momenta='all'):
    """The rule of nf_cluster_spectrum (include/normflow_hip.h, "cluster spectrum") from torch ops, on any device and any
    lattice of 1 to 4 axes with V < 2^31, fp32 / fp64: the dict of `_hip.cluster_spectrum`, out (C, 2 + sum K_mu) float64,
    status (C) int32, momenta (K_mu of the axes).  q, the int64 scatter_add_ and the `sum` in double are those of
    `cluster_moments`, on the same twiddle table: columns 0 and 1 and every k = 1 column are its bits.  The sine
    quantity at the Nyquist momentum is left out, as in the kernel.  Nothing is read back from the device."""
    from .. import _hip
    C, lat = phi.shape[0], tuple(phi.shape[1:])
    if not 1 <= len(lat) <= 4:
        raise ValueError(f"cluster_spectrum: lattices of 1 to 4 axes, got {lat}")
    if labels.shape != phi.shape:
        raise ValueError(f"cluster_spectrum: labels {tuple(labels.shape)} do not match phi {tuple(phi.shape)}")
    K = _hip.spectrum_momenta(lat, momenta)
    V = 1
    for n in lat:
        V *= n
    dev = phi.device
    x = phi.double().reshape(C, V)
    lab = labels.reshape(C, V).long()
    bad = (~(x.abs() < _hip.cluster_moments_limit(V)) | (lab < 0) | (lab >= V)).any(dim=1)
    x = torch.where(bad.unsqueeze(1), torch.zeros_like(x), x)
    lab = torch.where(bad.unsqueeze(1), torch.zeros_like(lab), lab)
    q = lambda w: torch.round(w * 2.0 ** 32).to(torch.int64)
    slots = lambda w: torch.zeros((C, V), dtype=torch.int64, device=dev).scatter_add_(1, lab, q(w))
    squares = lambda s: (s.double() * 2.0 ** -32).square().sum(dim=1)
    a2 = (slots(x).double() * 2.0 ** -32).square()
    cols = [a2.sum(dim=1), a2.square().sum(dim=1)]
    tw = _hip.twiddle_table(lat, dev)
    site = torch.arange(V, device=dev)
    off, stride = 4 - len(lat), V
    for n, Kmu in zip(lat, K):
        stride //= n
        xm = (site // stride) % n
        for k in range(1, Kmu + 1):
            t = tw[off + (k * xm) % n]                      # (V, 2)
            col = squares(slots(x * t[:, 0]))
            cols.append(col if 2 * k == n else col + squares(slots(x * t[:, 1])))
        off += n
    out = torch.stack(cols, dim=1)
    out = torch.where(bad.unsqueeze(1), torch.full_like(out, float('nan')), out)
    return dict(out=out, status=bad.to(torch.int32), momenta=K)


def cluster_modes(phi, labels, modes):
    """The rule of nf_cluster_modes (include/normflow_hip.h, "cluster modes") from torch ops, on any device and any
    lattice of 1 to 4 axes with V < 2^31 and N = lcm of the extents in 2 .. 65536, fp32 / fp64: the dict of
    `_hip.cluster_modes`, out (C, 2 + P) float64, status (C) int32, modes (the momenta reduced to 0 .. L_mu - 1).  q, the
    int64 scatter_add_ and the `sum` in double are those of `cluster_moments`; the phase index
    j(x) = (sum_mu m_mu x_mu) mod N, m_mu = (n_mu mod L_mu) (N / L_mu), is taken in int64 arithmetic on the table
    `_hip.mode_twiddle_table`.  The integer sums are the kernel's bit for bit, the doubles agree within rounding.  The
    sine quantity of a self-conjugate momentum (2 n_mu = 0 mod L_mu on every axis) is left out, as in the kernel.  Nothing
    is read back from the device."""
    from .. import _hip
    C, lat = phi.shape[0], tuple(phi.shape[1:])
    if not 1 <= len(lat) <= 4:
        raise ValueError(f"cluster_modes: lattices of 1 to 4 axes, got {lat}")
    if labels.shape != phi.shape:
        raise ValueError(f"cluster_modes: labels {tuple(labels.shape)} do not match phi {tuple(phi.shape)}")
    try:
        reduced = _hip.modes_reduced(lat, modes)
    except _hip.NormflowHipError as e:
        raise ValueError(f"cluster_modes: {e}") from None
    if len(reduced) > _hip.MODES_MAX:
        raise ValueError(f"cluster_modes: at most {_hip.MODES_MAX} momenta in one call, got {len(reduced)}")
    for m, given in zip(reduced, _hip.modes_list(lat, modes)):
        if any(L == 1 and n != 0 for n, L in zip(given, lat)):
            raise ValueError(f"cluster_modes: momentum {given}: a non-zero component on an axis of extent 1 of {lat}")
    N = _hip.modes_lcm(lat)
    if not 2 <= N <= _hip.MODES_MAX_N:
        raise ValueError(f"cluster_modes: N, the lcm of the extents of {lat}, is {N}: it must be in 2 .. {_hip.MODES_MAX_N}")
    V = 1
    for n in lat:
        V *= n
    dev = phi.device
    x = phi.double().reshape(C, V)
    lab = labels.reshape(C, V).long()
    bad = (~(x.abs() < _hip.cluster_moments_limit(V)) | (lab < 0) | (lab >= V)).any(dim=1)
    x = torch.where(bad.unsqueeze(1), torch.zeros_like(x), x)
    lab = torch.where(bad.unsqueeze(1), torch.zeros_like(lab), lab)
    q = lambda w: torch.round(w * 2.0 ** 32).to(torch.int64)
    slots = lambda w: torch.zeros((C, V), dtype=torch.int64, device=dev).scatter_add_(1, lab, q(w))
    squares = lambda s: (s.double() * 2.0 ** -32).square().sum(dim=1)
    a2 = (slots(x).double() * 2.0 ** -32).square()
    cols = [a2.sum(dim=1), a2.square().sum(dim=1)]
    tw = _hip.mode_twiddle_table(lat, dev)
    site = torch.arange(V, dtype=torch.int64, device=dev)
    coords, stride = [], V
    for n in lat:
        stride //= n
        coords.append((site // stride) % n)
    for m in reduced:
        j = torch.zeros_like(site)
        for n, L, xm in zip(m, lat, coords):
            j = j + (n * (N // L)) * xm
        t = tw[j % N]                                       # (V, 2)
        col = squares(slots(x * t[:, 0]))
        cols.append(col if all((2 * n) % L == 0 for n, L in zip(m, lat)) else col + squares(slots(x * t[:, 1])))
    out = torch.stack(cols, dim=1)
    out = torch.where(bad.unsqueeze(1), torch.full_like(out, float('nan')), out)
    return dict(out=out, status=bad.to(torch.int32), modes=reduced)

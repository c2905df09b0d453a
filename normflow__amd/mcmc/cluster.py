"""One Swendsen-Wang sweep of the embedded Ising signs of phi^4 chains (Brower-Tamayo), composed from torch ops: the rule
of include/normflow_hip.h (section "cluster updates") on any device.  `HMCSampler(cluster_every=E)` uses it for CPU
tensors and for the device lattices that neither nf_phi4_cluster nor, by TILED_CLASSES, nf_phi4_cluster_tiled is routed
to; on the device its `u` and `flip` come from nf_phi4_cluster_draws at the positions the kernels would use, so that it
walks the kernels' chain."""
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

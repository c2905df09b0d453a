"""Lattice phi^4 action, the target density of the flow (API of src/action/scalar_action.py).

    S[phi] = sum_x ( w2 phi^2 + w4 phi^4 ) - w0 sum_mu sum_x phi(x) phi(x - mu)        (periodic)
with w0 = kappa a^(d-2), w2 = (m^2 a^d + 2 d kappa a^(d-2)) / 2, w4 = lambda a^d.
On the device the whole thing is one pass of the `nf_phi4_action` kernel (with its VJP); the per-site
`action_density` is one pass of `nf_phi4_action_density`.
"""
import torch

from .. import _hip


class ScalarPhi4Action:

    def __init__(self, *, m_sq, lambd, kappa=1, a=1):
        self.m_sq, self.lambd, self.kappa, self.a = m_sq, lambd, kappa, a

    def get_coef(self, lat_ndim):
        """(w0, w2, w4) for a `lat_ndim`-dimensional lattice."""
        hop = self.kappa * self.a ** (lat_ndim - 2)
        vol = self.a ** lat_ndim
        return hop, (self.m_sq * vol + 2 * lat_ndim * hop) / 2, self.lambd * vol

    def action(self, cfgs):
        """(B, *L) configurations -> (B,) actions."""
        d = cfgs.ndim - 1
        w0, w2, w4 = self.get_coef(d)
        if d >= 1 and cfgs.numel() and _hip.endpoint_supported(cfgs):
            # An axis of extent 1 is its own neighbour: roll is the identity there and the hopping term is -w0 phi(x)^2.
            # The kernel takes extents of 1 as the padding of a lattice of fewer than four axes and reads no neighbour
            # along them, so that term goes into the site-local coefficient.
            own = sum(1 for n in cfgs.shape[1:] if n == 1)
            return _hip.Phi4ActionFn.apply(cfgs, float(w0), float(w2 - own * w0), float(w4))
        # host tensors: site-local part, then one nearest-neighbour product per direction
        flat = lambda t: t.flatten(1).sum(dim=1) if d >= 1 else t
        sq = cfgs.square()
        total = flat(sq * (w2 + w4 * sq))
        for mu in range(1, d + 1):
            total = total - w0 * flat(cfgs * cfgs.roll(1, dims=mu))
        return total

    __call__ = action

    def action_density(self, cfgs):
        """(B, *L) configurations -> (B, *L) per-site action (reference: scalar_action.py:48-62): the symmetric density
        with a non-negative kinetic term,
            s(x) = wm phi^2 + w4 phi^4 + (w0 / 4) sum_mu [(phi(x) - phi(x + mu))^2 + (phi(x) - phi(x - mu))^2],
        wm = w2 - d w0 (= m^2 a^d / 2).  Its sites sum to `action`.  On the device one `nf_phi4_action_density` pass."""
        d = cfgs.ndim - 1
        w0, w2, w4 = self.get_coef(d)
        wm = w2 - w0 * d
        if d >= 1 and cfgs.numel() and _hip.endpoint_supported(cfgs):
            return _hip.Phi4ActionDensityFn.apply(cfgs, float(w0), float(wm), float(w4))
        # host tensors: the reference's formula, one roll per direction and sign
        dens = wm * cfgs ** 2 + w4 * cfgs ** 4
        for mu in range(1, d + 1):
            dens = dens + (w0 / 4) * (cfgs - cfgs.roll(-1, dims=mu)) ** 2
            dens = dens + (w0 / 4) * (cfgs - cfgs.roll(1, dims=mu)) ** 2
        return dens

    def potential(self, x):
        return self.m_sq * x ** 2 + self.lambd * x ** 4

    def log_prob(self, x, action_logz=0):
        """log density up to the constant `action_logz`."""
        return -self.action(x) - action_logz


class ScalarPhi4Ladder:
    """K phi^4 actions that differ in their couplings: the rungs of a coupling ladder (MI355X-side extension, for
    `model.hmc.ladder`).  Each of m_sq, lambd, kappa, a is a scalar (the same on every rung) or a sequence of length K.
    `len(ladder)` is K, `ladder.rung(k)` the ScalarPhi4Action of rung k, `ladder.coef_table(lattice, device)` the (K, 3)
    float64 table (w0, w2, w4) that the ladder kernels take, and `ladder.action(cfgs, rung)` the action of every row under
    its own rung."""

    _NAMES = ('m_sq', 'lambd', 'kappa', 'a')

    def __init__(self, *, m_sq, lambd, kappa=1, a=1):
        given = dict(m_sq=m_sq, lambd=lambd, kappa=kappa, a=a)
        seqs = {}
        for name, v in given.items():
            if torch.is_tensor(v):
                v = v.tolist()
            if isinstance(v, (list, tuple)):
                seqs[name] = [float(x) for x in v]
        lengths = {len(v) for v in seqs.values()}
        if len(lengths) > 1 or 0 in lengths:
            raise ValueError("ScalarPhi4Ladder: the sequences among m_sq, lambd, kappa, a must share one length K >= 1, got "
                             + ", ".join(f"{n}: {len(v)}" for n, v in seqs.items()))
        self._K = lengths.pop() if lengths else 1
        for name in self._NAMES:
            setattr(self, name, seqs.get(name, [given[name]] * self._K))

    def __len__(self):
        return self._K

    def rung(self, k):
        k = int(k)
        if not 0 <= k < self._K:
            raise IndexError(f"rung {k} of a ladder of {self._K}")
        return ScalarPhi4Action(**{name: getattr(self, name)[k] for name in self._NAMES})

    def get_coef(self, lat_ndim):
        """[(w0, w2, w4)] per rung for a `lat_ndim`-dimensional lattice: ScalarPhi4Action.get_coef of every rung."""
        return [self.rung(k).get_coef(lat_ndim) for k in range(self._K)]

    def coef_table(self, lattice, device=None):
        """(K, 3) float64 on `device`: (w0, w2, w4) per rung as the HMC kernels take them -- ScalarPhi4Action.action's
        rule for a user axis of extent 1 (it is its own neighbour: -w0 phi^2) folded into w2."""
        own = sum(1 for n in lattice if n == 1)
        rows = [(float(w0), float(w2 - own * w0), float(w4)) for w0, w2, w4 in self.get_coef(len(lattice))]
        return torch.tensor(rows, dtype=torch.float64, device=device)

    def action(self, cfgs, rung):
        """(B, *L) configurations and their rungs (B) -> (B,) actions: row b under the couplings of rung[b].  The host
        formula of ScalarPhi4Action.action from torch ops on any device, with the coefficients broadcast per row: it is
        differentiable in cfgs, so the composed HMC path takes its force from it."""
        d = cfgs.ndim - 1
        rung = torch.as_tensor(rung, device=cfgs.device).long()
        table = torch.tensor(self.get_coef(d), dtype=torch.float64, device=cfgs.device).to(cfgs.dtype)
        w = table[rung].reshape((cfgs.shape[0], 3) + (1,) * d)
        w0, w2, w4 = table[rung][:, 0], w[:, 1], w[:, 2]       # w0 multiplies the rows' link sums, w2 and w4 the sites
        flat = lambda t: t.flatten(1).sum(dim=1) if d >= 1 else t
        sq = cfgs.square()
        total = flat(sq * (w2 + w4 * sq))
        for mu in range(1, d + 1):
            total = total - w0 * flat(cfgs * cfgs.roll(1, dims=mu))
        return total

    __call__ = action

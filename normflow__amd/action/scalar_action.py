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

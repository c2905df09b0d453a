"""Site-local Jacobian-tracking modules (reference: src/nn/scalar/modules_.py).

Expit_, SplineNet_, Logit_ and their composition DistConvertor_ run on the fused K4
kernel (`nf_distconv`): one pass over the field for any subset of the three stages,
the shared spline's knots staged in LDS.  DistConvertor_ keeps the reference's list
structure (so `1.weights_x`-style state_dict keys and `.spline_layer_` still work) but
executes the whole Expit_ -> SplineNet_ -> Logit_ triple as ONE launch.  With
propagate_density (on the instance or on the class) the same pass writes per-site
log-densities (`nf_distconv_sites`), in inference and in training.  Pade11_,
Pade22_, Pade32_, Tanh_ and ArcTanh_ run on `nf_pade`: one pass per direction,
per-site densities included.
"""
import math

import torch

from .modules import SplineNet, softplus_ln2
from .._core import Module_, ModuleList_
from ... import _hip


def _as_rows(x):
    """(B, V) view of a field whose axis 0 is the batch."""
    return x.reshape(x.shape[0], -1) if x.dim() > 1 else x.reshape(-1, 1)


def _site_log0(log0, x):
    """A per-site log0 as a (B, V) tensor (None for the number 0), broadcast against the field as the reference's
    `log0 + logJ` does."""
    if torch.is_tensor(log0):
        return log0.to(x.dtype).expand(x.shape).reshape(x.shape[0], -1).contiguous()
    return None if log0 == 0 else torch.full((x.shape[0], x[0].numel()), float(log0), dtype=x.dtype, device=x.device)


def _run_stages(per_site, x, log0, stages, inverse, knots=None, mask=None):
    """One K4 pass.  per_site (Module_.propagate_density): log0 + log|f'| at every site, shaped like x (nf_distconv_sites);
    otherwise the per-sample sum on the summed kernel (nf_distconv).  With an activity `mask` (V uint8 bytes: the
    invisibility wrapper) the masked pass of nf_distconv_sites in either mode."""
    v = _as_rows(x)
    if per_site:
        val, dens = _hip.DistConvSitesFn.apply(v, knots, _site_log0(log0, x), mask, stages, inverse, True)
        return val.reshape(x.shape), dens.reshape(x.shape)
    l0 = _hip._log0_tensor(log0, v, v.shape[0])
    if mask is not None:
        val, lj = _hip.DistConvSitesFn.apply(v, knots, l0, mask, stages, inverse, False)
    else:
        val, lj = _hip.DistConvFn.apply(v, knots, l0, stages, inverse)
    return val.reshape(x.shape), lj


class _K4Leaf:
    """A leaf that runs on K4: `_k4(inverse)` gives its (stages, inverse, knots) for nf_distconv(_sites); the invisibility
    wrapper reads it to run the whole wrapped module as one masked pass."""

    def _k4(self, inverse):
        raise NotImplementedError

    def forward(self, x, log0=0):
        return _run_stages(self.propagate_density, x, log0, *self._k4(False))

    def backward(self, x, log0=0):
        return _run_stages(self.propagate_density, x, log0, *self._k4(True))


class Identity_(Module_):
    def __init__(self, label='identity_'):
        super().__init__(label=label)

    def forward(self, x, log0=0, **extra):
        return x, log0

    def backward(self, x, log0=0, **extra):
        return x, log0


class Clone_(Module_):
    def __init__(self, label='clone_'):
        super().__init__(label=label)

    def forward(self, x, log0=0, **extra):
        return x.clone(), log0

    def backward(self, x, log0=0, **extra):
        return x.clone(), log0


class ScaleNet_(Module_):
    """x -> x * softplus_ln2(w), w a single learned logit; log|J| = V log(weight)
    (modules_.py:44-69)."""

    def __init__(self, label='scale_'):
        super().__init__(label=label)
        self._weight = torch.nn.Parameter(torch.zeros(1))

    @property
    def weight(self):
        return softplus_ln2(self._weight)

    def _logj(self, x):
        per_site = torch.log(self.weight)
        if self.propagate_density:
            return per_site.expand(x.shape)
        return (per_site * math.prod(x.shape[1:])).expand(x.shape[0])

    def forward(self, x, log0=0):
        return x * self.weight, log0 + self._logj(x)

    def backward(self, x, log0=0):
        return x / self.weight, log0 - self._logj(x)


class Expit_(_K4Leaf, Module_):
    """y = 1/(1+e^-x); log|J| = sum(-x + 2 log y) (modules_.py:93-102); with propagate_density the per-site terms.
    Unlike the reference, whose backward builds a fresh Logit_ that ignores this instance's flag (modules_.py:101-102),
    the flag holds in both directions."""

    def _k4(self, inverse):
        return (_hip.STAGE_LOGIT if inverse else _hip.STAGE_EXPIT), False, None


class Logit_(_K4Leaf, Module_):
    """y = log(x/(1-x)); log|J| = -sum log(x(1-x)) (modules_.py:105-114); with propagate_density the per-site terms.
    The instance's flag holds in both directions (the reference's backward is a fresh Expit_, modules_.py:113-114)."""

    def _k4(self, inverse):
        return (_hip.STAGE_EXPIT if inverse else _hip.STAGE_LOGIT), False, None


def _pade(module, x, log0, kind, inverse, d0, d1):
    """One nf_pade pass over x: the field is described to the kernel as (outer, C, inner) around the channel axis, with
    no copy; the per-channel parameters go in already mapped (autograd takes the chain through softplus_ln2 or expit).
    A module without `n_channels` (Tanh_, ArcTanh_) has no parameters: d0 and d1 are None."""
    _hip._require_device(x)
    C = getattr(module, 'n_channels', 1)
    if C == 1:
        B = x.shape[0] if x.dim() > 0 else 1
        layout = (B, B, 1, x.numel() // B if B else 0)
    else:
        axis = module.channels_axis % x.dim()
        if x.shape[axis] != C:
            raise ValueError(f"{type(module).__name__}: axis {module.channels_axis} of a {tuple(x.shape)} field has "
                             f"{x.shape[axis]} entries, not n_channels={C}")
        layout = (x.shape[0], math.prod(x.shape[:axis]), C, math.prod(x.shape[axis + 1:]))
    d0 = d0.to(x.dtype) if d0 is not None else None
    d1 = d1.to(x.dtype) if d1 is not None else None
    per_site = module.propagate_density
    if per_site:
        l0 = (log0.to(x.dtype).expand(x.shape).contiguous() if torch.is_tensor(log0)
              else None if log0 == 0 else torch.full_like(x, float(log0)))
    else:
        l0 = _hip._log0_tensor(log0, x, layout[0])
    return _hip.PadeFn.apply(x, d0, d1, l0, kind, inverse, per_site, layout)


class Pade11_(Module_):
    """y = x / (x + d (1 - x)) = expit(logit(x) - log d), d = softplus_ln2(w1) per channel: a monotone map of [0, 1]
    onto itself; the inverse is the same map with 1/d (modules_.py:117-163).  One nf_pade pass per direction; with
    propagate_density the per-site log-derivatives, in inference and in training."""

    def __init__(self, n_channels=1, channels_axis=1, label='pade11'):
        super().__init__(label=label)
        self.w1 = torch.nn.Parameter(torch.zeros(n_channels))
        self.n_channels = n_channels
        self.channels_axis = channels_axis

    def forward(self, x, log0=0):
        return _pade(self, x, log0, _hip.PADE11, False, softplus_ln2(self.w1), None)

    def backward(self, x, log0=0):
        return _pade(self, x, log0, _hip.PADE11, True, softplus_ln2(self.w1), None)


class Pade22_(Module_):
    """y = x (x + d0 (1 - x)) / (1 + (d0 + d1 - 2) x (1 - x)): a one-bin rational-quadratic spline of [0, 1] with
    end-point derivatives d0 = softplus_ln2(w0), d1 = softplus_ln2(w1) per channel; symmetric=True makes w1 the same
    parameter as w0 (modules_.py:166-222).  One nf_pade pass per direction (the inverse by the cancellation-free root);
    with propagate_density the per-site log-derivatives, in inference and in training."""

    def __init__(self, n_channels=1, channels_axis=1, symmetric=False, label='pade22'):
        super().__init__(label=label)
        self.w0 = torch.nn.Parameter(torch.zeros(n_channels))
        if not symmetric:
            self.w1 = torch.nn.Parameter(torch.zeros(n_channels))
        else:
            self.w1 = self.w0
        self.n_channels = n_channels
        self.channels_axis = channels_axis
        self.symmetric = symmetric

    def _run(self, x, log0, inverse):
        d0 = softplus_ln2(self.w0)
        d1 = d0 if self.symmetric else softplus_ln2(self.w1)
        return _pade(self, x, log0, _hip.PADE22, inverse, d0, d1)

    def forward(self, x, log0=0):
        return self._run(x, log0, False)

    def backward(self, x, log0=0):
        return self._run(x, log0, True)


class Pade32_(Module_):
    """y = x (a + x^2) / (1 + a x^2), a = 3 expit(w0) in (0, 3) per channel: an odd monotone map of the real line with the
    fixed points 0 and +-1, slope a at 0 and 1/a at infinity (modules_.py:225-274).  One nf_pade pass per direction; with
    propagate_density the per-site log-derivatives, in inference and in training.

    Departures from the reference: `w0` is a trainable Parameter (there `-torch.nn.Parameter(..)` leaves a plain tensor:
    no parameters, an empty state_dict, a = 1 for ever), initialised to the reference's constant -log 2 (a = 1, the
    identity); and `backward` works (there it raises UnboundLocalError): the one real root of
    x^3 - a y x^2 + a x - y = 0, finite and odd for every finite y."""

    def __init__(self, n_channels=1, channels_axis=1, label='pade32'):
        super().__init__(label=label)
        self.w0 = torch.nn.Parameter(torch.full((n_channels,), -math.log(2.0)))
        self.n_channels = n_channels
        self.channels_axis = channels_axis

    def forward(self, x, log0=0):
        return _pade(self, x, log0, _hip.PADE32, False, 3 * torch.special.expit(self.w0), None)

    def backward(self, x, log0=0):
        return _pade(self, x, log0, _hip.PADE32, True, 3 * torch.special.expit(self.w0), None)


class Tanh_(Module_):
    """y = tanh x; log|J| = -2 sum log cosh x (modules_.py:72-79); with propagate_density the per-site terms.  One nf_pade
    pass.  log cosh x is evaluated as |x| + log1p(e^{-2|x|}) - ln 2, finite for every finite x: the reference's
    log(cosh(x)) is inf once cosh overflows (|x| > 89 in fp32); the two agree wherever that one is finite.  The
    instance's propagate_density holds in both directions (the reference's backward is a fresh ArcTanh_)."""

    def forward(self, x, log0=0):
        return _pade(self, x, log0, _hip.TANH, False, None, None)

    def backward(self, x, log0=0):
        return _pade(self, x, log0, _hip.TANH, True, None, None)


class ArcTanh_(Module_):
    """y = atanh x; log|J| = -sum log(1 - x^2) = 2 sum log cosh y (modules_.py:82-90), as log1p(x) + log1p(-x): finite
    for every |x| < 1 (the reference's log(cosh(atanh x)) loses x -> +-1).  The inverse direction of Tanh_'s pass; the
    instance's propagate_density holds in both directions."""

    def forward(self, x, log0=0):
        return _pade(self, x, log0, _hip.TANH, True, None, None)

    def backward(self, x, log0=0):
        return _pade(self, x, log0, _hip.TANH, False, None, None)


class SplineNet_(_K4Leaf, SplineNet, Module_):
    """SplineNet with the log-Jacobian (modules_.py:277-302); with propagate_density the per-site log-derivatives."""

    def _k4(self, inverse):
        return _hip.STAGE_SPLINE, inverse, self.knots()


class UnityDistConvertor_(SplineNet_):
    """PDF convertor on [0, 1] (modules_.py:305-316)."""

    def __init__(self, knots_len, symmetric=False, **kwargs):
        extra = dict(xlim=(0.5, 1), ylim=(0.5, 1), extrap={'left': 'anti'}) if symmetric else {}
        super().__init__(knots_len, **kwargs, **extra)


class PhaseDistConvertor_(SplineNet_):
    """PDF convertor on [-pi, pi] (modules_.py:319-330)."""

    def __init__(self, knots_len, symmetric=False, label='phase-dc_', **kwargs):
        pi = math.pi
        extra = (dict(xlim=(0, pi), ylim=(0, pi), extrap={'left': 'anti'}) if symmetric
                 else dict(xlim=(-pi, pi), ylim=(-pi, pi)))
        super().__init__(knots_len, label=label, **kwargs, **extra)


class SgnBiasNet_(Module_):
    """x + sgn(x) w^2: only valid as the very first layer (modules_.py:386-400)."""

    def __init__(self, size=[1], label='sgnbias_'):
        super().__init__(label=label)
        self.w = torch.nn.Parameter(torch.rand(*size) / 10)

    def forward(self, x, log0=0):
        return x + torch.sgn(x) * self.w ** 2, log0

    def backward(self, x, log0=0):
        return x - torch.sgn(x) * self.w ** 2, log0


class DistConvertor_(ModuleList_):
    """PDF convertor for real variables: [SgnBias] [Scale] Expit_ SplineNet_ Logit_ [Scale]
    (modules_.py:333-383); symmetric => spline on (0.5, 1) with an anti-periodic left
    boundary.  The Expit_/SplineNet_/Logit_ triple runs as one fused kernel launch."""

    def __init__(self, knots_len, symmetric=False, label='dc_', sgnbias=False, initial_scale=False,
                 final_scale=False, **kwargs):
        lims = (dict(xlim=(0.5, 1), ylim=(0.5, 1), extrap={'left': 'anti'}) if symmetric
                else dict(xlim=(0, 1), ylim=(0, 1)))
        nets_ = []
        if knots_len > 1:
            nets_ = [Expit_(label='expit_'), SplineNet_(knots_len, label='spline_', **kwargs, **lims),
                     Logit_(label='logit_')]
        if initial_scale:
            nets_.insert(0, ScaleNet_(label='scale_'))
        elif final_scale:
            nets_.append(ScaleNet_(label='scale_'))
        if sgnbias:
            nets_.insert(0, SgnBiasNet_())
        super().__init__(nets_)
        self.label = label

    def _by_label(self, label):
        for net_ in self:
            if net_.label == label:
                return net_

    spline_layer_ = property(lambda self: self._by_label('spline_'))
    scale_layer_ = property(lambda self: self._by_label('scale_'))
    sgnbias_layer_ = property(lambda self: self._by_label('sgnbias_'))

    def _steps(self):
        """Group the children into ('fused', spline_) triples and ('single', module) steps.  A triple fuses when its three
        members carry the same propagate_density; with mixed flags they run one by one, as the reference composes them."""
        mods, steps, i = list(self), [], 0
        while i < len(mods):
            tri = mods[i:i + 3]
            if (len(tri) == 3 and type(tri[0]) is Expit_ and isinstance(tri[1], SplineNet_)
                    and type(tri[2]) is Logit_ and len({bool(t.propagate_density) for t in tri}) == 1):
                steps.append(('fused', tri[1]))
                i += 3
            else:
                steps.append(('single', mods[i]))
                i += 1
        return steps

    def _run(self, x, log0, inverse):
        steps = self._steps()
        for kind, mod in (reversed(steps) if inverse else steps):
            if kind == 'fused':
                x, log0 = _run_stages(bool(mod.propagate_density), x, log0, 7, inverse, mod.knots())
            else:
                x, log0 = mod.backward(x, log0) if inverse else mod.forward(x, log0)
        return x, log0

    def forward(self, x, log0=0):
        return self._run(x, log0, False)

    def backward(self, x, log0=0):
        return self._run(x, log0, True)

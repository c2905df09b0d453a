"""The flow-network protocol (API of the reference's src/nn/_core.py).

A module whose name ends in an underscore maps `(x, log0) -> (y, log0 + log|det dy/dx|)` in
`forward` and applies the inverse map in `backward`; `log0` may be the python number 0.
`Module_` is a leaf transformation and `ModuleList_` their composition.  Three wrappers compose
site-local leaves as the reference does: `MultiChannelModule_` (one module per channel),
`MultiOutChannelModule_` (every module on the whole input, outputs stacked as channels) and
`InvisibilityMaskWrapperModule_` (a leaf on the sites of a mask's channel 0, the others passed
through).  The last runs on `Module_.propagate_density`, the per-site log-density protocol; around
Expit_, Logit_ or SplineNet_ it is one masked K4 pass (`nf_distconv_sites`).
"""
import base64
import copy
import io
import math

import torch


def count_parameters(module):
    return sum(math.prod(p.shape) for p in torch.nn.Module.parameters(module))


class Module_(torch.nn.Module):
    """Leaf of a flow: subclasses implement forward / backward with the Jacobian bookkeeping."""

    propagate_density = False     # True: keep per-site log-densities instead of per-sample sums

    def __init__(self, label=None):
        super().__init__()
        self.label = label

    def forward(self, x, log0=0):
        raise NotImplementedError

    def backward(self, x, log0=0):
        raise NotImplementedError

    def sum_density(self, t):
        """Reduce a per-site log-density to one number per sample (axis 0 is the batch)."""
        if self.propagate_density or t.dim() < 2:
            return t
        return t.flatten(1).sum(dim=1)

    def transfer(self, **kwargs):
        return copy.deepcopy(self)

    npar = property(count_parameters)


def _same_partition(a, b):
    """Do two coupling blocks split the lattice the same way?  (The same mask object, or equal masks: compared once per pair.)"""
    ma, mb = getattr(a, 'mask', None), getattr(b, 'mask', None)
    if ma is None or mb is None:
        return False
    if ma is mb:
        return True
    fn = getattr(ma, 'same_partition', None)
    return bool(fn(mb)) if fn is not None else False


def _run_chain(blocks, method, x, log0):
    """Apply the blocks in order.  Consecutive coupling blocks over the SAME partition hand each other the two parts of the
    field as they are: `cat` followed by the next block's `split` gives the parts back (their supports are disjoint), and on a
    lattice field each of the three is a full pass through memory -- with one coupling block per layer (a common way to
    write a flow; the reference's protocol is unchanged: couplings_.py:54-78) they were ~8 % of a 32^4 inference pass."""
    blocks = list(blocks)
    part_method = 'parts_' + method
    i, n = 0, len(blocks)
    while i < n:
        blk = blocks[i]
        run = getattr(blk, part_method, None)
        j = i + 1
        if run is not None:
            while j < n and getattr(blocks[j], part_method, None) is not None and _same_partition(blk, blocks[j]):
                j += 1
        if run is None or j == i + 1:
            x, log0 = getattr(blk, method)(x, log0)
            i += 1
            continue
        parts = list(blk.mask.split(x))
        for k in range(i, j):
            parts, log0 = getattr(blocks[k], part_method)(parts, log0)
        x = blk.mask.cat(*parts)
        i = j
    return x, log0


class ModuleList_(torch.nn.ModuleList):
    """Composition of flow modules: forward applies them in order, backward inverts them in
    reverse order."""

    _groups = None

    def __init__(self, nets_, label=None):
        super().__init__(nets_)
        self.label = label

    def forward(self, x, log0=0):
        return _run_chain(self, 'forward', x, log0)

    def backward(self, x, log0=0):
        return _run_chain(reversed(list(self)), 'backward', x, log0)

    __call__ = forward        # bypass nn.Module hooks, as the reference does

    def hack(self, x, log0=0):
        """All intermediate (x, log0) pairs of a forward pass, input included."""
        states = [(x, log0)]
        for blk in self:
            states.append(blk.forward(*states[-1]))
        return states

    # -- optimizer parameter groups: [{'ind': [block indices], 'hyper': {...}}, ...]
    def setup_groups(self, groups=None):
        self._groups = groups

    def grouped_parameters(self):
        if self._groups is None:
            return super().parameters()
        return [dict(params=[p for k in grp['ind'] for p in self[k].parameters()], **grp['hyper'])
                for grp in self._groups]

    # -- (de)serialisation helpers
    def get_weights_blob(self):
        buf = io.BytesIO()
        torch.save(self.state_dict(), buf)
        return base64.b64encode(buf.getvalue()).decode('utf-8')

    def set_weights_blob(self, blob, map_location=torch.device('cpu')):
        state = torch.load(io.BytesIO(base64.b64decode(blob.strip())), map_location=map_location,
                           weights_only=True)
        self.load_state_dict(state)

    def _set_trainable(self, flag):
        for p in self.parameters():
            p.requires_grad = flag

    def freeze_parameters(self):
        self._set_trainable(False)

    def unfreeze_parameters(self):
        self._set_trainable(True)

    def transfer(self, **kwargs):
        return type(self)([blk.transfer(**kwargs) for blk in self])

    def to(self, *args, **kwargs):
        for blk in self:
            blk.to(*args, **kwargs)
        return self

    npar = property(count_parameters)


class MultiChannelModule_(torch.nn.ModuleList):
    """One module per channel (reference: src/nn/_core.py:137-178): channel j of the input, split off along
    `channels_axis` (kept as an axis of extent 1 with keep_channels_axis, removed otherwise), goes through nets_[j]; the
    outputs are put back together along the same axis and the log-Jacobians of the channels add up."""

    def __init__(self, nets_, label=None, channels_axis=1, keep_channels_axis=True):
        super().__init__(nets_)
        self.channels_axis = channels_axis
        self.keep_channels_axis = keep_channels_axis
        self.label = label

    def __call__(self, *args, **kwargs):
        return self.forward(*args, **kwargs)

    def forward(self, x, log0=0):
        return self._map(x, [net_.forward for net_ in self], log0=log0)

    def backward(self, x, log0=0):
        return self._map(x, [net_.backward for net_ in self], log0=log0)

    def _map(self, x, f_, log0=0):
        if self.keep_channels_axis:
            parts = x.split(1, dim=self.channels_axis)
        else:
            parts = x.unbind(dim=self.channels_axis)
        if len(parts) != len(f_):
            raise ValueError(f"{len(parts)} channels on axis {self.channels_axis} but {len(f_)} networks")
        out = [fj_(xj) for fj_, xj in zip(f_, parts)]
        join = torch.cat if self.keep_channels_axis else torch.stack
        x = join([o[0] for o in out], dim=self.channels_axis)
        return x, log0 + sum(o[1] for o in out)

    npar = property(count_parameters)


class MultiOutChannelModule_(MultiChannelModule_):
    """Every module on the whole input; the outputs are concatenated along `channels_axis` and the log-Jacobians add up
    (reference: src/nn/_core.py:182-191)."""

    def _map(self, x, f_, log0=0):
        out = [fj_(x) for fj_ in f_]
        x = torch.cat([o[0] for o in out], dim=self.channels_axis)
        return x, log0 + sum(o[1] for o in out)


class InvisibilityMaskWrapperModule_(Module_):
    """`net_` on the visible sites only: the sites of the mask's channel 0 are transformed and keep their log-densities,
    the others pass through with log-density 0 (reference: src/nn/_core.py:195-231).  Sets net_.propagate_density, as
    the reference does; the wrapper's own flag chooses per-sample sums or per-site densities.

    Around Expit_, Logit_ or SplineNet_ (any K4 leaf) on a mask with `activity()` whose shape is the lattice, the whole
    wrapper is ONE masked nf_distconv_sites pass over the visible sites: no split, purify, cat or per-site tensor.  Any
    other leaf takes the reference's composition.  Departure: the reference evaluates net_ on the zeroed invisible sites
    too, and for Logit_ its log(0) * 0 gives NaN in both y and log J; the masked pass copies those sites unchanged, so
    its values are finite, and equal to the reference's wherever those are finite."""

    def __init__(self, net_, *, mask):
        super().__init__(label=f'wrapper:{net_.label}')
        self.net_ = net_
        self.mask = mask
        self.net_.propagate_density = True  # does not sum the density

    def _activity(self, x):
        """The visible sites as (V,) uint8 bytes on x's device, or None where the masked pass does not apply."""
        if not hasattr(self.net_, '_k4') or not hasattr(self.mask, 'activity') or not x.is_cuda or x.dim() < 2:
            return None
        act = self.mask.activity(0)
        if tuple(act.shape) != tuple(x.shape[1:]):
            return None
        cache = self.__dict__.get('_act_cache')
        if cache is None or cache[0] is not act or cache[1] != x.device:
            cache = (act, x.device, act.to(device=x.device, dtype=torch.uint8).reshape(-1).contiguous())
            self.__dict__['_act_cache'] = cache
        return cache[2]

    def _run(self, x, log0, inverse):
        act = self._activity(x)
        if act is not None:
            from .scalar.modules_ import _run_stages
            return _run_stages(bool(self.propagate_density), x, log0, *self.net_._k4(inverse), mask=act)
        x_v, x_invisible = self.mask.split(x)  # x_v: x_visible
        x_v, logJ_density = self.net_.backward(x_v) if inverse else self.net_.forward(x_v)
        x_v = self.mask.purify(x_v, channel=0)
        logJ = self.sum_density(self.mask.purify(logJ_density, channel=0))
        return self.mask.cat(x_v, x_invisible), log0 + logJ

    def forward(self, x, log0=0):
        return self._run(x, log0, False)

    def backward(self, x, log0=0):
        return self._run(x, log0, True)

"""Controlled coupling layers (reference: src/nn/scalar/cntr_couplings_.py).

A controlled block is a coupling block whose FIRST parameter net reads a control field instead of the frozen half of
the field it transforms; every later net reads the frozen half as usual.  `DirectCntrCoupling_` takes and returns the
pair `(x, control)`; `CntrCoupling_` draws the control from a generator in `forward`, keeps it and reuses it in
`backward`, so the caller sees an ordinary `(x, log0)` module.

The control goes to the net exactly as it is given: it is not purified, so the net convolves its values on ALL sites,
the active ones of the first atom included, and those values change the output, as in the reference.  The kernels
behind a controlled atom make no assumption about where their net's input vanishes (every first layer is a full
convolution of its input: `frozen_input_is_masked = False` keeps the parity-compact first layer of the split-fp16 chain,
which reads the frozen sites only, out of a controlled block), so the controlled atom takes the same paths as an ordinary one: the materialising path in fp64 / fp32,
the pair-compact logits of `ConvAct.forward_active`, the one-launch small-lattice kernel, the split-fp16 chains, the
logit-free training node and the per-site densities (tests/test_cntr_couplings.py holds each of them to the oracle
with a control that is non-zero everywhere).
"""
import torch

from .couplings_ import Coupling_
from .couplings_ import ShiftCoupling_, AffineCoupling_
from .couplings_ import RQSplineCoupling_, MultiRQSplineCoupling_


class _Absent:
    """An inherited attribute a subclass does not have: looking it up raises AttributeError."""

    def __set_name__(self, owner, name):
        self._name = name

    def __get__(self, obj, cls=None):
        raise AttributeError(f"{(cls or type(obj)).__name__} has no {self._name}: a controlled block takes (x, control)")


class DirectCntrCoupling_(Coupling_):
    """`Coupling_` whose net 0 reads `control` (shaped like x) in place of the frozen half:
    `forward((x, control), log0) -> ((y, control), log0 + log|J|)`, and `backward` the inverse.

    Its input is a pair, so a `ModuleList_` must not merge it into a chain of blocks over one partition: it has no
    `parts_forward` / `parts_backward`."""

    parts_forward = _Absent()
    parts_backward = _Absent()
    # net 0 reads the control, which is non-zero on every site: no first layer of this block may skip the active sites
    frozen_input_is_masked = False

    def _as_control(self, control, like):
        """The control as the net takes it: on the field's device and in its dtype, otherwise untouched (not purified);
        no gradient flows into it."""
        control = control.detach()
        if control.device != like.device or control.dtype != like.dtype:
            control = control.to(device=like.device, dtype=like.dtype)
        return control

    def _cntr_parts(self, inverse, parts, control, log0):
        """The block on the two parts of the field: `Coupling_.parts_forward` / `parts_backward` with the control as net 0's
        input."""
        atom = self.atomic_backward if inverse else self.atomic_forward
        ctl = self._as_control(control, parts[0])
        order = reversed(range(len(self.nets))) if inverse else range(len(self.nets))
        for k in order:
            p = k % 2
            parts[p], log0 = atom(x_active=parts[p], x_frozen=ctl if k == 0 else parts[1 - p], parity=p,
                                  net=self.nets[k], log0=log0)
        return parts, log0

    def forward(self, x_and_control, log0=0):
        x, control = x_and_control
        parts, log0 = self._cntr_parts(False, list(self.mask.split(x)), control, log0)
        return (self.mask.cat(*parts), control), log0

    def backward(self, x_and_control, log0=0):
        x, control = x_and_control
        parts, log0 = self._cntr_parts(True, list(self.mask.split(x)), control, log0)
        return (self.mask.cat(*parts), control), log0


class CntrCoupling_(DirectCntrCoupling_):
    """A controlled block that hides the control: `forward(x, log0)` calls `control_generator(batch_size)`, keeps the
    result in `self.control` (replaced by the next forward) and `backward(x, log0)` reuses it.

    It has its own `parts_forward` / `parts_backward`, so a `ModuleList_` chain over one mask stays controlled; the
    generator is called once per forward and never in backward.  `backward` before any `forward` is an error.

    Replaying a controlled layer from a captured HIP graph (`posterior.graphed`, `GraphedTrainStep`) is not supported:
    whether the generator's draw is part of the capture depends on the generator, and nothing tests it."""

    def __init__(self, *args, control_generator=None, **kwargs):
        super().__init__(*args, **kwargs)
        self.control_generator = control_generator
        self.control = None

    def _new_control(self, batch_size):
        if self.control_generator is None:
            raise RuntimeError(f"{type(self).__name__} was built without a control_generator")
        self.control = self.control_generator(batch_size)
        return self.control

    def _kept_control(self):
        if self.control is None:
            raise RuntimeError(f"{type(self).__name__}.backward reuses the control of the last forward call, and forward "
                               "has not been called yet")
        return self.control

    def parts_forward(self, parts, log0=0):
        return self._cntr_parts(False, parts, self._new_control(parts[0].shape[0]), log0)

    def parts_backward(self, parts, log0=0):
        return self._cntr_parts(True, parts, self._kept_control(), log0)

    def forward(self, x, log0=0):
        (x, _), log0 = super().forward((x, self._new_control(x.shape[0])), log0=log0)
        return x, log0

    def backward(self, x, log0=0):
        (x, _), log0 = super().backward((x, self._kept_control()), log0=log0)
        return x, log0

    def _ctor_kwargs(self):
        return dict(super()._ctor_kwargs(), control_generator=self.control_generator)


class CntrShiftCoupling_(CntrCoupling_, ShiftCoupling_):
    pass


class CntrAffineCoupling_(CntrCoupling_, AffineCoupling_):
    pass


class CntrRQSplineCoupling_(CntrCoupling_, RQSplineCoupling_):
    pass


class CntrMultiRQSplineCoupling_(CntrCoupling_, MultiRQSplineCoupling_):
    pass

#!/usr/bin/env python3
"""Generate tests/golden/sites.npz by RUNNING THE REFERENCE's per-site density protocol.

Container-only, like make_golden.py (same invocation, with this file's name):

    mkdir -p /tmp/nf_oracle && ln -sfn /root/reference/src /tmp/nf_oracle/normflow
    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=/tmp/nf_oracle python3 tests/golden/make_golden_sites.py

The file holds data only, CPU, fp64: per case the module's state_dict, the input and the reference's outputs.
  * leaves: Expit_, Logit_, SplineNet_ on (0, 1) and on the symmetric range (0.5, 1) with the anti left boundary, random
    non-zero weights; forward and backward, each per sample and per site (the class flag Module_.propagate_density, under
    which the reference's Expit_.backward / Logit_.backward, fresh opposite modules, are per site as well);
  * DistConvertor_ (symmetric and not) under the class flag, both directions;
  * InvisibilityMaskWrapperModule_ around SplineNet_ and Pade22_ on an EvenOddMask, both directions, with the wrapper's
    own flag off and on; around Expit_ and Logit_ forward (Logit_: NaN at the invisible sites in the reference);
  * MultiChannelModule_ (keep_channels_axis True and False) and MultiOutChannelModule_ of [SplineNet_, Pade22_];
  * ScalarPhi4Action.action_density and action on 1-D to 4-D lattices with a != 1.
tests/test_site_densities.py replays it.
"""
import os
import warnings

import numpy as np

warnings.filterwarnings("ignore")
HERE = os.path.dirname(os.path.abspath(__file__))

import torch  # noqa: E402
import normflow  # noqa: E402  (the REFERENCE; sets default dtype fp64)
from normflow.nn import Module_, DistConvertor_, Pade22_  # noqa: E402
from normflow.nn import InvisibilityMaskWrapperModule_, MultiChannelModule_, MultiOutChannelModule_  # noqa: E402
from normflow.nn.scalar.modules_ import Expit_, Logit_, SplineNet_  # noqa: E402
from normflow.mask import EvenOddMask  # noqa: E402
from normflow.action import ScalarPhi4Action  # noqa: E402

torch.set_default_device('cpu')
assert torch.get_default_dtype() == torch.float64

LAT = (4, 6)
B = 3
SYM = dict(xlim=(0.5, 1), ylim=(0.5, 1), extrap={'left': 'anti'})


def randomise(mod, gen, scale=0.8):
    with torch.no_grad():
        for p in mod.parameters():
            p.copy_(scale * torch.randn(p.shape, generator=gen))
    return mod


def unit(gen, shape):
    return torch.rand(shape, generator=gen) * 0.96 + 0.02


def real(gen, shape):
    return 2.5 * torch.randn(shape, generator=gen)


def run(mod, x, inverse, class_flag):
    Module_.propagate_density = class_flag
    try:
        with torch.no_grad():
            return mod.backward(x) if inverse else mod.forward(x)
    finally:
        Module_.propagate_density = False


def put(out, pre, mod, **arrays):
    for key, val in mod.state_dict().items():
        out[pre + "state/" + key] = val.numpy().copy()
    for key, val in arrays.items():
        out[pre + key] = val.numpy().copy() if torch.is_tensor(val) else val


def main():
    out = {}
    gen = torch.Generator().manual_seed(2025)
    shape = (B,) + LAT
    # -- leaves and DistConvertor_: (module, forward input domain, backward input domain)
    leaves = {
        'expit': (Expit_(), real, unit),
        'logit': (Logit_(), unit, real),
        'spline': (randomise(SplineNet_(6), gen), unit, unit),
        'spline_sym': (randomise(SplineNet_(6, **SYM), gen), unit, unit),
        'dc': (randomise(DistConvertor_(6), gen), real, real),
        'dc_sym': (randomise(DistConvertor_(6, symmetric=True), gen), real, real),
    }
    for name, (mod, dom_f, dom_b) in leaves.items():
        pre = f"leaf/{name}/"
        put(out, pre, mod)
        for d, inverse, dom in (("fwd", False, dom_f), ("bwd", True, dom_b)):
            x = dom(gen, shape)
            y, logj = run(mod, x, inverse, False)
            y_s, sites = run(mod, x, inverse, True)
            assert torch.equal(y, y_s) and sites.shape == x.shape
            out[pre + d + "_x"] = x.numpy()
            out[pre + d + "_y"] = y.numpy()
            out[pre + d + "_logj"] = logj.numpy()
            out[pre + d + "_sites"] = sites.numpy()
    # -- the invisibility wrapper on an even-odd mask
    mask = EvenOddMask(shape=LAT)
    out["mask"] = mask._mask.numpy().copy()
    wrapped = {
        'spline': (lambda: randomise(SplineNet_(6), gen), unit, unit, True),
        'pade22': (lambda: randomise(Pade22_(), gen), unit, unit, True),
        'expit': (lambda: Expit_(), real, None, False),
        'logit': (lambda: Logit_(), unit, None, False),
    }
    for name, (make, dom_f, dom_b, both) in wrapped.items():
        leaf = make()
        wrap = InvisibilityMaskWrapperModule_(leaf, mask=mask)
        pre = f"wrap/{name}/"
        put(out, pre, leaf)
        for d, inverse, dom in (("fwd", False, dom_f), ("bwd", True, dom_b)):
            if not both and inverse:
                continue
            x = dom(gen, shape)
            out[pre + d + "_x"] = x.numpy()
            for flag in (False, True):
                wrap.propagate_density = flag
                with torch.no_grad():
                    y, logj = wrap.backward(x) if inverse else wrap.forward(x)
                tag = "sites" if flag else "sum"
                out[pre + d + f"_{tag}_y"] = y.numpy()
                out[pre + d + f"_{tag}_logj"] = logj.numpy()
    # -- multi-channel composition: channel 0 through a spline, channel 1 through a Pade22_
    for name, keep in (("keep", True), ("drop", False)):
        mod = MultiChannelModule_([randomise(SplineNet_(5), gen), randomise(Pade22_(), gen)], channels_axis=1,
                                  keep_channels_axis=keep)
        pre = f"multi/{name}/"
        put(out, pre, mod)
        x = unit(gen, (B, 2) + LAT)
        out[pre + "x"] = x.numpy()
        for d, inverse in (("fwd", False), ("bwd", True)):
            y, logj = run(mod, x, inverse, False)
            out[pre + d + "_y"] = y.numpy()
            out[pre + d + "_logj"] = logj.numpy()
    mod = MultiOutChannelModule_([randomise(SplineNet_(5), gen), randomise(Pade22_(), gen)], channels_axis=1)
    pre = "multiout/"
    put(out, pre, mod)
    x = unit(gen, (B, 1) + LAT)
    out[pre + "x"] = x.numpy()
    for d, inverse in (("fwd", False), ("bwd", True)):
        y, logj = run(mod, x, inverse, False)
        out[pre + d + "_y"] = y.numpy()
        out[pre + d + "_logj"] = logj.numpy()
    # -- action density
    act = ScalarPhi4Action(m_sq=-1.3, lambd=0.6, kappa=0.8, a=0.7)
    for name, lat in (("d1", (10,)), ("d2", (4, 6)), ("d3", (3, 2, 5)), ("d4", (2, 3, 4, 3))):
        x = torch.randn((B,) + lat, generator=gen)
        pre = f"action/{name}/"
        out[pre + "x"] = x.numpy()
        out[pre + "density"] = act.action_density(x).numpy()
        out[pre + "action"] = act.action(x).numpy()
    out["action/coef"] = np.array([act.m_sq, act.lambd, act.kappa, act.a])
    path = os.path.join(HERE, "sites.npz")
    np.savez_compressed(path, **out)
    print(f"sites: {len(out)} arrays, {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()

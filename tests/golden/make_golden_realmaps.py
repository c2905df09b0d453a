#!/usr/bin/env python3
"""Generate tests/golden/realmaps.npz by RUNNING THE REFERENCE's Tanh_, ArcTanh_ and Pade32_.

Invoked like make_golden.py (the reference importable as `normflow`), with this file's name.

The file holds data only, CPU, fp64.
  * `tanh`, `arctanh`: forward and backward, each per sample and per site (the class flag Module_.propagate_density,
    under which the reference's backward, a fresh opposite module, is per site as well).  Field (3, 3, 4, 6).  Inputs on the
    real line: 0, +-1e-7, +-1, +-30 and draws of scale 2.5; inputs on (-1, 1): 0, +-(1 - 1e-6) and uniform draws between.
  * `p32_*`: Pade32_ FORWARD only (the reference's backward raises UnboundLocalError).  The reference's `w0` is a plain
    tensor, not a parameter (`-torch.nn.Parameter(..)`), so the generator assigns it and stores it as the array `w0`:
    C = 1 with w0 = -log 2 (a = 1, the identity), -3, 3, 0.4; C = 3 on channels_axis 1 and -1 with w0 = (-2, 0.3, 2.5).
    x: 0, +-1e-7, +-1, +-1e3 and draws of scale 2.
tests/test_realmaps.py replays it.
"""
import math
import os
import warnings

import numpy as np

warnings.filterwarnings("ignore")
HERE = os.path.dirname(os.path.abspath(__file__))

import torch  # noqa: E402
import normflow  # noqa: E402  (the REFERENCE; sets default dtype fp64)
from normflow.nn import Module_  # noqa: E402
from normflow.nn.scalar.modules_ import Tanh_, ArcTanh_, Pade32_  # noqa: E402

torch.set_default_device('cpu')
assert torch.get_default_dtype() == torch.float64

SHAPE = (3, 3, 4, 6)
REAL_ENDS = [0.0, 1e-7, -1e-7, 1.0, -1.0, 30.0, -30.0]
UNIT_ENDS = [0.0, 1 - 1e-6, -(1 - 1e-6)]
PADE_ENDS = [0.0, 1e-7, -1e-7, 1.0, -1.0, 1e3, -1e3]

# name: (n_channels, channels_axis, field shape, w0)
PADE32 = {
    'p32_a1': (1, 1, SHAPE, [-math.log(2.0)]),
    'p32_wm3': (1, 1, SHAPE, [-3.0]),
    'p32_wp3': (1, 1, SHAPE, [3.0]),
    'p32_w04': (1, 1, SHAPE, [0.4]),
    'p32_c3_ax1': (3, 1, SHAPE, [-2.0, 0.3, 2.5]),
    'p32_c3_axm1': (3, -1, (3, 4, 6, 3), [-2.0, 0.3, 2.5]),
}


def grid(shape, draws, ends):
    x = draws.reshape(-1).clone()
    x[:len(ends)] = torch.tensor(ends)
    x[-len(ends):] = torch.tensor(ends[::-1])
    return x.reshape(shape)


def run(mod, x, inverse, per_site):
    Module_.propagate_density = per_site
    try:
        with torch.no_grad():
            return mod.backward(x) if inverse else mod.forward(x)
    finally:
        Module_.propagate_density = False


def record(out, pre, mod, x, d, inverse):
    y, logj = run(mod, x, inverse, False)
    y_s, sites = run(mod, x, inverse, True)
    assert torch.equal(y, y_s) and sites.shape == x.shape and logj.shape == x.shape[:1]
    out[pre + d + "_x"] = x.numpy()
    out[pre + d + "_y"] = y.numpy()
    out[pre + d + "_logj"] = logj.numpy()
    out[pre + d + "_sites"] = sites.numpy()


def main():
    out = {}
    gen = torch.Generator().manual_seed(2026)
    n = int(np.prod(SHAPE))
    real = grid(SHAPE, 2.5 * torch.randn(n, generator=gen), REAL_ENDS)
    unit = grid(SHAPE, (torch.rand(n, generator=gen) * 2 - 1) * (1 - 1e-6), UNIT_ENDS)
    assert unit.abs().max() <= 1 - 1e-6
    # tanh: forward on the real line, backward (= atanh) on (-1, 1); arctanh the other way round
    for name, mod, x_f, x_b in (("tanh", Tanh_(), real, unit), ("arctanh", ArcTanh_(), unit, real)):
        record(out, f"{name}/", mod, x_f, "fwd", False)
        record(out, f"{name}/", mod, x_b, "bwd", True)
    for name, (nch, axis, shape, w0) in PADE32.items():
        mod = Pade32_(n_channels=nch, channels_axis=axis)
        assert len(list(mod.parameters())) == 0 and len(mod.state_dict()) == 0      # the reference has no state here
        mod.w0 = torch.tensor(w0)
        x = grid(shape, 2.0 * torch.randn(int(np.prod(shape)), generator=gen), PADE_ENDS)
        pre = f"{name}/"
        out[pre + "n_channels"] = np.int64(nch)
        out[pre + "channels_axis"] = np.int64(axis)
        out[pre + "w0"] = np.array(w0)
        record(out, pre, mod, x, "fwd", False)
    path = os.path.join(HERE, "realmaps.npz")
    np.savez_compressed(path, **out)
    print(f"realmaps: {len(out)} arrays, {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()

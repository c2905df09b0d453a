#!/usr/bin/env python3
"""Generate tests/golden/pade.npz by RUNNING THE REFERENCE's Pade11_ / Pade22_.

Container-only, like make_golden.py (same invocation, with this file's name):

    mkdir -p /tmp/nf_oracle && ln -sfn /root/reference/src /tmp/nf_oracle/normflow
    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=/tmp/nf_oracle python3 tests/golden/make_golden_pade.py

The file holds data only: per case the module's constructor arguments, its state_dict and the reference's outputs, CPU,
fp64.  Inputs: a grid on [0, 1] that holds 0, 1e-7, 1 - 1e-7 and 1, plus uniform draws.  Per case and direction
(forward on x, backward on the same values read as y): the value, log J summed per sample and log J per site
(Module_.propagate_density = True).  Cases: n_channels 1 and 3, channels_axis 1 and -1, random non-zero weights,
symmetric True and False; `d0one`: w0 = 0 (d0 = 1) and w1 = (0, 1.3, -0.8), so a = 0 at every y in channel 0 (the
identity) and at y = 0 in the others: the reference's a == 0 branch; `zero`: the zero-initialised modules.
tests/test_pade.py replays it.
"""
import os
import warnings

import numpy as np

warnings.filterwarnings("ignore")
HERE = os.path.dirname(os.path.abspath(__file__))

import torch  # noqa: E402
import normflow  # noqa: E402  (the REFERENCE; sets default dtype fp64)
from normflow.nn import Module_, Pade11_, Pade22_  # noqa: E402

torch.set_default_device('cpu')
assert torch.get_default_dtype() == torch.float64

ENDS = [0.0, 1e-7, 1 - 1e-7, 1.0]

# name: (class, n_channels, channels_axis, symmetric, field shape, weights: None = random, or {name: values})
CASES = {
    'p11_c1': (Pade11_, 1, 1, False, (4, 2, 6), None),
    'p11_c3_ax1': (Pade11_, 3, 1, False, (4, 3, 5), None),
    'p11_c3_axm1': (Pade11_, 3, -1, False, (4, 5, 3), None),
    'p11_zero': (Pade11_, 1, 1, False, (3, 8), {'w1': [0.0]}),
    'p22_c1': (Pade22_, 1, 1, False, (4, 2, 6), None),
    'p22_c3_ax1': (Pade22_, 3, 1, False, (4, 3, 5), None),
    'p22_c3_axm1': (Pade22_, 3, -1, False, (4, 5, 3), None),
    'p22_sym_c3_ax1': (Pade22_, 3, 1, True, (4, 3, 5), None),
    'p22_sym_c1': (Pade22_, 1, 1, True, (4, 2, 6), None),
    'p22_d0one': (Pade22_, 3, 1, False, (4, 3, 5), {'w0': [0.0, 0.0, 0.0], 'w1': [0.0, 1.3, -0.8]}),
    'p22_zero': (Pade22_, 1, 1, False, (3, 8), {'w0': [0.0], 'w1': [0.0]}),
}


def grid(shape, gen):
    n = int(np.prod(shape))
    x = torch.rand(n, generator=gen)
    x[:len(ENDS)] = torch.tensor(ENDS)
    x[-len(ENDS):] = torch.tensor(ENDS[::-1])
    return x.reshape(shape)


def run(mod, x, inverse, per_site):
    Module_.propagate_density = per_site
    try:
        with torch.no_grad():
            return mod.backward(x) if inverse else mod.forward(x)
    finally:
        Module_.propagate_density = False


def main():
    out = {}
    gen = torch.Generator().manual_seed(2024)
    for name, (cls, nch, axis, sym, shape, weights) in CASES.items():
        kw = dict(n_channels=nch, channels_axis=axis)
        if cls is Pade22_:
            kw['symmetric'] = sym
        mod = cls(**kw)
        with torch.no_grad():
            for pname, p in mod.named_parameters():
                if weights is None:
                    p.copy_(1.5 * torch.randn(nch, generator=gen))
                else:
                    p.copy_(torch.tensor(weights[pname]))
        x = grid(shape, gen)
        pre = f"{name}/"
        out[pre + "kind"] = np.int64(11 if cls is Pade11_ else 22)
        out[pre + "n_channels"] = np.int64(nch)
        out[pre + "channels_axis"] = np.int64(axis)
        out[pre + "symmetric"] = np.bool_(sym)
        for key, val in mod.state_dict().items():
            out[pre + "state/" + key] = val.numpy().copy()
        out[pre + "x"] = x.numpy()
        for direction, inverse in (("fwd", False), ("bwd", True)):
            y, logj = run(mod, x, inverse, False)
            y_site, logj_site = run(mod, x, inverse, True)
            assert torch.equal(y, y_site)
            out[pre + direction + "_y"] = y.numpy()
            out[pre + direction + "_logj"] = logj.numpy()
            out[pre + direction + "_sites"] = logj_site.numpy()
    path = os.path.join(HERE, "pade.npz")
    np.savez_compressed(path, **out)
    print(f"pade: {len(CASES)} cases, {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()

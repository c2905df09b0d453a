#!/usr/bin/env python3
"""Generate tests/golden/cntr.npz by RUNNING THE REFERENCE's controlled couplings (nn/scalar/cntr_couplings_.py).

Invoked like make_golden.py (the reference importable as `normflow`), with this file's name.

The file holds data only, CPU, fp64.  Per lattice ((4, 6) and (2, 2, 4, 4), B = 3) and variant (CntrShiftCoupling_,
CntrAffineCoupling_, CntrRQSplineCoupling_ with m = 5 knots, xlim = ylim = (-3, 3), linear tails): three nets
ConvAct(1, n_out, 3, conv_dim=d, hidden_sizes=[4], acts=['tanh', None]) on an EvenOddMask, a control that is random on
ALL sites (the generator returns this one tensor), the parameters, x, forward y and log J, the gradients of
mean(y^2) + mean(log J) with respect to x and every parameter, and for shift and affine the outputs of
backward(y, log J).  The RQ-spline inverse is not recorded (the reference's inverse with linear tails does not round-trip),
and neither is CntrMultiRQSplineCoupling_ (the reference's ConvAct does not take its (B, n_s, *L) control).
tests/test_cntr_couplings.py replays it.
"""
import os
import warnings

import numpy as np

warnings.filterwarnings("ignore")
HERE = os.path.dirname(os.path.abspath(__file__))

import torch  # noqa: E402
import normflow  # noqa: E402  (the REFERENCE; sets default dtype fp64)
from normflow.mask import EvenOddMask  # noqa: E402
from normflow.nn import ConvAct  # noqa: E402
from normflow.nn.scalar.cntr_couplings_ import (CntrShiftCoupling_, CntrAffineCoupling_,  # noqa: E402
                                                CntrRQSplineCoupling_)

torch.set_default_device('cpu')
assert torch.get_default_dtype() == torch.float64

B, M = 3, 5
LIM = dict(xlim=(-3.0, 3.0), ylim=(-3.0, 3.0), extrap={'left': 'linear', 'right': 'linear'})
VARIANTS = {'shift': (CntrShiftCoupling_, 1, {}), 'affine': (CntrAffineCoupling_, 2, {}),
            'rqs': (CntrRQSplineCoupling_, 3 * M - 2, LIM)}


def npy(t):
    return t.detach().cpu().numpy().copy()


def main():
    out, seed = {}, 5000
    for d, shape in ((2, (4, 6)), (4, (2, 2, 4, 4))):
        for kind, (cls, n_out, kw) in VARIANTS.items():
            seed += 1
            torch.manual_seed(seed)
            nets = [ConvAct(1, n_out, 3, conv_dim=d, hidden_sizes=[4], acts=['tanh', None]) for _ in range(3)]
            control = 1.1 * torch.randn((B,) + shape)
            calls = []

            def generator(n, control=control, calls=calls):
                calls.append(n)
                return control
            cpl = cls(nets, mask=EvenOddMask(shape=shape), control_generator=generator, **kw)
            x = (1.3 * torch.randn((B,) + shape)).requires_grad_(True)
            y, logJ = cpl(x)
            if not torch.is_tensor(logJ):          # a shift leaves log0 = 0 as it is
                logJ = torch.zeros(B)
            loss = (y ** 2).mean() + logJ.mean()
            names = [n for n, _ in cpl.named_parameters()]
            plist = [p for _, p in cpl.named_parameters()]
            grads = torch.autograd.grad(loss, [x] + plist, allow_unused=True)
            tag = f"{kind}/d{d}"
            out.update({f"{tag}/shape": np.array(shape), f"{tag}/x": npy(x), f"{tag}/control": npy(control),
                        f"{tag}/y": npy(y), f"{tag}/logJ": npy(logJ), f"{tag}/grad_x": npy(grads[0])})
            for n, p, gp in zip(names, plist, grads[1:]):
                out[f"{tag}/param/{n}"] = npy(p)
                out[f"{tag}/gparam/{n}"] = npy(gp if gp is not None else torch.zeros_like(p))
            if kind != 'rqs':
                with torch.no_grad():
                    xhat, l_rt = cpl.backward(y.detach(), logJ.detach())
                assert (xhat - x).abs().max().item() < 1e-12
                out[f"{tag}/xhat"] = npy(xhat)
                out[f"{tag}/logJ_rt"] = npy(l_rt)
            assert calls == [B]
            assert all(np.isfinite(v).all() for k, v in out.items() if k.startswith(tag))
    path = os.path.join(HERE, "cntr.npz")
    np.savez_compressed(path, **out)
    print(f"cntr: {len(out)} arrays, {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()

"""The per-site density protocol without a GPU: the reference's wrappers are importable with its constructor arguments,
`npar` and state_dict keys; ScalarPhi4Action.action_density on host tensors against the reference's outputs
(tests/golden/sites.npz) and summed against `action`; DistConvertor_ grouping by flag; the new C entry points are
exported and validate their arguments before touching a device."""
import ctypes

import pytest
import torch

from normflow__amd import _hip
from normflow__amd.action import ScalarPhi4Action
from normflow__amd.mask import EvenOddMask
from normflow__amd.nn import (InvisibilityMaskWrapperModule_, MultiChannelModule_, MultiOutChannelModule_,
                              DistConvertor_, Expit_, Logit_, SplineNet_, Pade22_, Module_)


def test_wrappers_exported_with_the_reference_arguments(golden):
    z = golden("sites")
    mod = MultiChannelModule_([SplineNet_(5), Pade22_()], label='mc', channels_axis=1, keep_channels_axis=False)
    assert mod.channels_axis == 1 and mod.keep_channels_axis is False and mod.label == 'mc'
    keys = {k[len("multi/drop/state/"):] for k in z.files if k.startswith("multi/drop/state/")}
    assert set(mod.state_dict()) == keys
    assert mod.npar == 4 + 4 + 5 + 2
    out = MultiOutChannelModule_([SplineNet_(5), Pade22_()])
    keys = {k[len("multiout/state/"):] for k in z.files if k.startswith("multiout/state/")}
    assert set(out.state_dict()) == keys and out.keep_channels_axis is True
    leaf = SplineNet_(6, label='spl')
    assert leaf.propagate_density is False
    wrap = InvisibilityMaskWrapperModule_(leaf, mask=EvenOddMask(shape=(4, 6)))
    assert leaf.propagate_density is True and wrap.propagate_density is False and Module_.propagate_density is False
    assert wrap.label == 'wrapper:spl' and wrap.npar == leaf.npar
    assert wrap._activity(torch.zeros(2, 4, 6)) is None          # host tensor: the generic composition


def test_wrapper_generic_composition_on_host():
    """A leaf without a K4 pass takes the reference's composition: visible sites transformed, the others passed."""
    class Double_(Module_):
        def forward(self, x, log0=0):
            dens = torch.full_like(x, 0.6931471805599453)
            return 2 * x, log0 + (dens if self.propagate_density else dens.flatten(1).sum(1))

        def backward(self, x, log0=0):
            dens = torch.full_like(x, -0.6931471805599453)
            return x / 2, log0 + (dens if self.propagate_density else dens.flatten(1).sum(1))

    mask = EvenOddMask(shape=(4, 6))
    wrap = InvisibilityMaskWrapperModule_(Double_(label='d'), mask=mask)
    x = torch.randn(3, 4, 6, dtype=torch.float64)
    y, lj = wrap(x)
    vis = mask._mask.bool().cpu()
    assert torch.equal(y[:, vis], 2 * x[:, vis]) and torch.equal(y[:, ~vis], x[:, ~vis])
    assert torch.allclose(lj, torch.full((3,), 12 * 0.6931471805599453, dtype=torch.float64))
    wrap.propagate_density = True
    xb, s = wrap.backward(y)
    assert torch.equal(xb, x) and s.shape == x.shape and (s[:, ~vis] == 0).all()


def test_action_density_on_host_vs_reference(golden):
    z = golden("sites")
    m_sq, lambd, kappa, a = (float(v) for v in z["action/coef"])
    act = ScalarPhi4Action(m_sq=m_sq, lambd=lambd, kappa=kappa, a=a)
    for name in ("d1", "d2", "d3", "d4"):
        x = torch.from_numpy(z[f"action/{name}/x"])
        dens = act.action_density(x)
        ref = torch.from_numpy(z[f"action/{name}/density"])
        assert dens.shape == x.shape
        assert ((dens - ref).abs() / ref.abs().clamp(min=1)).max().item() < 1e-12
        tot = dens.flatten(1).sum(1)
        assert ((tot - act.action(x)).abs() / act.action(x).abs().clamp(min=1)).max().item() < 1e-12
        assert torch.allclose(tot, torch.from_numpy(z[f"action/{name}/action"]), rtol=1e-12, atol=1e-12)


def test_distconvertor_fuses_only_equal_flags():
    dc = DistConvertor_(6)
    assert [k for k, _ in dc._steps()] == ['fused']
    dc[0].propagate_density = True
    assert [k for k, _ in dc._steps()] == ['single'] * 3
    for m in dc:
        m.propagate_density = True
    assert [k for k, _ in dc._steps()] == ['fused']
    dc2 = DistConvertor_(6)
    Module_.propagate_density = True
    try:
        assert [k for k, _ in dc2._steps()] == ['fused']
    finally:
        Module_.propagate_density = False
    assert isinstance(Expit_(), Module_) and isinstance(Logit_(), Module_)


def test_new_entry_points_are_exported_and_validate():
    lib = _hip.load()
    for name in ("nf_distconv_sites", "nf_distconv_sites_vjp", "nf_phi4_action_density", "nf_phi4_action_density_vjp"):
        assert name in _hip.PROTOTYPES and hasattr(lib, name)
    x = ctypes.c_void_p(16)
    # bad mode, bad stages, NULL output: refused before any launch
    assert lib.nf_distconv_sites(x, None, 0, None, None, x, x, x, 1, 4, 1, 0, 5, None, 0, _hip.NF_F32, None) == -1
    assert b"mode" in lib.nf_last_error_string()
    assert lib.nf_distconv_sites(x, None, 0, None, None, x, x, x, 1, 4, 0, 0, 1, None, 0, _hip.NF_F32, None) == -1
    assert lib.nf_distconv_sites(x, None, 0, None, None, x, None, x, 1, 4, 1, 0, _hip.DC_SITES, None, 0,
                                 _hip.NF_F32, None) == -1
    assert lib.nf_distconv_sites_vjp(x, None, 0, None, x, x, x, None, 1, 4, 1, 0, 3, None, 0, _hip.NF_F32, None) == -1
    lat = (ctypes.c_int32 * 4)(1, 1, 0, 4)
    assert lib.nf_phi4_action_density(x, x, 1, lat, 1.0, 1.0, 1.0, _hip.NF_F32, None) == -1
    lat = (ctypes.c_int32 * 4)(1, 1, 2, 4)
    assert lib.nf_phi4_action_density_vjp(x, x, x, 1, lat, 1.0, 1.0, 1.0, 7, None) == -1
    assert lib.nf_version() == 301

"""Pade11_ / Pade22_ without a GPU: the imports, the reference's constructor signatures, parameter names and state_dict
keys (tests/golden/pade.npz holds the reference's state_dicts), the exported C entry points and their argument checks,
and the refusal of CPU tensors."""
import ctypes
import inspect
import subprocess

import numpy as np
import pytest
import torch

from normflow__amd import _hip
from normflow__amd.nn import Pade11_, Pade22_, Module_


def _cases(golden):
    z = golden("pade")
    names = sorted({k.split("/")[0] for k in z.files})
    return z, names


def _make(z, name):
    kw = dict(n_channels=int(z[f"{name}/n_channels"]), channels_axis=int(z[f"{name}/channels_axis"]))
    if int(z[f"{name}/kind"]) == 11:
        return Pade11_(**kw)
    return Pade22_(symmetric=bool(z[f"{name}/symmetric"]), **kw)


def test_pade_modules_are_exported_from_nn():
    import normflow__amd.nn as nn
    assert nn.Pade11_ is Pade11_ and nn.Pade22_ is Pade22_
    assert issubclass(Pade11_, Module_) and issubclass(Pade22_, Module_)


def test_constructor_signatures_match_the_reference():
    sig = lambda cls: [(p.name, p.default) for p in inspect.signature(cls.__init__).parameters.values()][1:]
    assert sig(Pade11_) == [('n_channels', 1), ('channels_axis', 1), ('label', 'pade11')]
    assert sig(Pade22_) == [('n_channels', 1), ('channels_axis', 1), ('symmetric', False), ('label', 'pade22')]
    m = Pade22_(4, channels_axis=-1)
    assert (m.n_channels, m.channels_axis, m.symmetric, m.label) == (4, -1, False, 'pade22')
    assert Pade11_().label == 'pade11'


def test_zero_init_and_symmetric_tie():
    m11, m22, s22 = Pade11_(3), Pade22_(3), Pade22_(3, symmetric=True)
    assert [n for n, _ in m11.named_parameters()] == ['w1'] and torch.equal(m11.w1, torch.zeros(3))
    assert [n for n, _ in m22.named_parameters()] == ['w0', 'w1']
    assert torch.equal(m22.w0, torch.zeros(3)) and torch.equal(m22.w1, torch.zeros(3))
    assert s22.w1 is s22.w0 and len(list(s22.parameters())) == 1
    assert list(s22.state_dict()) == ['w0', 'w1']


def test_reference_state_dicts_load(golden):
    z, names = _cases(golden)
    assert len(names) == 11
    for name in names:
        mod = _make(z, name)
        ref = {k.split("/", 2)[2]: torch.from_numpy(z[k]) for k in z.files if k.startswith(f"{name}/state/")}
        assert sorted(ref) == sorted(mod.state_dict()), name
        mod.load_state_dict(ref)
        for key, val in mod.state_dict().items():
            assert torch.equal(val.double(), ref[key]), (name, key)
        if getattr(mod, 'symmetric', False):
            assert mod.w1 is mod.w0


def test_cpu_tensors_raise():
    x = torch.rand(4, 3, 5)
    for mod in (Pade11_(), Pade22_(3), Pade22_(symmetric=True)):
        with pytest.raises(_hip.NormflowHipError):
            mod(x)
        with pytest.raises(_hip.NormflowHipError):
            mod.backward(x)


def test_entry_points_exported_and_no_environment_read():
    out = subprocess.run(["nm", "-D", "--defined-only", _hip.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    for name in ("nf_pade", "nf_pade_vjp", "nf_pade_workspace_bytes"):
        assert f" {name}\n" in out, name
    und = subprocess.run(["nm", "-D", "--undefined-only", _hip.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    assert "getenv" not in und
    assert _hip.load().nf_version() == 301


def test_argument_checks_without_gpu():
    lib = _hip.load()
    p = ctypes.c_void_p(16)          # never dereferenced: every call below fails its checks before any launch
    err = lambda: lib.nf_last_error_string().decode()
    assert lib.nf_pade(None, None, None, None, None, None, 1, 1, 1, 1, 22, 0, 0, None, 0, 0, None) == -1
    assert "NULL" in err()
    assert lib.nf_pade(p, p, None, None, p, p, 1, 1, 1, 4, 22, 0, 0, None, 0, 0, None) == -1     # Pade22 needs d1
    assert lib.nf_pade(p, p, p, None, p, p, 1, 1, 1, 4, 33, 0, 0, None, 0, 0, None) == -1
    assert "kind" in err()
    assert lib.nf_pade(p, p, p, None, p, p, 1, 1, 1, 4, 22, 0, 0, None, 0, 2, None) == -1       # NF_F16
    assert lib.nf_pade(p, p, p, None, p, p, 2, 3, 1, 4, 22, 0, 0, None, 0, 0, None) == -1
    assert "whole rows" in err()
    assert lib.nf_pade(p, p, p, None, p, p, 2, 2, 3, 1, 22, 0, 0, None, 0, 0, None) == -2       # no workspace
    assert "workspace" in err()
    assert lib.nf_pade_vjp(p, p, p, p, p, p, None, 1, 1, 1, 4, 22, 0, 0, None, 0, 0, None) == -1
    # 4 rows per sample with C = 3: neither a multiple of C nor one row
    assert lib.nf_pade_workspace_bytes(3, 4, 3, 2) == 0
    assert lib.nf_pade_workspace_bytes(1024, 1024, 1, 32 ** 4) > 0
    assert lib.nf_pade_workspace_bytes(0, 0, 1, 5) == 0


def test_golden_fixture_is_self_consistent(golden):
    """The fixture's per-site densities sum to its per-sample ones, and its grid holds the end points."""
    z, names = _cases(golden)
    for name in names:
        for d in ("fwd", "bwd"):
            sites, logj = z[f"{name}/{d}_sites"], z[f"{name}/{d}_logj"]
            np.testing.assert_allclose(sites.reshape(sites.shape[0], -1).sum(1), logj, rtol=1e-12, atol=1e-12)
        x = z[f"{name}/x"]
        assert x.min() == 0.0 and x.max() == 1.0 and (x == 1e-7).any() and (x == 1 - 1e-7).any()

"""The host side of nf_phi4_hmc_tiled, without a GPU: the exported symbols, what the planner answers (and that the case
list of tests/hmc_tiled_cases.py reaches every regime of the kernels, per dtype -- the check that the GPU cases mean
something), the workspace size, every NF_EINVAL of the launcher, and the sampler's own refusals of path='tiled'."""
import ctypes as C
import os

import pytest
import torch

from normflow__amd import _hip

import hmc_cases as H
import hmc_tiled_cases as TC

F32, F64 = torch.float32, torch.float64
CPU = torch.device("cpu")
_name = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v).replace("torch.", "")
LATTICES = sorted({lat for dt in (F32, F64) for lat, _ in TC.cases(dt)}) + [(32,) * 4, (48,) * 4, (32, 32, 32), (16,) * 4,
                                                                             (16384,), (2 ** 31 - 1,)]


def test_symbols_and_version():
    lib = _hip.load()
    for name in ("nf_phi4_hmc_tiled_supported", "nf_phi4_hmc_tiled_plan", "nf_phi4_hmc_tiled_workspace", "nf_phi4_hmc_tiled"):
        assert hasattr(lib, name)
    assert lib.nf_version() == 301
    header = open(os.path.join(_hip._HERE, "..", "include", "normflow_hip.h")).read()
    assert f"#define NF_HMC_TILED_MAX_LAUNCHES {_hip.HMC_TILED_MAX_LAUNCHES}\n" in header


@pytest.mark.parametrize("dtype", [F32, F64], ids=_name)
@pytest.mark.parametrize("lattice", LATTICES, ids=_name)
def test_supported_and_plan_invariants(lattice, dtype):
    assert _hip.hmc_tiled_supported(lattice, dtype) is True
    p = _hip.hmc_tiled_plan(lattice, dtype)
    # the tiles cover the lattice exactly once: n tiles of extent T reach the end of every axis and n - 1 do not
    tiles = 1
    for L, T, n in zip(lattice, p['tile'], p['ntiles']):
        assert 1 <= T <= L and n >= 1 and (n - 1) * T < L <= n * T, (L, T, n)
        tiles *= n
    assert tiles == p['tiles']
    assert p['lanes'] > 0 and p['lanes'] % 64 == 0
    assert 0 < p['lds_bytes'] <= p['lds_budget'] <= 160 * 1024
    big = [mu for mu, L in enumerate(lattice) if L > 1]
    if len(big) >= 3:
        assert p['march_axis'] == big[0] and p['ring_depth'] >= 3       # the force needs three planes at once
    else:
        assert p['march_axis'] is None and p['ring_depth'] == 0
    elem = 4 if dtype == F32 else 8
    assert p['vec'] in (1, 16 // elem) and lattice[-1] % p['vec'] == 0 and p['tile'][-1] % p['vec'] == 0


def test_not_supported():
    assert _hip.hmc_tiled_supported((16, 16), torch.float16) is False
    assert _hip.hmc_tiled_supported((2,) * 5, F32) is False
    assert _hip.hmc_tiled_supported((2 ** 16, 2 ** 15), F32) is False               # 2^31 sites
    lib = _hip.load()
    assert lib.nf_phi4_hmc_tiled_supported(_hip._lat4((4, 0)), _hip.NF_F32) == 0
    assert "extents" in lib.nf_last_error_string().decode()
    assert lib.nf_phi4_hmc_tiled_plan(_hip._lat4((4, 4)), _hip.NF_F32, None) == -1


@pytest.mark.parametrize("dtype", [F32, F64], ids=_name)
def test_the_cases_reach_every_regime(dtype):
    hit = {}
    for lattice, Cn in TC.cases(dtype):
        for r in TC.regimes(lattice, Cn, dtype):
            hit.setdefault(r, []).append(TC.case_id((lattice, Cn)))
    for r in sorted(hit):
        print(f"{_name(dtype)} {r}: {len(hit[r])} cases, e.g. {hit[r][0]}")
    assert set(hit) == TC.ALL_REGIMES, TC.ALL_REGIMES - set(hit)


@pytest.mark.parametrize("dtype", [F32, F64], ids=_name)
def test_workspace(dtype):
    lib = _hip.load()
    code = _hip.NF_F32 if dtype == F32 else _hip.NF_F64
    elem = 4 if dtype == F32 else 8
    for lattice in [(5,), (130, 130), (12, 12, 12, 12), (32,) * 4]:
        lat, V = _hip._lat4(lattice), _hip._sites(lattice)
        sizes = [lib.nf_phi4_hmc_tiled_workspace(Cn, lat, code) for Cn in (1, 2, 3, 64, 65535)]
        assert all(s > 0 for s in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[-1], sizes
        # two phi and two pi buffers and four doubles per tile
        tiles = _hip.hmc_tiled_plan(lattice, dtype)['tiles']
        assert sizes[1] >= 2 * (4 * V * elem + 32 * tiles)
        assert lib.nf_phi4_hmc_tiled_workspace(0, lat, code) == 0
    assert lib.nf_phi4_hmc_tiled_workspace(1, _hip._lat4((4, 4)), _hip.NF_F16) == 0


def _call(**over):
    """nf_phi4_hmc_tiled with valid arguments on a (4, 4) fp32 lattice except for `over`; the pointers are never followed,
    because every call here is refused before anything is launched."""
    ptr = C.c_void_p(0x1000)
    a = dict(phi=ptr, action_out=ptr, pi_in=None, pi_out=None, dh_out=ptr, accept_out=ptr, record=None, record_every=1,
             C=2, lattice=_hip._lat4((4, 4)), w0=0.5, w2=1.0, w4=0.1, n_md=3, dt=0.1, n_traj=1, force_accept=0, seed=1,
             offset=0, workspace=ptr, workspace_bytes=1 << 30, dtype=_hip.NF_F32, stream=None)
    a.update(over)
    lib = _hip.load()
    rc = lib.nf_phi4_hmc_tiled(*a.values())
    return rc, lib.nf_last_error_string().decode()


_NEED = _hip.load().nf_phi4_hmc_tiled_workspace(2, _hip._lat4((4, 4)), _hip.NF_F32)
EINVAL = [
    ("phi", dict(phi=None), "NULL"), ("action_out", dict(action_out=None), "NULL"), ("dh_out", dict(dh_out=None), "NULL"),
    ("accept_out", dict(accept_out=None), "NULL"), ("lattice", dict(lattice=None), "NULL"),
    ("C=0", dict(C=0), "C (0)"), ("C=65536", dict(C=65536), "C (65536)"),
    ("n_md=0", dict(n_md=0), "n_md (0)"), ("n_traj=0", dict(n_traj=0), "n_traj (0)"),
    ("record_every=0", dict(record_every=0), "record_every (0)"),
    ("pi_in with n_traj=2", dict(pi_in=C.c_void_p(0x1000), n_traj=2), "pi_in"),
    ("extent 0", dict(lattice=_hip._lat4((4, 0))), "extents"),
    ("2^31 sites", dict(lattice=_hip._lat4((2 ** 16, 2 ** 15))), "2^31"),
    ("fp16", dict(dtype=_hip.NF_F16), "dtype"),
    ("no workspace", dict(workspace=None), "workspace"),
    ("short workspace", dict(workspace_bytes=_NEED - 1), f"< {_NEED} B"),
    ("too many launches", dict(n_md=1022, n_traj=65), "NF_HMC_TILED_MAX_LAUNCHES"),
    ("too many workgroups", dict(lattice=_hip._lat4((48,) * 4), C=65535), "workgroups"),
]


@pytest.mark.parametrize("name,over,word", EINVAL, ids=[e[0] for e in EINVAL])
def test_argument_validation(name, over, word):
    rc, msg = _call(**over)
    assert rc == -1 and word in msg and "nf_phi4_hmc_tiled" in msg, (rc, msg)


def test_the_resident_kernel_keeps_its_answers():
    assert _hip.hmc_supported((16, 16), F32) is True and _hip.hmc_supported((32,) * 4, F32) is False
    assert "does not fit" in _hip.load().nf_last_error_string().decode()


def test_host_side_errors():
    m = H.model((4, 4), F64, CPU, **H.INTERACTING)
    with pytest.raises(_hip.NormflowHipError, match="tiled.*cpu"):
        m.hmc.sample(4, n_chains=2, path='tiled')
    with pytest.raises(_hip.NormflowHipError, match="path='tiled'"):
        m.hmc.trajectory(torch.zeros(2, 4, 4, dtype=F64), path='tiled')
    with pytest.raises(_hip.NormflowHipError, match="fused"):
        m.hmc.sample(4, n_chains=2, path='fused')
    with pytest.raises(ValueError, match="path"):
        m.hmc.sample(4, n_chains=2, path='eager')
    with pytest.raises(ValueError, match="path"):
        m.hmc.trajectory(torch.zeros(2, 4, 4, dtype=F64), path='Tiled')
    # a CPU tensor with path=None still takes the composed path
    assert m.hmc.sample(4, n_chains=2, n_md=2).shape == (4, 4, 4)

    class Other:
        def action(self, x):
            return (x ** 2).flatten(1).sum(1)
        __call__ = action
    m.action = Other()
    with pytest.raises(_hip.NormflowHipError, match="tiled.*Other"):
        m.hmc.trajectory(torch.zeros(2, 4, 4, dtype=F64), path='tiled')

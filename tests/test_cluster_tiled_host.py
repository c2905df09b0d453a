"""The tiled cluster sweep without a GPU: the exported symbols, every NF_EINVAL of the four entry points, the planner's
table, the sampler's refusal of path='tiled' on CPU tensors, the lock-free union of normflow__amd/csrc/nf_cluster_union.h
as a stand-alone host program under the sanitizers, and the tie guard of every field that tests/test_cluster_tiled.py
compares bit for bit."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from normflow__amd import _hip

import hmc_cases as H
import cluster_cases as Cc
import cluster_tiled_cases as Tc

F32, F64 = torch.float32, torch.float64
CPU = torch.device("cpu")
NEW = ("nf_phi4_cluster_tiled_supported", "nf_phi4_cluster_tiled_plan", "nf_phi4_cluster_tiled_workspace",
       "nf_phi4_cluster_tiled")
PTR = C.c_void_p(0x1000)
MAX_TILE = 32704                   # 256 + 5 x 32704 B <= 160 KiB
DEFAULT_TILE = Tc.DEFAULT_TILE


def test_symbols_are_declared_exported_and_prototyped():
    header = open(os.path.join(_hip._HERE, "..", "include", "normflow_hip.h")).read()
    declared = set(re.findall(r"\b(nf_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    lib = _hip.load()
    for name in NEW:
        assert name in declared and hasattr(lib, name) and name in _hip.PROTOTYPES, name
    assert set(_hip.PROTOTYPES) == declared
    assert lib.nf_version() == 301
    for name in ("ClusterTiledPlan", "cluster_tiled_supported", "cluster_tiled_plan", "phi4_cluster_tiled"):
        assert hasattr(_hip, name), name


def _tiled(**over):
    """nf_phi4_cluster_tiled with valid arguments on a (4, 4) fp32 lattice except for `over`; the pointers are never
    followed, because every call here is refused before anything is launched."""
    a = dict(phi=PTR, stats=PTR, labels_out=None, C=6, lattice=_hip._lat4((4, 4)), w0=0.5, seed=1, offset=0,
             dtype=_hip.NF_F32, tile_sites=0, workspace=PTR, workspace_bytes=1 << 20, stream=None)
    assert set(over) <= set(a), over
    a.update(over)
    lib = _hip.load()
    return lib.nf_phi4_cluster_tiled(*a.values()), lib.nf_last_error_string().decode()


NEED = 9 * 6 * 16 + 8 * 6          # the workspace of `_tiled`'s call
TILED_EINVAL = [
    ("phi", dict(phi=None), "NULL"), ("stats", dict(stats=None), "NULL"), ("lattice", dict(lattice=None), "NULL"),
    ("C=0", dict(C=0), "C (0)"), ("C=65536", dict(C=65536), "C (65536)"), ("fp16", dict(dtype=_hip.NF_F16), "dtype"),
    ("extent 0", dict(lattice=_hip._lat4((4, 0))), "extents"),
    ("2^31 sites", dict(lattice=_hip._lat4((2 ** 16, 2 ** 15))), "2^31"),
    ("tile above the LDS", dict(tile_sites=MAX_TILE + 1), "tile_sites"), ("tile < 0", dict(tile_sites=-1), "tile_sites"),
    ("too many tiles", dict(lattice=_hip._lat4((2 ** 15, 2 ** 15)), tile_sites=1), "tiles"),
    ("NULL workspace", dict(workspace=None), "workspace"), ("short workspace", dict(workspace_bytes=NEED - 1), "workspace"),
    ("misaligned workspace", dict(workspace=C.c_void_p(0x1004)), "aligned"),
]


@pytest.mark.parametrize("name,over,word", TILED_EINVAL, ids=[e[0] for e in TILED_EINVAL])
def test_tiled_argument_validation(name, over, word):
    rc, msg = _tiled(**over)
    assert rc == -1 and "nf_phi4_cluster_tiled" in msg and word in msg, (name, rc, msg)


def test_planner_argument_validation():
    lib = _hip.load()
    plan = _hip.ClusterTiledPlan()
    lat = _hip._lat4((4, 4))
    assert lib.nf_phi4_cluster_tiled_workspace(6, lat, 0) == NEED
    for bad in ((0, lat, 0), (65536, lat, 0), (6, None, 0), (6, _hip._lat4((4, 0)), 0), (6, lat, MAX_TILE + 1)):
        assert lib.nf_phi4_cluster_tiled_workspace(*bad) == 0, bad
    assert lib.nf_phi4_cluster_tiled_plan(lat, _hip.NF_F32, 0, None) == -1
    assert "nf_phi4_cluster_tiled_plan" in lib.nf_last_error_string().decode()
    assert lib.nf_phi4_cluster_tiled_plan(None, _hip.NF_F32, 0, C.byref(plan)) == -1
    assert lib.nf_phi4_cluster_tiled_plan(lat, _hip.NF_F16, 0, C.byref(plan)) == -1
    assert lib.nf_phi4_cluster_tiled_plan(lat, _hip.NF_F32, MAX_TILE + 1, C.byref(plan)) == -1
    assert lib.nf_phi4_cluster_tiled_supported(None, _hip.NF_F32, 0) == 0
    assert "nf_phi4_cluster_tiled_supported" in lib.nf_last_error_string().decode()
    assert lib.nf_phi4_cluster_tiled_supported(lat, _hip.NF_F32, MAX_TILE) == 1
    assert not _hip.cluster_tiled_supported((4, 4), torch.float16)
    assert not _hip.cluster_tiled_supported((2 ** 16, 2 ** 15), F32)
    with pytest.raises(_hip.NormflowHipError, match="tile_sites"):
        _hip.cluster_tiled_plan((4, 4), F32, MAX_TILE + 1)


def _lds(ts):
    return 256 + (4 * ts + 15) // 16 * 16 + (ts + 15) // 16 * 16


# (lattice, tile_sites asked): (tiles per chain, tile_sites in force, lanes); LDS = 256 B of flags, 4 ts of labels and ts of
# bond bytes, the two arrays rounded up to 16 B; workspace = 9 V per chain + 8 B of flags
PLAN = {
    ((16, 16), 64): (4, 64, 64), ((16, 16), 100): (3, 100, 128), ((3, 5), 4): (4, 4, 64), ((2, 2, 2, 2), 5): (4, 5, 64),
    ((1, 8), 3): (3, 3, 64), ((4,), 1): (4, 1, 64), ((16, 16), 0): (1, 256, 256), ((16, 16), MAX_TILE): (1, 256, 256),
    ((32, 32, 32), 0): (-(-32 ** 3 // DEFAULT_TILE), DEFAULT_TILE, 1024),
    ((16, 16, 16, 16), 0): (-(-16 ** 4 // DEFAULT_TILE), DEFAULT_TILE, 1024),
    ((32, 32, 32, 32), 0): (-(-32 ** 4 // DEFAULT_TILE), DEFAULT_TILE, 1024),
    ((48, 48, 48, 48), 0): (-(-48 ** 4 // DEFAULT_TILE), DEFAULT_TILE, 1024),
    ((48, 48, 48, 48), MAX_TILE): (-(-48 ** 4 // MAX_TILE), MAX_TILE, 1024),
}


def test_planner_table():
    assert DEFAULT_TILE in (4096, 8192, 16384)
    for (lat, ask), want in PLAN.items():
        V = int(np.prod(lat))
        for dt in (F32, F64):
            p = _hip.cluster_tiled_plan(lat, dt, ask)
            assert (p['tiles'], p['tile_sites'], p['lanes']) == want, (lat, ask, dt, p)
            assert p['lds_bytes'] == _lds(want[1]) <= 160 * 1024, (lat, ask, p)
            assert p['workspace_bytes'] == 9 * V == _hip.cluster_tiled_workspace(1, lat, ask) - 8
            assert _hip.cluster_tiled_supported(lat, dt, ask)
            for Cn in (1, 3, 70):
                assert _hip.cluster_tiled_workspace(Cn, lat, ask) == 9 * Cn * V + 8 * Cn
    assert _lds(MAX_TILE) <= 160 * 1024 < _lds(MAX_TILE + 64)
    # the existing kernel keeps its class
    for lat, dt in [((32, 32, 32), F32), ((16, 16, 16, 16), F32), ((24, 24, 24), F64)]:
        assert not _hip.cluster_supported(lat, dt) and _hip.cluster_tiled_supported(lat, dt)


def test_sampler_refuses_forced_paths_that_do_not_apply():
    m = H.model((4, 4), F64, CPU, **H.INTERACTING)
    phi = torch.zeros((2, 4, 4), dtype=F64)
    for path in ('tiled', 'kernel'):
        with pytest.raises(_hip.NormflowHipError, match="does not apply"):
            m.hmc.cluster(phi, path=path)
    with pytest.raises(ValueError, match="path"):
        m.hmc.cluster(phi, path='fused')
    torch.manual_seed(1)
    a = m.hmc.cluster(phi + 1.0, path='composed')
    torch.manual_seed(1)
    b = m.hmc.cluster(phi + 1.0)
    assert torch.equal(a['phi'], b['phi']) and torch.equal(a['labels'], b['labels'])
    with pytest.raises(_hip.NormflowHipError):
        _hip.phi4_cluster_tiled(torch.zeros((2, 4, 4)), 0.5)


def test_routing_classes_are_well_formed():
    from normflow__amd.mcmc import cluster
    assert cluster.PATHS == (None, 'kernel', 'tiled', 'composed')
    for dt, axes, least in cluster.TILED_CLASSES:
        assert dt in (F32, F64) and axes in (3, 4) and least >= 32 ** 3       # what was measured: 32^3; 16^4, 32^4, 48^4


# ---------------------------------------------------------------- the union routine, as a host program
def _compiler():
    for cxx in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    raise AssertionError("no host C++ compiler found (CXX, g++, c++, clang++)")


SANITIZERS = {"address,undefined": ["-static-libasan", "-static-libubsan"], "thread": ["-static-libtsan"]}


@pytest.mark.parametrize("sanitizer", sorted(SANITIZERS))
def test_union_program_under_the_sanitizers(sanitizer, tmp_path):
    """tests/cluster_union_main.cpp: 8 threads on std::atomic<int>, against a sequential union-find; random link lists, one
    long path, one list in which every link joins one cluster.  A stand-alone program with the sanitizer's runtime linked
    into it: it runs in the environment of the test as it is."""
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "cluster_union")
    cxx = _compiler()
    static = SANITIZERS[sanitizer] if "clang" not in os.path.basename(cxx) else ["-static-libsan"]
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", f"-fsanitize={sanitizer}",
                            "-fno-sanitize-recover=all", *static, "-pthread", os.path.join(here, "cluster_union_main.cpp"),
                            "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(run.stdout[-2000:])
    assert run.returncode == 0 and run.stdout.rstrip().endswith("PASS"), (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    assert "wrong = 0 bound hit = 0" in run.stdout and "Sanitizer" not in run.stderr, run.stderr[-4000:]


# ---------------------------------------------------------------- the tie guard of the GPU tests' fields
@pytest.mark.parametrize("lat,dt,chains", Cc.CASES, ids=[f"{'x'.join(map(str, c[0]))}-{c[1]}" for c in Cc.CASES])
def test_every_case_is_clear_of_ties(lat, dt, chains):
    assert Cc.case(lat, dt, chains)['clear']


@pytest.mark.parametrize("name", sorted(Tc.FIELDS))
def test_every_field_of_the_gpu_tests_is_clear_of_ties(name):
    """A condition, asserted here on the CPU: scale and lattice of every field are chosen so that it holds."""
    lat, w0, make = Tc.FIELDS[name]
    phi = make()
    u, _ = Cc.draws(phi.shape[0], lat, *Cc.POS)
    assert tuple(phi.shape[1:]) == tuple(lat)
    assert Cc.clear_of_ties(phi, lat, w0, u), name

"""The tiled spectrum kernel without a GPU: the exported symbols, the planner and the workspace against a written-out
table, every NF_EINVAL of the entry points with its message, the cap on the quantities, the arguments of
`measure_improved(spectrum_path=...)` and of the samplers, the refusal of CPU tensors, and the quantity descriptor of
normflow__amd/csrc/nf_cluster_spectrum_core.h as a stand-alone host program under the sanitizers."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

from normflow__amd import _hip
from normflow__amd.lib import observables as ob

import spectrum_tiled_cases as Tc

F32, F64 = torch.float32, torch.float64
NEW = ("nf_cluster_spectrum_tiled_supported", "nf_cluster_spectrum_tiled_plan", "nf_cluster_spectrum_tiled_workspace",
       "nf_cluster_spectrum_tiled")
PTR = C.c_void_p(0x1000)
NF_EINVAL = -1                     # include/normflow_hip.h


def _kmax(momenta):
    return 0 if momenta == 'all' else momenta


def test_symbols_are_declared_exported_and_prototyped():
    header = open(os.path.join(_hip._HERE, "..", "include", "normflow_hip.h")).read()
    declared = set(re.findall(r"\b(nf_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    lib = _hip.load()
    for name in NEW:
        assert name in declared and hasattr(lib, name) and name in _hip.PROTOTYPES, name
    assert set(_hip.PROTOTYPES) == declared
    assert "nf_spectrum_tiled_plan" in header
    for name in ("SpectrumTiledPlan", "cluster_spectrum_tiled_supported", "cluster_spectrum_tiled_plan",
                 "cluster_spectrum_tiled_workspace", "cluster_spectrum_tiled_per_pass", "cluster_spectrum_tiled"):
        assert hasattr(_hip, name), name
    assert lib.nf_version() == 301                           # an added entry point leaves the version
    csrc = os.path.join(_hip._HERE, "csrc")
    assert "nf_cluster_spectrum_core.h" in open(os.path.join(csrc, "Makefile")).read()
    for user in ("nf_cluster_spectrum.hip", "nf_cluster_spectrum_tiled.hip"):            # the descriptor is stated once
        text = open(os.path.join(csrc, user)).read()
        assert '#include "nf_cluster_spectrum_core.h"' in text and "struct CsQuantity" not in text, user


PLAN_IDS = [f"{'x'.join(map(str, k[0]))}-k{k[1]}-b{k[2]}-p{k[3]}" for k in Tc.PLAN]


@pytest.mark.parametrize("lat,momenta,bs,pp", list(Tc.PLAN), ids=PLAN_IDS)
def test_planner_and_workspace_against_the_table(lat, momenta, bs, pp):
    blocks, bsf, Q, cols, ppf, passes, launches = Tc.PLAN[(lat, momenta, bs, pp)]
    K4 = (0,) * (4 - len(lat)) + Tc.kmax_of(lat, momenta)
    for dt in (F32, F64):
        assert _hip.cluster_spectrum_tiled_supported(lat, dt, momenta, bs)
        p = _hip.cluster_spectrum_tiled_plan(lat, dt, momenta, bs, pp)
        assert p == dict(blocks=blocks, block_sites=bsf, kmax=K4, columns=cols, quantities=Q, per_pass=ppf, passes=passes,
                         table_entries=Tc.TABLE, launches=launches, lds_bytes=Tc.lds(ppf)), p
    # the table against the formulas it was written from
    V = Tc.volume(lat)
    assert bsf == min(bs or Tc.DEFAULT_BLOCK, V) and blocks == -(-V // bsf)
    assert Q == Tc.quantities(lat, momenta) and cols == Tc.columns(lat, momenta)
    assert ppf == (pp or min(Q, Tc.MAX_PASS)) and passes == -(-Q // ppf) and launches == 2 + 2 * passes
    for chains in (1, 3, 300, 65535):
        need = _hip.cluster_spectrum_tiled_workspace(chains, lat, momenta, bs, pp)
        assert need == Tc.workspace(chains, lat, momenta, bs, pp) and need % 8 == 0, (chains, need)
        # the flags, per_pass C V 8 bytes of slots, C (Q + 1) blocks doubles of partials
        assert need == -(-4 * chains // 16) * 16 + ppf * chains * V * 8 + chains * (Q + 1) * blocks * 8


@pytest.mark.parametrize("chains,lat", sorted(Tc.DEFAULT_PER_PASS))
def test_default_per_pass_is_a_footprint_policy(chains, lat, monkeypatch):
    monkeypatch.delenv("NF_MOMENTS_MAX_WORKSPACE", raising=False)
    want = Tc.DEFAULT_PER_PASS[(chains, lat)]
    cap = min(Tc.quantities(lat, 'all'), Tc.MAX_PASS)
    assert _hip.cluster_spectrum_tiled_per_pass(chains, lat) == want
    if want < cap:                                           # the largest that stays under the limit, and at least 1
        assert Tc.workspace(chains, lat, 'all', 0, want + 1) > 1 << 30
    assert want == 1 or Tc.workspace(chains, lat, 'all', 0, want) <= 1 << 30
    monkeypatch.setenv("NF_MOMENTS_MAX_WORKSPACE", "1")
    assert _hip.cluster_spectrum_tiled_per_pass(chains, lat) == 1
    monkeypatch.setenv("NF_MOMENTS_MAX_WORKSPACE", str(1 << 50))
    assert _hip.cluster_spectrum_tiled_per_pass(chains, lat) == cap
    assert _hip.cluster_spectrum_tiled_per_pass(chains, lat, 1) == min(Tc.quantities(lat, 1), Tc.MAX_PASS)


def _call(**over):
    """nf_cluster_spectrum_tiled with valid arguments on a (4, 4) fp32 lattice at all momenta except for `over`; the
    pointers are never followed, because every call here is refused before anything is launched."""
    a = dict(phi=PTR, labels=PTR, out=PTR, status=PTR, C=6, lattice=_hip._lat4((4, 4)), kmax=0, tw=PTR, dtype=_hip.NF_F32,
             block_sites=0, per_pass=0, workspace=PTR, workspace_bytes=1 << 20, stream=None)
    assert set(over) <= set(a), over
    a.update(over)
    lib = _hip.load()
    return lib.nf_cluster_spectrum_tiled(*a.values()), lib.nf_last_error_string().decode()


NEED = 32 + 7 * 6 * 16 * 8 + 6 * 8 * 1 * 8          # the workspace of `_call`'s call: Q = 1 + 2 x 3 = 7, one block
EINVAL = [
    ("phi", dict(phi=None), "NULL"), ("labels", dict(labels=None), "NULL"), ("out", dict(out=None), "NULL"),
    ("status", dict(status=None), "NULL"), ("tw", dict(tw=None), "tw is NULL"), ("lattice", dict(lattice=None), "lattice is NULL"),
    ("C=0", dict(C=0), "C (0)"), ("C=65536", dict(C=65536), "C (65536)"), ("fp16", dict(dtype=_hip.NF_F16), "dtype"),
    ("extent 0", dict(lattice=_hip._lat4((4, 0))), "extents"),
    ("2^31 sites", dict(lattice=_hip._lat4((2 ** 16, 2 ** 15)), kmax=1), "2^31"),
    ("kmax < 0", dict(kmax=-1), "kmax (-1)"),
    ("block < 0", dict(block_sites=-1), "block_sites"),
    ("too many blocks", dict(lattice=_hip._lat4((2 ** 15, 2 ** 15)), kmax=1, block_sites=1), "blocks"),
    ("per_pass < 0", dict(per_pass=-1), "per_pass"), ("per_pass above the quantities", dict(per_pass=8), "per_pass (8)"),
    ("per_pass above 16", dict(lattice=_hip._lat4((16, 16)), per_pass=17), "per_pass (17)"),
    ("too many quantities", dict(lattice=_hip._lat4((4096, 4096))), "kmax"),
    ("no workspace", dict(workspace=None), f"workspace is NULL ({NEED} B needed)"),
    ("short workspace", dict(workspace_bytes=NEED - 1), f"too small, {NEED} B needed"),
    ("misaligned workspace", dict(workspace=C.c_void_p(0x1008)), "aligned"),
]


@pytest.mark.parametrize("name,over,words", EINVAL, ids=[e[0] for e in EINVAL])
def test_every_refusal_states_its_reason(name, over, words):
    rc, msg = _call(**over)
    assert rc == NF_EINVAL and words in msg and "nf_cluster_spectrum_tiled" in msg, (rc, msg)


def test_workspace_of_the_refusal_table_and_the_pure_host_refusals():
    assert _hip.cluster_spectrum_tiled_workspace(6, (4, 4)) == NEED == Tc.workspace(6, (4, 4), 'all', 0, 0)
    lib = _hip.load()
    for chains in (0, 65536):
        assert _hip.cluster_spectrum_tiled_workspace(chains, (4, 4)) == 0
    assert _hip.cluster_spectrum_tiled_workspace(2, (4, 4), per_pass=8) == 0
    assert _hip.cluster_spectrum_tiled_workspace(2, (16, 16), per_pass=17) == 0
    assert _hip.cluster_spectrum_tiled_workspace(2, (2 ** 16, 2 ** 15), 1) == 0
    assert not _hip.cluster_spectrum_tiled_supported((4, 4), torch.float16)
    assert not _hip.cluster_spectrum_tiled_supported((2 ** 16, 2 ** 15), F32, 1)
    assert "2^31" in lib.nf_last_error_string().decode()
    assert not _hip.cluster_spectrum_tiled_supported((2 ** 15, 2 ** 15), F32, 1, 64)          # 2^24 blocks x 256 = 2^32
    assert "blocks" in lib.nf_last_error_string().decode()
    assert _hip.cluster_spectrum_tiled_supported((2 ** 15, 2 ** 15), F32, 1, 65)
    with pytest.raises(_hip.NormflowHipError, match="per_pass"):
        _hip.cluster_spectrum_tiled_plan((4, 4), F32, 'all', 0, 8)
    assert lib.nf_cluster_spectrum_tiled_plan(_hip._lat4((4, 4)), _hip.NF_F32, 0, 0, 0, None) == NF_EINVAL
    assert lib.nf_cluster_spectrum_tiled_plan(None, _hip.NF_F32, 0, 0, 0, C.byref(_hip.SpectrumTiledPlan())) == NF_EINVAL
    with pytest.raises(_hip.NormflowHipError, match="block_sites"):
        _hip.cluster_spectrum_tiled_plan((4, 4), F32, 'all', -3)
    with pytest.raises(_hip.NormflowHipError, match="momenta"):
        _hip.cluster_spectrum_tiled_plan((4, 4), F32, 0)


def test_the_cap_on_the_quantities_names_kmax():
    """(4096, 4096) at 'all' has 1 + 2 x 4095 = 8191 quantities: refused, with kmax as the remedy; at momenta 4 it has 17."""
    lib = _hip.load()
    assert not _hip.cluster_spectrum_tiled_supported((4096, 4096), F32, 'all')
    msg = lib.nf_last_error_string().decode()
    assert "kmax" in msg and "8191" in msg and str(Tc.MAX_Q) in msg, msg
    assert _hip.cluster_spectrum_tiled_workspace(1, (4096, 4096), 'all') == 0
    with pytest.raises(_hip.NormflowHipError, match="kmax"):
        _hip.cluster_spectrum_tiled_plan((4096, 4096), F32, 'all')
    assert _hip.cluster_spectrum_tiled_supported((4096, 4096), F32, 4)
    p = _hip.cluster_spectrum_tiled_plan((4096, 4096), F64, 4)
    assert p['quantities'] == 17 and p['columns'] == 10 and p['passes'] == 2 and p['blocks'] == 4096
    # the largest 1-d lattice under the cap, and the first above it
    assert _hip.cluster_spectrum_tiled_plan((1024,), F32, 'all')['quantities'] == 1024
    assert not _hip.cluster_spectrum_tiled_supported((1025,), F32, 'all')


def test_measure_improved_arguments():
    assert ob.IMPROVED_PATHS == (None, 'kernel', 'composed', 'hbm')
    phi, lab = torch.zeros((2, 4, 4)), torch.zeros((2, 4, 4), dtype=torch.int32)
    with pytest.raises(ValueError, match="momenta"):                  # the path of the spectrum needs momenta
        ob.measure_improved(phi, lab, spectrum_path='hbm')
    with pytest.raises(ValueError, match="momenta"):
        ob.measure_improved(phi, lab, path='hbm', spectrum_path='hbm')
    for path in ('kernel', 'composed'):
        with pytest.raises(ValueError, match="spectrum_path"):
            ob.measure_improved(phi, lab, path=path, momenta='all', spectrum_path='hbm')
    with pytest.raises(ValueError, match="spectrum_path"):
        ob.measure_improved(phi, lab, momenta='all', spectrum_path='HBM')
    with pytest.raises(ValueError, match="momenta"):
        ob.measure_improved(phi, lab, momenta=0, spectrum_path='hbm')
    ws = torch.empty(256, dtype=torch.uint8)
    for kw in (dict(), dict(momenta='all'), dict(path='hbm'), dict(path='composed', momenta=1)):      # a workspace no path takes
        with pytest.raises(ValueError, match="workspace"):
            ob.measure_improved(phi, lab, workspace=ws, **kw)
    for path in (None, 'hbm'):                                        # no quiet fall-back
        with pytest.raises(_hip.NormflowHipError):
            ob.measure_improved(phi, lab, path=path, momenta='all', spectrum_path='hbm')
    with pytest.raises(_hip.NormflowHipError):
        _hip.cluster_spectrum_tiled(phi, lab)
    # the pinned error still raises, and now points to the keyword
    with pytest.raises(ValueError, match="hbm") as e:
        ob.measure_improved(phi, lab, path='hbm', momenta='all')
    assert "spectrum_path='hbm'" in str(e.value)
    # without the keyword: what it did (the composed path on CPU tensors)
    im = ob.measure_improved(phi, lab, momenta='all')
    assert im.momenta == (2, 2) and (im.status == 0).all()
    assert ob.route_improved(torch.zeros((1, 32, 32, 32))) == 'composed'


def test_sampler_arguments():
    import hmc_cases as H
    from normflow__amd.action import ScalarPhi4Ladder
    from normflow__amd.mcmc.hmc import HMCSampler
    from normflow__amd.mcmc.ladder import LadderHMCSampler
    for cls in (HMCSampler, LadderHMCSampler):
        assert cls._spectrum_path(None, None, False) is None and cls._spectrum_path('hbm', 'all', None) is None
        assert cls._spectrum_path('hbm', 2, 'hbm') is None
        with pytest.raises(ValueError, match="momenta"):
            cls._spectrum_path('hbm', None, None)
        with pytest.raises(ValueError, match="spectrum_path"):
            cls._spectrum_path('tiled', 'all', None)
        for ipath in ('kernel', 'composed', False):
            with pytest.raises(ValueError, match="improved"):
                cls._spectrum_path('hbm', 'all', ipath)
    m = H.model((4, 4), F32, 'cpu', **H.INTERACTING)
    lad = m.hmc.ladder(ScalarPhi4Ladder(kappa=(0.3, 0.5), m_sq=-2.68, lambd=0.5))
    for s, C_ in ((m.hmc, 2), (lad, 2)):
        s.start(n_chains=C_)
        before = s._ref['sample'].clone()
        with pytest.raises(ValueError, match="momenta"):
            s.measure(C_ * 2, n_chains=C_, n_md=2, dt=0.1, cluster_every=1, improved=True, spectrum_path='hbm')
        with pytest.raises(ValueError, match="improved"):
            s.measure(C_ * 2, n_chains=C_, n_md=2, dt=0.1, cluster_every=1, improved='composed', momenta='all',
                      spectrum_path='hbm')
        with pytest.raises(_hip.NormflowHipError):                   # chains on the CPU: no quiet fall-back
            s.measure(C_ * 2, n_chains=C_, n_md=2, dt=0.1, cluster_every=1, improved=True, momenta='all', spectrum_path='hbm')
        assert torch.equal(s._ref['sample'], before)


# ---------------------------------------------------------------- the quantity descriptor, as a host program
def _compiler():
    for cxx in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    raise AssertionError("no host C++ compiler found (CXX, g++, c++, clang++)")


def test_core_program_under_the_sanitizers(tmp_path):
    """tests/cluster_spectrum_core_main.cpp: cs_layout and cs_quantity of nf_cluster_spectrum_core.h against a brute-force
    enumeration of the rule, for every lattice with extents in 1 .. 9 and every kmax in 0 .. 5.  A stand-alone program
    with the sanitizers' runtime linked into it: it runs in the environment of the test as it is."""
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "cluster_spectrum_core")
    cxx = _compiler()
    static = ["-static-libasan", "-static-libubsan"] if "clang" not in os.path.basename(cxx) else ["-static-libsan"]
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", *static, os.path.join(here, "cluster_spectrum_core_main.cpp"),
                            "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(run.stdout[-2000:])
    assert run.returncode == 0 and run.stdout.rstrip().endswith("PASS"), (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    assert "lattices = 6561 " in run.stdout and "wrong = 0" in run.stdout and "Sanitizer" not in run.stderr, run.stderr[-4000:]
    assert "MISMATCH" not in run.stdout

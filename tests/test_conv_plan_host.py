"""nf_conv_plan on the host: the convolution dispatcher's decisions, held to a recorded table.

tests/golden/conv_plan.json holds, for every layer of the grid in tests/conv_plan_cases.py, what the dispatcher decided
when planning and launching were still one function (tests/golden/make_golden_conv_plan.py says how it was recorded):
kernel path, weight layout, MT, two-site and packed modes, box, plane stride, channels per pass, LDS bytes, log-det
partials per sample and launches, or the return code and the start of the message of a refusal.  nf_conv_plan is the
planner the launchers execute, so a change of any decision shows here as a changed row, without a GPU.

The table must also hold every branch of the planner at least once: a pruned grid must not hide one."""
import ctypes as C
import json
import os
import re

import pytest
import torch

from normflow__amd import _hip

import conv_plan_cases as G

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_plan.json")


@pytest.fixture(scope="module")
def table():
    with open(GOLDEN) as f:
        doc = json.load(f)
    cases = G.cases()
    assert len(doc["case_plan"]) == len(cases) and 2000 <= len(cases) <= 9999
    return doc, cases


def test_symbol_header_and_binding():
    header = open(os.path.join(_hip._HERE, "..", "include", "normflow_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _hip.load()
    assert hasattr(lib, "nf_conv_plan")
    args = re.search(r"\bint\s+nf_conv_plan\s*\(([^)]*)\)", code).group(1).split(",")
    kinds = [C.POINTER(C.c_int32) if "int32_t" in a else C.c_void_p if "*" in a else C.c_int64 if "int64_t" in a else C.c_int
             for a in args]
    assert (C.c_int, kinds) == tuple(_hip.PROTOTYPES["nf_conv_plan"])
    body = re.search(r"typedef struct nf_conv_layer_plan \{(.*?)\} nf_conv_layer_plan;", code, flags=re.S).group(1)
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64}
    fields = [(n, ctype[t] * 4 if dim else ctype[t]) for t, n, dim in re.findall(r"(int32_t|int64_t)\s+(\w+)(\[4\])?;", body)]
    assert fields == list(_hip.ConvPlan._fields_)
    assert lib.nf_version() == 301
    out = _hip.ConvPlan()
    lat4, k4 = _hip._lat4([8, 8], [3, 3])
    assert lib.nf_conv_plan(lat4, k4, 8, 8, 0, 0, _hip.NF_F32, 1, None) == -1 and b"NULL" in lib.nf_last_error_string()
    assert lib.nf_conv_plan(None, k4, 8, 8, 0, 0, _hip.NF_F32, 1, C.byref(out)) == -1 and b"NULL" in lib.nf_last_error_string()


def test_the_grid_has_the_axes():
    cases = G.cases()
    axis = lambda i: {c[i] for c in cases}
    assert {(8, 8, 8, 16), (4, 4, 4, 32), (2, 2, 2, 64), (6, 6, 6, 48), (32,) * 4, (48,) * 4, (5, 7, 9)} <= axis(0)
    assert {len(lat) for lat in axis(0)} == {1, 2, 3, 4}
    assert axis(1) == {(1,) * 4, (3,) * 4, (5,) * 4, (3, 3, 3, 5)}
    assert {1, 2, 6, 8, 12, 16} <= axis(2) and {1, 8, 20, 46, 52} <= axis(3)
    assert axis(4) == {0, 1, 2} and axis(5) == {0, 1, 3, 7} and axis(6) == {_hip.NF_F32, _hip.NF_F64}
    assert axis(7) == {0, 1, 2} and axis(8) == {1, 65535}
    assert G.OPTIONS == [dict(split16=True, pipe=True), dict(split16=False, pipe=True), dict(split16=False, pipe=False)]


def test_the_table_has_every_branch(table):
    doc, cases = table
    col = {name: i for i, name in enumerate(doc["columns"])}
    rows = [(case, doc["plans"][i]) for case, i in zip(cases, doc["case_plan"])]
    ok = [(c, p) for c, p in rows if p[0] == 0]
    refused = [(c, doc["messages"][p[1]]) for c, p in rows if p[0] != 0]
    get = lambda p, name: p[col[name]]
    assert {get(p, "path") for _, p in ok} == {0, 1, 2, 3}
    assert {get(p, "mt") for _, p in ok if get(p, "path") != 3} == {2, 4}
    assert any(get(p, "two_site") for _, p in ok) and any(get(p, "packed") for _, p in ok)
    assert any(get(p, "path") == 0 and not get(p, "packed") and get(p, "channels_per_pass") < ((c[2] + 3) & ~3)
               for c, p in ok), "chunked channels"
    assert any(c[3] == 52 and get(p, "launches") == 2 for c, p in ok), "more than one one-box launch"
    assert all(get(p, "launches") == (1 if get(p, "path") else (((c[3] + 15) >> 4) + 2) // 3) for c, p in ok)
    assert any(c[0][-1] == 48 and get(p, "box3") == 16 and get(p, "nbox3") == 3 for c, p in ok), "the 48-wide box"
    assert any(c[8] == 65535 and "batch x boxes >= 2^" in m for c, m in refused), "too many items"
    assert any("input box needs" in m for c, m in refused), "LDS"
    assert any(c[5] == 7 and m.startswith("nf_conv_rqs: split-fp16 input") for c, m in refused), "split-fp16 input"
    assert any(c[5] and c[6] == _hip.NF_F64 and "unsupported dtype" in m for c, m in refused), "fp64 fused"
    assert all(p[0] in (0, -1) for _, p in rows)
    assert all((get(p, "partials") > 0) == bool(c[5]) for c, p in ok)


def test_nf_conv_plan_gives_the_recorded_plans(table):
    doc, cases = table
    messages = list(doc["messages"])
    wrong = []
    for case, i in zip(cases, doc["case_plan"]):
        got = G.plan_of(case, messages)
        if got != doc["plans"][i]:
            wrong.append((case, got, doc["plans"][i]))
    assert messages == doc["messages"], messages[len(doc["messages"]):]
    assert not wrong, (len(wrong), wrong[:5])


def test_weight_layout_is_the_plans(table):
    """nf_conv_weight_layout is nf_conv_plan's weight_layout at batch 1 (-1 for a refused layer), except that a pair-tensor
    layer (fused bit 2) the split-fp16 kernel does not take is answered as the same layer on fp32 planes."""
    doc, cases = table
    lib = _hip.load()
    col = doc["columns"].index("weight_layout")
    by_case = {c: doc["plans"][i] for c, i in zip(cases, doc["case_plan"])}
    n = 0
    for case, plan in by_case.items():
        lat, k, cin, cout, compact, fused, dtype, opt, B = case
        if B != 1:
            continue
        if plan[0] and fused == 7:
            plan = by_case[(lat, k, cin, cout, compact, 3, dtype, opt, B)]
        lat4, k4 = _hip._lat4(list(lat), list(k[4 - len(lat):]))
        with _hip.options(**G.OPTIONS[opt]):
            got = lib.nf_conv_weight_layout(lat4, k4, cin, cout, compact, fused, dtype)
        assert got == (-1 if plan[0] else plan[col]), case
        n += 1
    assert n > 1000


def test_conv_plan_wrapper():
    p = _hip.conv_plan((4, 4, 4, 32), (3, 3, 3, 3), 8, 46, compact=1, fused=3, B=5)
    assert p["path"] == 3 and p["weight_layout"] == 2 and p["box"] == [2, 2, 2, 32] and p["partials"] == 8
    assert set(p) == {n for n, _ in _hip.ConvPlan._fields_}
    with pytest.raises(_hip.NormflowHipError, match="split the batch"):
        _hip.conv_plan((48,) * 4, (3,) * 4, 8, 20, B=65535)
    with pytest.raises(_hip.NormflowHipError, match="1 to 4 axes"):
        _hip.conv_plan((4,) * 5, (3,) * 5, 8, 8)
    assert _hip.conv_plan((8, 8), (3, 3), 8, 8, dtype=torch.float64)["path"] == 0

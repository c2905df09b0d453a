"""Host side of tests/test_batch_slabs.py (no GPU): every function of normflow__amd/_hip.py that cuts its batch with
`_slabs(` has a crossing-batch test in the case table of tests/batch_slab_cases.py, and every test the table names
exists.  A new slab loop then cannot arrive untested."""
import ast
import os

from normflow__amd import _hip

import batch_slab_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _slab_loops():
    """qualified name -> number of `_slabs(...)` calls, for every function of _hip.py that makes one."""
    tree = ast.parse(open(os.path.join(ROOT, "normflow__amd", "_hip.py")).read())
    found = {}

    def visit(node, prefix):
        for child in ast.iter_child_nodes(node):
            if isinstance(child, ast.ClassDef):
                visit(child, prefix + child.name + ".")
            elif isinstance(child, (ast.FunctionDef, ast.AsyncFunctionDef)):
                n = sum(1 for c in ast.walk(child)
                        if isinstance(c, ast.Call) and isinstance(c.func, ast.Name) and c.func.id == "_slabs")
                if n:
                    found[prefix + child.name] = n
                visit(child, prefix + child.name + ".")
            else:
                visit(child, prefix)
    visit(tree, "")
    return found


def _device_tests():
    tree = ast.parse(open(os.path.join(ROOT, "tests", "test_batch_slabs.py")).read())
    return {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}


def test_every_slab_loop_has_a_crossing_batch_test():
    loops = _slab_loops()
    assert sum(loops.values()) >= 26 and "normal_sample" in loops and "MultiRQSCouplingFn.backward" in loops, loops
    missing = sorted(set(loops) - set(S.COVERED))
    assert not missing, f"_hip.py functions with a `_slabs(` loop and no case in batch_slab_cases.COVERED: {missing}"
    stale = sorted(set(S.COVERED) - set(loops))
    assert not stale, f"batch_slab_cases.COVERED names functions without a `_slabs(` loop: {stale}"


def test_the_case_table_names_existing_tests():
    tests = _device_tests()
    named = {t for ts in S.COVERED.values() for t in ts}
    named |= {t for ts in S.NO_LOOP.values() for t in ((ts,) if isinstance(ts, str) else ts)}
    assert named <= tests, sorted(named - tests)
    for name in S.NO_LOOP:
        assert hasattr(_hip, name), name


def test_batch_sizes_cross_the_limits():
    """B2: two slabs with a ragged tail; B3: three slabs, beyond the C entry points' 65535 rows, two slabs of rqs_knots."""
    assert [b1 - b0 for b0, b1 in _hip._slabs(S.B2)] == [_hip.MAX_B, 5]
    assert [b1 - b0 for b0, b1 in _hip._slabs(S.B3)] == [_hip.MAX_B, _hip.MAX_B, 3] and S.B3 > 65535
    assert [b1 - b0 for b0, b1 in _hip._slabs(S.B3, 65535)] == [65535, 4]
    assert S.rows_R(S.B2) == [0, 1, _hip.MAX_B - 2, _hip.MAX_B - 1, _hip.MAX_B, _hip.MAX_B + 1, S.B2 - 1]
    assert set(S.rows_R(S.B3)) >= {2 * _hip.MAX_B - 1, 2 * _hip.MAX_B, 65535, S.B3 - 1}


def test_slabs_read_max_b_when_called(monkeypatch):
    """`_slabs` and `_workspace(min(B, MAX_B), ...)` read the same MAX_B: the default step is not frozen at definition."""
    monkeypatch.setattr(_hip, "MAX_B", 7)
    assert list(_hip._slabs(16)) == [(0, 7), (7, 14), (14, 16)]

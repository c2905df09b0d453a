"""The batch-slab helpers every entry point of normflow__amd._hip cuts its batch with.  Host only: no GPU, no library."""
import pytest
import torch

from normflow__amd import _hip


@pytest.mark.parametrize("step", [None, 7])
def test_slabs_cover_the_batch_exactly(step):
    """For B in {0, 1, step, step + 1, 2 step + 5}: the slabs are contiguous, ordered, non-empty, cover [0, B) exactly and
    never exceed `step` (default: MAX_B)."""
    n = _hip.MAX_B if step is None else step
    for B in (0, 1, n, n + 1, 2 * n + 5):
        slabs = list(_hip._slabs(B) if step is None else _hip._slabs(B, step))
        assert len(slabs) == -(-B // n)                    # none for an empty batch
        end = 0
        for b0, b1 in slabs:
            assert b0 == end and b0 < b1 <= B and b1 - b0 <= n
            end = b1
        assert end == B


def test_slab_of_an_optional_tensor():
    t = torch.arange(10)
    assert torch.equal(_hip._slab(t, 3, 7), t[3:7])
    assert _hip._slab(t, 3, 7).data_ptr() == t[3:7].data_ptr()      # a view: the kernels write through it
    assert _hip._slab(None, 3, 7) is None

"""The parity-compact first layer (nf_conv_c.hip, conv_c3_kernel), host side: the fragment packer
`_hip.pack_conv_weight_split16_first_parity` against a plain statement of the layout in include/normflow_hip.h, and the
frozen-parity flags of `nf_conv_first_split16_supported`.  No GPU."""
import itertools

import pytest
import torch

import normflow__amd  # noqa: F401
from normflow__amd import _hip

SCALE = 1024.0


def expected_entry(w, sigma, n, r, tp):
    """The scaled fp32 weight that column n = 8*shift + co multiplies at live tap t' of kernel row r for row-parity
    class sigma, and whether the layout rule names the entry (tap inside the 3-tap kernel, row < 27)."""
    shift, co = divmod(n, 8)
    if r >= 27:
        return 0.0, False
    j0, j1, j2 = r // 9, (r // 3) % 3, r % 3
    e = sigma ^ ((j0 + j1 + j2 + 1) & 1)
    t = 1 - e + 2 * tp                      # the live taps of the pair's four (sites 2p - 1 .. 2p + 2)
    j3 = t - shift
    if not 0 <= j3 <= 2:
        return 0.0, False
    return float(w[co, 0, j0, j1, j2, j3]) * SCALE, True


@pytest.fixture(scope="module")
def packed():
    g = torch.Generator(device='cpu').manual_seed(11)
    w = 0.3 * torch.randn((8, 1, 3, 3, 3, 3), generator=g, device='cpu')
    w[w == 0] = 0.25                        # every kernel entry non-zero: a zero in the blob is then the layout's
    return w, _hip.pack_conv_weight_split16_first_parity(w)


def test_blob_shape_and_dense_part(packed):
    w, blob = packed
    assert blob.dtype == torch.float16 and tuple(blob.shape) == (16, 64, 8) and blob.is_contiguous()
    assert torch.equal(blob[:8], _hip.pack_conv_weight_split16_first(w).reshape(8, 64, 8))


@pytest.mark.parametrize("sigma", [0, 1])
def test_parity_fragments_follow_the_layout(packed, sigma):
    w, blob = packed
    frag = blob[8:].reshape(2, 2, 2, 64, 8).float()          # sigma, slice, hi|lo, lane, value
    named = 0
    for sl, g, n, h, tp in itertools.product(range(2), range(4), range(16), range(4), range(2)):
        r = 16 * sl + 4 * g + h
        want, live = expected_entry(w, sigma, n, r, tp)
        hi = float(frag[sigma, sl, 0, 16 * g + n, 2 * h + tp])
        lo = float(frag[sigma, sl, 1, 16 * g + n, 2 * h + tp])
        if not live:
            assert hi == 0.0 and lo == 0.0, (sigma, sl, g, n, h, tp)
            continue
        named += 1
        assert hi != 0.0, (sigma, sl, g, n, h, tp)           # exactly the (row, tap) entries the rule names are non-zero
        assert hi == float(torch.tensor(want, device='cpu').half())         # hi = fp16(scaled weight)
        # hi + lo reproduces the scaled weight to the accuracy of the split: lo = fp16(w - hi), |w - hi| <= 2^-11 |w|,
        # so the residue is at most 2^-11 of that again (or fp16's smallest subnormal, 2^-24, for tiny lo)
        assert abs(hi + lo - want) <= max(abs(want) * 2.0 ** -22, 2.0 ** -24), (hi, lo, want)
    # per (row < 27, column): kernel taps j3 = t - shift with t in the live pair: 3 of the 4 (shift, t') combinations fall
    # inside 0..2 in total for the two shifts
    assert named == 27 * 8 * 3


def test_both_sets_cover_the_kernel(packed):
    """Between the two sigma sets and the two shifts every kernel entry W[co][r][j3] appears, at the tap the rule names."""
    w, blob = packed
    frag = blob[8:].reshape(2, 2, 2, 64, 8).float()
    seen = set()
    for sigma, n, r, tp in itertools.product(range(2), range(16), range(27), range(2)):
        want, live = expected_entry(w, sigma, n, r, tp)
        if live:
            e = sigma ^ ((r // 9 + (r // 3) % 3 + r % 3 + 1) & 1)
            seen.add((n % 8, r, 1 - e + 2 * tp - n // 8))
    assert seen == set(itertools.product(range(8), range(27), range(3)))
    assert not torch.equal(frag[0], frag[1])


def test_supported_accepts_the_flags_and_leaves_unflagged_answers():
    lib = _hip.load()
    T, S = _hip.ACT_CODES['tanh'], _hip.ACT_CODES['expit']
    k4 = _hip._lat4((3, 3, 3, 3))
    even, odd = _hip.FIRST_FROZEN_FLAG
    assert (even, odd) == (0x100, 0x200) and _hip.FIRST_PARITY_FRAGS == 16 << 16
    for lat in ((4, 4, 4, 32), (2, 2, 4, 32), (4, 4, 4, 48), (8, 4, 6, 64), (4, 4, 4, 20), (4, 4, 3, 32), (1, 1, 1, 32)):
        lat4 = _hip._lat4(lat)
        for act in (T, S, 0, 2, 5):
            plain = lib.nf_conv_first_split16_supported(lat4, k4, 8, act)
            assert plain == (1 if act in (T, S) and lat in ((4, 4, 4, 32), (2, 2, 4, 32), (4, 4, 4, 48), (8, 4, 6, 64)) else 0)
            for flag in (even, odd, even | _hip.FIRST_PARITY_FRAGS, odd | _hip.FIRST_PARITY_FRAGS):
                assert lib.nf_conv_first_split16_supported(lat4, k4, 8, act | flag) == plain, (lat, act, hex(flag))
            assert lib.nf_conv_first_split16_supported(lat4, k4, 8, act | even | odd) == 0      # both parities: no such field
            assert lib.nf_conv_first_split16_supported(lat4, k4, 8, act | 0x400) == 0           # an unknown bit is no activation
    assert lib.nf_conv_first_split16_supported(_hip._lat4((4, 4, 4, 32)), k4, 4, T | even) == 0  # 8 channels only

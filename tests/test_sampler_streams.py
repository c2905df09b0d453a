"""The one Philox draw of the samplers, bitwise: the momenta of nf_phi4_hmc and nf_phi4_hmc_tiled and the proposal of
nf_block_propose on the whole field ARE the draw of nf_normal_sample at the same position (csrc/nf_sampler_core.h), where
the trajectory tests of tests/test_hmc.py and tests/test_hmc_tiled.py see a misplaced momentum only through a tolerance."""
import pytest
import torch

from normflow__amd import _hip

import hmc_cases as H
from hmc_cases import DEV

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
_name = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v).replace("torch.", "")


def _normal_sample_at(pos, C, shape, dtype):
    gen = torch.Generator(device=DEV)
    gen.manual_seed(pos[0])
    gen.set_offset(4 * pos[1])
    return _hip.normal_sample(None, None, C, shape, dtype, DEV, generator=gen)[0]


# (5, 7, 9): 315 sites, the last group is cut in both dtypes, no row is a multiple of a group and the tiled kernel draws
# site by site; (4, 4): the 16-byte path of the tiled kernel, one whole group per unit
@pytest.mark.parametrize("lattice", [(5, 7, 9), (4, 4)], ids=_name)
@pytest.mark.parametrize("dtype", [F32, F64], ids=_name)
@pytest.mark.parametrize("kernel", ["phi4_hmc", "phi4_hmc_tiled"])
def test_momenta_are_the_draw_of_normal_sample(kernel, dtype, lattice):
    """w0 = w2 = w4 = 0: the force is exactly zero, so pi comes back as drawn and dH is exactly 0."""
    C, pos = 3, (0x5EED0000F00D, 37)
    phi = H.field((C,) + lattice, dtype, 1000)
    r = getattr(_hip, kernel)(phi, 0.0, 0.0, 0.0, 1, 0.1, n_traj=1, want_pi=True, position=pos)
    assert torch.equal(r['pi'], _normal_sample_at(pos, C, lattice, dtype))
    assert bool((r['dh'] == 0).all())


@pytest.mark.parametrize("V", [315, 316])
@pytest.mark.parametrize("dtype", [F32, F64], ids=_name)
def test_block_propose_on_the_whole_field_is_normal_sample(dtype, V):
    C, pos = 3, (0x5EED0000F00D, 41)
    x = H.field((C, V), dtype, 1001)
    x0 = x.clone()
    backup = torch.full((C, V), float('nan'), dtype=dtype, device=DEV)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(pos[0])
    gen.set_offset(4 * pos[1])
    _hip.block_propose(x, backup, None, None, V, 0, generator=gen)
    assert torch.equal(x, _normal_sample_at(pos, C, (V,), dtype))
    assert torch.equal(backup, x0)

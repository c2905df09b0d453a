"""ctypes binding of libnormflow_hip.so (the C ABI in include/normflow_hip.h) and the
`torch.autograd.Function`s that put its kernels behind differentiable tensor ops.

There is NO fallback here: if the shared library is missing, or a tensor is not on a
HIP device, the call raises.  PyTorch is used for device memory, the current
stream and autograd bookkeeping only.
"""
import ctypes as C
import math
import os
import threading
import weakref

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libnormflow_hip.so")

NF_F32, NF_F64, NF_F16, NF_F16_FIELD = 0, 1, 2, 3
LAYOUT_FULL, LAYOUT_PAIR = 0, 1
EXTRAP = {None: 0, 'none': 0, 'linear': 1, 'anti': 2, 'anti-periodic': 2}


OPT_SPLIT16, OPT_PIPE = 0, 1


class NormflowHipError(RuntimeError):
    pass


class RqsOpts(C.Structure):
    _fields_ = [("m", C.c_int32), ("extrap_left", C.c_int32), ("extrap_right", C.c_int32),
                ("layout", C.c_int32), ("xlo", C.c_double), ("xhi", C.c_double),
                ("ylo", C.c_double), ("yhi", C.c_double),
                ("fixed_knots_x", C.c_void_p), ("fixed_knots_y", C.c_void_p)]


class Strides(C.Structure):
    _fields_ = [("x_batch", C.c_int64), ("y_batch", C.c_int64), ("params_batch", C.c_int64)]


_P, _I64, _I, _SZ, _D = C.c_void_p, C.c_int64, C.c_int, C.c_size_t, C.c_double
_MAP_ARGS = [_P, _P, _P, _P, _P, _P, _I64, _I64, C.POINTER(RqsOpts), C.POINTER(Strides), _P, _SZ, _I, _P]
_VJP_ARGS = [_P, _P, _P, _P, _P, _P, _P, _I64, _I64, C.POINTER(RqsOpts), C.POINTER(Strides), _I, _P]
_SITES_ARGS = [_P, _P, _P, _P, _P, _P, _P, _I, _I64, _I64, C.POINTER(RqsOpts), C.POINTER(Strides), _P, _SZ, _I, _P]
PROTOTYPES = {
    "nf_version": (C.c_int, []),
    "nf_last_error_string": (C.c_char_p, []),
    "nf_set_option": (C.c_int, [C.c_int, C.c_int]),
    "nf_get_option": (C.c_int, [C.c_int]),
    "nf_workspace_bytes": (_SZ, [_I64, _I64]),
    "nf_plan_tiling": (_I, [_I64, _I64, _I, C.POINTER(C.c_int), C.POINTER(_I64)]),
    "nf_rqs_plan_block": (_I, [C.POINTER(RqsOpts), _I]),
    "nf_rqs_fwd": (_I, _MAP_ARGS),
    "nf_rqs_inv": (_I, _MAP_ARGS),
    "nf_rqs_fwd_sites": (_I, _SITES_ARGS),
    "nf_rqs_inv_sites": (_I, _SITES_ARGS),
    "nf_rqs_knots": (_I, [_P, _P, _I64, _I64, C.POINTER(RqsOpts), _I, _P]),
    "nf_spline_eval": (_I, [_P, _P, _P, _P, _P, _P, _I64, _I64, _I, _I, _I, _I, _I, _I, _P]),
    "nf_rqs_fwd_vjp": (_I, _VJP_ARGS),
    "nf_rqs_inv_vjp": (_I, _VJP_ARGS),
    "nf_affine_fwd": (_I, [_P, _P, _P, _P, _P, _P, _I64, _I64, _I, _I, _P, _SZ, _I, _P]),
    "nf_affine_inv": (_I, [_P, _P, _P, _P, _P, _P, _I64, _I64, _I, _I, _P, _SZ, _I, _P]),
    "nf_affine_sites": (_I, [_P, _P, _P, _P, _P, _P, _P, _I64, _I64, _I, _I, _I, _P, _SZ, _I, _P]),
    "nf_affine_vjp": (_I, [_P, _P, _P, _P, _P, _P, _P, _I64, _I64, _I, _I, _I, _I, _P]),
    "nf_distconv": (_I, [_P, _P, _I, _P, _P, _P, _I64, _I64, _I, _I, _P, _SZ, _I, _P]),
    "nf_distconv_vjp": (_I, [_P, _P, _I, _P, _P, _P, _P, _I64, _I64, _I, _I, _P, _SZ, _I, _P]),
    "nf_distconv_sites": (_I, [_P, _P, _I, _P, _P, _P, _P, _P, _I64, _I64, _I, _I, _I, _P, _SZ, _I, _P]),
    "nf_distconv_sites_vjp": (_I, [_P, _P, _I, _P, _P, _P, _P, _P, _I64, _I64, _I, _I, _I, _P, _SZ, _I, _P]),
    "nf_pade_workspace_bytes": (_SZ, [_I64, _I64, _I64, _I64]),
    "nf_pade": (_I, [_P, _P, _P, _P, _P, _P, _I64, _I64, _I64, _I64, _I, _I, _I, _P, _SZ, _I, _P]),
    "nf_pade_vjp": (_I, [_P, _P, _P, _P, _P, _P, _P, _I64, _I64, _I64, _I64, _I, _I, _I, _P, _SZ, _I, _P]),
    "nf_spectral_supported": (_I, [C.POINTER(C.c_int32), _I, _I, _I]),
    "nf_spectral_workspace_bytes": (_SZ, [C.POINTER(C.c_int32), _I, _I64, _I]),
    "nf_spectral_filter": (_I, [_P, _P, _P, _P, _P, C.POINTER(C.c_int32), _I, _I64, _I, _P]),
    "nf_spectral_filter_vjp": (_I, [_P, _P, _P, _I, _P, _P, _P, _P, _SZ, C.POINTER(C.c_int32), _I, _I64, _I, _P]),
    "nf_conv_two_site": (_I, [_I, _I, _I, _I]),
    "nf_conv_cin_pad": (_I, [_I]),
    "nf_conv_ntiles": (_I, [_I]),
    "nf_conv_packed_steps": (_I, [_I, _I]),
    "nf_phi4_action": (_I, [_P, _P, _I64, C.POINTER(C.c_int32), _D, _D, _D, _P, _SZ, _I, _P]),
    "nf_phi4_action_vjp": (_I, [_P, _P, _P, _I64, C.POINTER(C.c_int32), _D, _D, _D, _I, _P]),
    "nf_phi4_action_density": (_I, [_P, _P, _I64, C.POINTER(C.c_int32), _D, _D, _D, _I, _P]),
    "nf_phi4_action_density_vjp": (_I, [_P, _P, _P, _I64, C.POINTER(C.c_int32), _D, _D, _D, _I, _P]),
    "nf_normal_logprob": (_I, [_P, _P, _P, _P, _I64, _I64, _P, _SZ, _I, _P]),
    "nf_normal_logprob_vjp": (_I, [_P, _P, _P, _P, _P, _I64, _I64, _I, _P]),
    "nf_normal_sample": (_I, [_P, _P, _P, _P, _I64, _I64, C.c_uint64, C.c_uint64, _P, _SZ, _I, _P]),
    "nf_normal_sample_rows": (_I, [_P, _P, _P, _P, _I64, _I64, _I64, C.c_uint64, C.c_uint64, _P, _SZ, _I, _P]),
    "nf_block_propose": (_I, [_P, _P, _P, _P, _I64, _I64, _I64, _I64, C.c_uint64, C.c_uint64, _I, _P]),
    "nf_block_accept": (_I, [_P, _P, _P, _P, _P, _P, _I64, _I64, _I64, _I64, _I, C.c_uint64, C.c_uint64, _I, _P]),
    "nf_metropolis_chains": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I64, _I64, _I, C.c_uint64, C.c_uint64, _I, _P]),
    "nf_metropolis_select": (_I, [_P, _P, _P, _P, _I64, _I64, _I64, _I, _P]),
    "nf_phi4_hmc_supported": (_I, [C.POINTER(C.c_int32), _I]),
    "nf_phi4_hmc": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I64, C.POINTER(C.c_int32), _D, _D, _D, _I, _D, _I, _I,
                         C.c_uint64, C.c_uint64, _I, _P]),
    "nf_phi4_hmc_plan": (_I, [C.POINTER(C.c_int32), _I, _P]),
    "nf_phi4_hmc_measure": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I64, C.POINTER(C.c_int32), _D, _D, _D, _I, _D, _I,
                                 _I, C.c_uint64, C.c_uint64, _I, _P]),
    "nf_phi4_hmc_tiled_supported": (_I, [C.POINTER(C.c_int32), _I]),
    "nf_phi4_hmc_tiled_plan": (_I, [C.POINTER(C.c_int32), _I, _P]),
    "nf_phi4_hmc_tiled_workspace": (_SZ, [_I64, C.POINTER(C.c_int32), _I]),
    "nf_phi4_hmc_tiled": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I64, C.POINTER(C.c_int32), _D, _D, _D, _I, _D, _I, _I,
                               C.c_uint64, C.c_uint64, _P, _SZ, _I, _P]),
    "nf_phi4_hmc_ladder": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I64, C.POINTER(C.c_int32), _P, _I, _P, _I, _D, _I, _I,
                                C.c_uint64, C.c_uint64, _I, _P]),
    "nf_phi4_hmc_tiled_ladder": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I64, C.POINTER(C.c_int32), _P, _I, _P, _I, _D, _I,
                                      _I, C.c_uint64, C.c_uint64, _P, _SZ, _I, _P]),
    "nf_phi4_ladder_exchange": (_I, [_P, _I64, _P, _I, _P, _P, _P, _I64, _I, C.c_uint64, C.c_uint64, _P]),
    "nf_hmc_scheme_check": (_I, [_P]),
    "nf_hmc_scheme_named": (_I, [_I, _P]),
    "nf_phi4_cluster_supported": (_I, [C.POINTER(C.c_int32), _I]),
    "nf_phi4_cluster_plan": (_I, [C.POINTER(C.c_int32), _I, _P]),
    "nf_phi4_cluster": (_I, [_P, _P, _P, _I64, C.POINTER(C.c_int32), _D, C.c_uint64, C.c_uint64, _I, _P]),
    "nf_phi4_cluster_draws": (_I, [_P, _P, _I64, C.POINTER(C.c_int32), C.c_uint64, C.c_uint64, _P]),
    "nf_phi4_cluster_tiled_supported": (_I, [C.POINTER(C.c_int32), _I, _I64]),
    "nf_phi4_cluster_tiled_plan": (_I, [C.POINTER(C.c_int32), _I, _I64, _P]),
    "nf_phi4_cluster_tiled_workspace": (_SZ, [_I64, C.POINTER(C.c_int32), _I64]),
    "nf_phi4_cluster_tiled": (_I, [_P, _P, _P, _I64, C.POINTER(C.c_int32), _D, C.c_uint64, C.c_uint64, _I, _I64, _P, _SZ,
                                   _P]),
    "nf_cluster_moments_supported": (_I, [C.POINTER(C.c_int32), _I]),
    "nf_cluster_moments_plan": (_I, [C.POINTER(C.c_int32), _I, _P]),
    "nf_cluster_moments": (_I, [_P, _P, _P, _P, _P, _I64, C.POINTER(C.c_int32), _P, _I, _P]),
    "nf_cluster_spectrum_supported": (_I, [C.POINTER(C.c_int32), _I, _I]),
    "nf_cluster_spectrum_plan": (_I, [C.POINTER(C.c_int32), _I, _I, _P]),
    "nf_cluster_spectrum": (_I, [_P, _P, _P, _P, _I64, C.POINTER(C.c_int32), _I, _P, _I, _P]),
    "nf_cluster_modes_supported": (_I, [C.POINTER(C.c_int32), _I, _P, _I]),
    "nf_cluster_modes_plan": (_I, [C.POINTER(C.c_int32), _I, _P, _I, _P]),
    "nf_cluster_modes_describe": (_I, [C.POINTER(C.c_int32), _P, _I, _P, _P, _P]),
    "nf_cluster_modes_check": (_I, [C.POINTER(C.c_int32), _P, _I, _I]),
    "nf_cluster_modes": (_I, [_P, _P, _P, _P, _I64, C.POINTER(C.c_int32), _P, _I, _P, _I, _I, _P]),
    "nf_cluster_moments_tiled_supported": (_I, [C.POINTER(C.c_int32), _I, _I64]),
    "nf_cluster_moments_tiled_plan": (_I, [C.POINTER(C.c_int32), _I, _I64, _I, _P]),
    "nf_cluster_moments_tiled_workspace": (_SZ, [_I64, C.POINTER(C.c_int32), _I64, _I]),
    "nf_cluster_moments_tiled": (_I, [_P, _P, _P, _P, _P, _I64, C.POINTER(C.c_int32), _P, _I, _I64, _I, _P, _SZ, _P]),
    "nf_cluster_spectrum_tiled_supported": (_I, [C.POINTER(C.c_int32), _I, _I, _I64]),
    "nf_cluster_spectrum_tiled_plan": (_I, [C.POINTER(C.c_int32), _I, _I, _I64, _I, _P]),
    "nf_cluster_spectrum_tiled_workspace": (_SZ, [_I64, C.POINTER(C.c_int32), _I, _I64, _I]),
    "nf_cluster_spectrum_tiled": (_I, [_P, _P, _P, _P, _I64, C.POINTER(C.c_int32), _I, _P, _I, _I64, _I, _P, _SZ, _P]),
    "nf_cluster_modes_tiled_supported": (_I, [C.POINTER(C.c_int32), _I, _P, _I, _I64]),
    "nf_cluster_modes_tiled_plan": (_I, [C.POINTER(C.c_int32), _I, _P, _I, _I64, _I, _P]),
    "nf_cluster_modes_tiled_workspace": (_SZ, [_I64, C.POINTER(C.c_int32), _I, _I64, _I]),
    "nf_cluster_modes_tiled": (_I, [_P, _P, _P, _P, _I64, C.POINTER(C.c_int32), _P, _I, _P, _I, _I, _I64, _I, _P, _SZ, _P]),
    "nf_phi4_cluster_ladder": (_I, [_P, _P, _P, _I64, C.POINTER(C.c_int32), _P, _I, _P, C.c_uint64, C.c_uint64, _I, _P]),
    "nf_phi4_cluster_tiled_ladder": (_I, [_P, _P, _P, _I64, C.POINTER(C.c_int32), _P, _I, _P, C.c_uint64, C.c_uint64, _I,
                                          _I64, _P, _SZ, _P]),
    "nf_lattice_measure_supported": (_I, [C.POINTER(C.c_int32), _I]),
    "nf_lattice_measure_plan": (_I, [C.POINTER(C.c_int32), _I, _P]),
    "nf_lattice_measure_workspace": (_SZ, [_I64, C.POINTER(C.c_int32), _I]),
    "nf_lattice_measure": (_I, [_P, _P, _I64, C.POINTER(C.c_int32), _P, _SZ, _I, _P]),
    "nf_lattice_measure_tiled_supported": (_I, [C.POINTER(C.c_int32), _SZ, _I]),
    "nf_lattice_measure_tiled_plan": (_I, [C.POINTER(C.c_int32), _SZ, _I, _P]),
    "nf_lattice_measure_tiled_workspace": (_SZ, [_I64, C.POINTER(C.c_int32), _SZ, _I]),
    "nf_lattice_measure_tiled": (_I, [_P, _P, _I64, C.POINTER(C.c_int32), _SZ, _P, _SZ, _I, _P]),
    "nf_act_vjp": (_I, [_P, _P, _P, _I64, _I, _I, _P]),
    "nf_conv_wgrad_cols": (_I, [_I, _I]),
    "nf_conv_wgrad": (_I, [_P, _P, _P, _I64, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _I, _I, _I, _P]),
    "nf_planes_to_split16": (_I, [_P, _P, _P, _I64, _I, C.POINTER(C.c_int32), _I, _P]),
    "nf_conv_dgrad_split16": (_I, [_P, _P, _P, _P, _I64, C.POINTER(C.c_int32), _P, _I, _I, _P]),
    "nf_absmax_bits": (_I, [_P, _I64, _P, _P]),
    "nf_cotangent_pow2": (_I, [_P, _I64, _P, _I64, _P, _P]),
    "nf_conv_last_logits_split16": (_I, [_P, _I, _P, _P, _P, _I64, C.POINTER(C.c_int32), _I, _P, _P]),
    "nf_conv_last_logits_split16_acc": (_I, [_P, _I, _P, _P, _P, _I64, C.POINTER(C.c_int32), _I, _P, _I, _I, _P]),
    "nf_expand_pairs": (_I, [_P, _P, _I64, C.POINTER(C.c_int32), _I, _I, _P]),
    "nf_gather_pad": (_I, [_P, _P, _P, _I64, _I64, _I, _P]),
    "nf_conv_wgrad_sites_supported": (_I, [C.POINTER(C.c_int32), C.POINTER(C.c_int32), _I, _I, _I]),
    "nf_conv_wgrad_sites_workspace": (_SZ, [C.POINTER(C.c_int32), _I, _I, _I]),
    "nf_conv_wgrad_sites": (_I, [_P, _P, _P, _I64, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _I, _I, _I, _P, _SZ, _I, _P]),
    "nf_conv_wgrad_split16_supported": (_I, [C.POINTER(C.c_int32), C.POINTER(C.c_int32), _I, _I]),
    "nf_conv_wgrad_split16_workspace": (_SZ, [_I64, C.POINTER(C.c_int32), _I]),
    "nf_conv_wgrad_split16": (_I, [_P, _P, _P, _I64, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _I, _I, _P, _I, _P, _SZ, _P]),
    "nf_small_lattice_supported": (_I, [C.POINTER(C.c_int32), _I, _I, _I, _I, _I, _I]),
    "nf_small_lattice_coupling": (_I, [_I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I64, C.POINTER(C.c_int32), _I, _I, _I, _I, _I,
                                       C.POINTER(RqsOpts), _I, _P]),
    "nf_conv_rqs_split16_train": (_I, [_P, _I, _P, _P, _I, _P, _P, _P, _P, _I64, C.POINTER(C.c_int32), _I, _P,
                                       C.POINTER(RqsOpts), _I, _P, _SZ, _P]),
    "nf_conv_rqs_split16_vjp": (_I, [_P, _I, _P, _P, _I, _P, _P, _P, _P, _P, _I64, C.POINTER(C.c_int32), _I, _P,
                                     C.POINTER(RqsOpts), _I, _P]),
    "nf_conv_rqs_supported": (_I, [_I, _I]),
    "nf_conv_rqs_split16_supported": (_I, [C.POINTER(C.c_int32), _I, _I]),
    "nf_conv_last_path": (_I, []),
    "nf_conv_split16_supported": (_I, [_P, _P, _I, _I, _I]),
    "nf_conv_fwd_split16": (_I, [_P, _P, _P, _P, _I64, _P, _I, _P]),
    "nf_conv_affine_split16": (_I, [_P, _P, _P, _P, _P, _P, _P, _I64, _P, _I, _I, _I, _P, _SZ, _P]),
    "nf_conv_first_split16_supported": (_I, [_P, _P, _I, _I]),
    "nf_conv_first_split16": (_I, [_P, _P, _P, _P, _I64, _P, _I, _P]),
    "nf_conv_weight_layout": (_I, [_P, _P, _I, _I, _I, _I, _I]),
    "nf_conv_plan": (_I, [C.POINTER(C.c_int32), C.POINTER(C.c_int32), _I, _I, _I, _I, _I, _I64, _P]),
    "nf_conv_rqs": (_I, [_P, _P, _P, _P, _P, _P, _P, _I64, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _I, _I, _I,
                         C.POINTER(RqsOpts), _I, _I, _P, _SZ, _I, _P]),
    "nf_conv_fwd": (_I, [_P, _P, _P, _P, _I64, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _I, _I, _I, _I, _I,
                         _I, _P]),
}

PROTOTYPES.update({
    "nf_phi4_hmc_fa_supported": (_I, [C.POINTER(C.c_int32), _I]),
    "nf_phi4_hmc_fa_plan": (_I, [C.POINTER(C.c_int32), _I, _I, _I, _P]),
    "nf_phi4_hmc_fa_table": (_I, [C.POINTER(C.c_int32), _P]),
    # nf_phi4_hmc's arguments, `const nf_hmc_scheme *scheme` and `double fa_mass_sq`
    "nf_phi4_hmc_fa": (_I, PROTOTYPES["nf_phi4_hmc"][1] + [_P, _D]),
})

# the _scheme form of the five HMC launchers: the launcher's arguments and `const nf_hmc_scheme *scheme`
for _name in ("nf_phi4_hmc", "nf_phi4_hmc_measure", "nf_phi4_hmc_ladder", "nf_phi4_hmc_tiled", "nf_phi4_hmc_tiled_ladder"):
    PROTOTYPES[_name + "_scheme"] = (_I, PROTOTYPES[_name][1] + [_P])
del _name

PROTOTYPES.update({
    "nf_phi4_hmc_fa_tiled_supported": (_I, [C.POINTER(C.c_int32), _I]),
    "nf_phi4_hmc_fa_tiled_plan": (_I, [C.POINTER(C.c_int32), _I, _I, _I, _I, _P]),
    "nf_phi4_hmc_fa_tiled_workspace": (_SZ, [_I64, C.POINTER(C.c_int32), _I]),
    # nf_phi4_hmc_tiled_scheme's arguments, `double fa_mass_sq` and `int cut`
    "nf_phi4_hmc_fa_tiled": (_I, PROTOTYPES["nf_phi4_hmc_tiled_scheme"][1] + [_D, _I]),
})

_lib = None
_lock = threading.Lock()


def load():
    """Load the HIP library once; raise loudly if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise NormflowHipError(
                    f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; "
                    "g.build()'` or `make -C normflow__amd/csrc` (hipcc --offload-arch=gfx950). "
                    "normflow__amd has no CPU or eager-PyTorch fallback for its kernels.")
            lib = C.CDLL(LIB_PATH)
            for name, (res, args) in PROTOTYPES.items():
                fn = getattr(lib, name)
                fn.restype, fn.argtypes = res, args
            _lib = lib
    return _lib


class options:
    """Context manager / setter for the library's kernel-selection options (include/normflow_hip.h, nf_set_option):
    `with _hip.options(split16=False): ...` runs the block with exact fp32 MFMA products everywhere."""
    _CODES = {"split16": OPT_SPLIT16, "pipe": OPT_PIPE}

    def __init__(self, **kw):
        self._new = {self._CODES[k]: int(bool(v)) for k, v in kw.items()}
        self._old = {}

    def __enter__(self):
        lib = load()
        for code, val in self._new.items():
            self._old[code] = lib.nf_set_option(code, val)
        return self

    def __exit__(self, *exc):
        lib = load()
        for code, val in self._old.items():
            lib.nf_set_option(code, val)
        return False


def _check(rc, what):
    if rc != 0:
        msg = load().nf_last_error_string().decode("utf-8", "replace")
        raise NormflowHipError(f"{what} failed (code {rc}): {msg}")


def _dtype_code(t):
    if t.dtype == torch.float32:
        return NF_F32
    if t.dtype == torch.float64:
        return NF_F64
    if t.dtype == torch.float16:      # storage only (RQ-spline map kernels): fp32 arithmetic, fp32 log-det
        return NF_F16
    raise TypeError(f"normflow__amd kernels support float32 and float64 (and float16 storage for the spline map), got {t.dtype}")


def _require_device(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise NormflowHipError(
                "normflow__amd kernels need tensors on an MI355X (torch device 'cuda'); got a "
                f"{t.device} tensor and there is no CPU fallback")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _workspace(B, V, device):
    """Scratch buffer for the per-workgroup log-det partials of ONE call, taken from torch's caching allocator:
    stream-aware (two streams never share partials) and graph-pool safe (a buffer captured into a HIP graph belongs
    to the graph's private pool and is never handed out again while the graph lives)."""
    need = load().nf_workspace_bytes(B, V)
    return torch.empty(max(int(need), 256), dtype=torch.uint8, device=device)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _log0_tensor(log0, like, B):
    """log0 may be the python number 0 (nn/_core.py:25 default) or a (B,) tensor."""
    dt = torch.float32 if like.dtype == torch.float16 else like.dtype       # fp16 fields accumulate log|J| in fp32
    if torch.is_tensor(log0):
        if log0.dim() == 0:
            log0 = log0.expand(B)
        return log0.to(dtype=dt, device=like.device).contiguous()
    if log0 == 0:
        return None
    return torch.full((B,), float(log0), dtype=dt, device=like.device)


MAX_B = 32768  # the batch is the grid's y extent; larger batches are cut into slabs


def _slabs(B, step=None):
    """(b0, b1) of the consecutive slabs of at most `step` (MAX_B) samples that cover a batch of B (none when B == 0)."""
    step = MAX_B if step is None else step
    for b0 in range(0, B, step):
        yield b0, min(B, b0 + step)


def _slab(t, b0, b1):
    """Rows b0 .. b1 of a tensor that may be None (log0, a bias)."""
    return None if t is None else t[b0:b1]


def _c_ints(vals):
    return (C.c_int32 * len(vals))(*vals)


def _lat4(lat, ksize=None):
    """The lattice extents as the c_int32[4] the library takes, fewer than four axes padded with leading 1s; with `ksize`
    the pair (lattice, kernel extents)."""
    pad4 = lambda t: _c_ints([1] * (4 - len(t)) + list(t))
    return pad4(lat) if ksize is None else (pad4(lat), pad4(ksize))


def _sites(lat):
    """Number of sites of a lattice (or of elements of any shape)."""
    n = 1
    for k in lat:
        n *= k
    return n


# =============================================================================== RQS
def make_rqs_opts(m, xlim, ylim, extrap, layout, knots_x=None, knots_y=None):
    """knots_x / knots_y: optional contiguous 1-D device tensors of m fixed knot coordinates (of
    the call's dtype); the limits are then the end knots."""
    extrap = extrap or {}
    for side in ('left', 'right'):
        if extrap.get(side) not in EXTRAP:
            raise NotImplementedError(f"extrapolation {extrap.get(side)!r} is not supported "
                                      "(supported: None, 'linear', 'anti')")
    if knots_x is not None:
        xlim = (float(knots_x[0]), float(knots_x[-1]))
    if knots_y is not None:
        ylim = (float(knots_y[0]), float(knots_y[-1]))
    opts = RqsOpts(int(m), EXTRAP[extrap.get('left')], EXTRAP[extrap.get('right')], int(layout),
                   float(xlim[0]), float(xlim[1]), float(ylim[0]), float(ylim[1]),
                   knots_x.data_ptr() if knots_x is not None else None,
                   knots_y.data_ptr() if knots_y is not None else None)
    opts._keepalive = (knots_x, knots_y)
    return opts


def _rqs_call(fn_name, v, params, mask, log0, opts, strides, B, V, sites_mode=None, what=None):
    """(value, logJ) of nf_rqs_fwd / nf_rqs_inv; with `sites_mode` (an nf_sites_mode) the *_sites entry points, which take
    one more output: (value, logJ, per-site log-derivative or derivative)."""
    lib = load()
    out = torch.empty_like(v)
    sites = None if sites_mode is None else torch.empty_like(v)
    logj = torch.empty(B, dtype=torch.float32 if v.dtype == torch.float16 else v.dtype, device=v.device)
    if log0 is not None and log0.dtype != logj.dtype:
        raise TypeError(f"log0 must be {logj.dtype} for a {v.dtype} field")
    ws = _workspace(min(B, MAX_B), V, v.device)
    for b0, b1 in _slabs(B):
        extra = () if sites is None else (_ptr(sites[b0:b1]), int(sites_mode))
        _check(getattr(lib, fn_name)(_ptr(v[b0:b1]), _ptr(params[b0:b1]), _ptr(mask), _ptr(_slab(log0, b0, b1)),
                                      _ptr(out[b0:b1]), _ptr(logj[b0:b1]), *extra, b1 - b0, V, C.byref(opts),
                                      C.byref(strides) if strides is not None else None, _ptr(ws),
                                      ws.numel(), _dtype_code(v), _stream()), what or fn_name)
    return (out, logj) if sites is None else (out, logj, sites)


SITES_LOG, SITES_DERIVATIVE = 1, 2       # nf_sites_mode


def rqs_sites(v, params, mask, log0, opts, inverse, mode=SITES_LOG):
    """nf_rqs_fwd_sites / nf_rqs_inv_sites: (value, logJ, per-site log-derivative or derivative).  Inference only
    (no autograd): the spline-object / propagate_density path of the reference (couplings_.py:202-209, _core.py:38-42)."""
    _require_device(v, params, mask, log0)
    if v.dtype not in (torch.float32, torch.float64) or params.dtype != v.dtype:
        raise TypeError(f"per-site derivatives are built for float32 / float64 fields; got {v.dtype} / {params.dtype}")
    B, V = v.shape
    v, params = v.detach().contiguous(), params.detach().contiguous()
    return _rqs_call("nf_rqs_inv_sites" if inverse else "nf_rqs_fwd_sites", v, params, mask, log0, opts, None, B, V,
                     sites_mode=mode, what="nf_rqs_sites")


def _channels(params, b0, b1, i, Cs):
    """The logits of spline i of a multi-spline call: a view, whose first element the kernel addresses with batch strides."""
    return params[b0:b1, i * Cs:(i + 1) * Cs]


def multi_rqs_sites(v, params, mask, opts_list, inverse, mode=SITES_LOG):
    """Per-site values and log-derivatives (or derivatives) of `n_s` splines, one per data channel
    (MultiRQSplineCoupling_ with propagate_density, couplings_.py:304-329 + nn/_core.py:38-42).
    v: (B, n_s, V), params: (B, n_s*C, V) -> (value (B, n_s, V), sites (B, n_s, V)).  Inference only."""
    _require_device(v, params, mask)
    if v.dtype not in (torch.float32, torch.float64) or params.dtype != v.dtype:
        raise TypeError(f"per-site derivatives are built for float32 / float64 fields; got {v.dtype} / {params.dtype}")
    lib = load()
    B, ns, V = v.shape
    v, params = v.detach().contiguous(), params.detach().contiguous()
    Ctot, Vp = params.shape[1], params.shape[2]
    Cs = Ctot // ns
    out = torch.empty_like(v)
    sites = torch.empty(ns, B, V, dtype=v.dtype, device=v.device)
    logj = torch.empty(B, dtype=v.dtype, device=v.device)
    ws = _workspace(min(B, MAX_B), V, v.device)
    fn = lib.nf_rqs_inv_sites if inverse else lib.nf_rqs_fwd_sites
    st = Strides(ns * V, ns * V, Ctot * Vp)
    for i, opts in enumerate(opts_list):
        for b0, b1 in _slabs(B):
            _check(fn(_ptr(v[b0:b1, i]), _ptr(_channels(params, b0, b1, i, Cs)), _ptr(mask), None,
                      _ptr(out[b0:b1, i]), _ptr(logj[b0:b1]), _ptr(sites[i, b0:b1]),
                      int(mode), b1 - b0, V, C.byref(opts), C.byref(st), _ptr(ws), ws.numel(), _dtype_code(v),
                      _stream()), "nf_rqs_sites (multi)")
    return out, sites.movedim(0, 1)


def spline_eval(v, kx, ky, kd, K, shared, inverse, grad):
    """nf_spline_eval: a spline given by explicit knots at every site.  v: (B, V); each knot tensor (K, B*V) planes... laid
    out (K, V) per batch row when B == 1, or a shared (K,) vector (`shared` = three flags).  Returns (value, derivative|None)."""
    _require_device(v, kx, ky, kd)
    B, V = v.shape
    if B != 1 and not all(shared):
        raise NotImplementedError("per-site explicit knots are addressed as one (K, V) block: pass B == 1")
    out = torch.empty_like(v)
    der = torch.empty_like(v) if grad else None
    _check(load().nf_spline_eval(_ptr(v), _ptr(kx), _ptr(ky), _ptr(kd), _ptr(out), _ptr(der), B, V, int(K),
                                 int(shared[0]), int(shared[1]), int(shared[2]), int(bool(inverse)), _dtype_code(v),
                                 _stream()), "nf_spline_eval")
    return out, der


def rqs_knots(params, opts):
    """nf_rqs_knots: (B, C, V) logits -> (B, 3m, V) = knots_x | knots_y | knots_d, before boundary augmentation."""
    _require_device(params)
    if params.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"knots are built for float32 / float64 logits; got {params.dtype}")
    params = params.detach().contiguous()
    B, _, V = params.shape
    knots = torch.empty(B, 3 * opts.m, V, dtype=params.dtype, device=params.device)
    for b0, b1 in _slabs(B, 65535):
        _check(load().nf_rqs_knots(_ptr(params[b0:b1]), _ptr(knots[b0:b1]), b1 - b0, V, C.byref(opts),
                                   _dtype_code(params), _stream()), "nf_rqs_knots")
    return knots


def _rqs_vjp_call(fn_name, x, params, mask, gout, glogj, opts, strides, B, V):
    lib = load()
    gin = torch.empty_like(x)
    gpar = torch.empty_like(params)
    for b0, b1 in _slabs(B):
        _check(getattr(lib, fn_name)(_ptr(x[b0:b1]), _ptr(params[b0:b1]), _ptr(mask), _ptr(gout[b0:b1]),
                                      _ptr(glogj[b0:b1]), _ptr(gin[b0:b1]), _ptr(gpar[b0:b1]), b1 - b0, V,
                                      C.byref(opts), C.byref(strides) if strides is not None else None,
                                      _dtype_code(x), _stream()), fn_name)
    return gin, gpar


class RQSCouplingFn(torch.autograd.Function):
    """(value, logJ) of one RQ-spline coupling layer on the active sublattice.

    v: (B, V) field (only active sites are read); params: (B, C, V) or (B, C, V/2) raw
    logits; mask: (V,) uint8 activity; log0: (B,) tensor or None.
    """

    @staticmethod
    def forward(ctx, v, params, log0, mask, opts, inverse):
        _require_device(v, params, mask, log0)
        B, V = v.shape
        v, params = v.contiguous(), params.contiguous()
        if params.dtype != v.dtype:
            raise TypeError(f"field is {v.dtype} but net output is {params.dtype}")
        out, logj = _rqs_call("nf_rqs_inv" if inverse else "nf_rqs_fwd", v, params, mask, log0, opts,
                              None, B, V)
        ctx.save_for_backward(out if inverse else v, params, mask)
        ctx.opts, ctx.inverse, ctx.has_log0 = opts, inverse, log0 is not None
        return out, logj

    @staticmethod
    def backward(ctx, gout, glogj):
        x, params, mask = ctx.saved_tensors
        if x.dtype == torch.float16:
            raise NotImplementedError("fp16 storage is an inference path (nf_rqs_fwd / nf_rqs_inv); train in fp32")
        B, V = x.shape
        gin, gpar = _rqs_vjp_call("nf_rqs_inv_vjp" if ctx.inverse else "nf_rqs_fwd_vjp", x, params, mask,
                                  gout.contiguous(), glogj.contiguous(), ctx.opts, None, B, V)
        return gin, gpar, (glogj if ctx.has_log0 else None), None, None, None


class MultiRQSCouplingFn(torch.autograd.Function):
    """`n_s` independent splines, one per data channel, addressed in place through batch
    strides (MultiRQSplineCoupling_).  v: (B, n_s, V); params: (B, n_s*C, Vp)."""

    @staticmethod
    def forward(ctx, v, params, log0, mask, opts_list, inverse):
        _require_device(v, params, mask, log0)
        B, ns, V = v.shape
        v, params = v.contiguous(), params.contiguous()
        if params.dtype != v.dtype:        # the kernel reads both with the field's dtype code: a silent reinterpretation otherwise
            raise TypeError(f"field is {v.dtype} but net output is {params.dtype}")
        if log0 is not None and log0.dtype != v.dtype:
            raise TypeError(f"log0 must be {v.dtype} for a {v.dtype} field")
        Ctot, Vp = params.shape[1], params.shape[2]
        Cs = Ctot // ns
        out = torch.empty_like(v)
        lib = load()
        fn = lib.nf_rqs_inv if inverse else lib.nf_rqs_fwd
        ws = _workspace(min(B, MAX_B), V, v.device)
        st = Strides(ns * V, ns * V, Ctot * Vp)
        logj = log0
        for i, opts in enumerate(opts_list):
            nxt = torch.empty(B, dtype=v.dtype, device=v.device)
            for b0, b1 in _slabs(B):       # the batch is the grid's y extent
                _check(fn(_ptr(v[b0:b1, i]), _ptr(_channels(params, b0, b1, i, Cs)), _ptr(mask), _ptr(_slab(logj, b0, b1)),
                          _ptr(out[b0:b1, i]), _ptr(nxt[b0:b1]), b1 - b0, V,
                          C.byref(opts), C.byref(st), _ptr(ws), ws.numel(), _dtype_code(v), _stream()),
                       "nf_rqs (multi)")
            logj = nxt
        ctx.save_for_backward(out if inverse else v, params, mask)
        ctx.opts_list, ctx.inverse, ctx.has_log0 = opts_list, inverse, log0 is not None
        return out, logj

    @staticmethod
    def backward(ctx, gout, glogj):
        x, params, mask = ctx.saved_tensors
        B, ns, V = x.shape
        Ctot, Vp = params.shape[1], params.shape[2]
        Cs = Ctot // ns
        gout, glogj = gout.contiguous(), glogj.contiguous()
        gin, gpar = torch.empty_like(x), torch.empty_like(params)
        lib = load()
        fn = lib.nf_rqs_inv_vjp if ctx.inverse else lib.nf_rqs_fwd_vjp
        st = Strides(ns * V, ns * V, Ctot * Vp)
        for i, opts in enumerate(ctx.opts_list):
            for b0, b1 in _slabs(B):
                _check(fn(_ptr(x[b0:b1, i]), _ptr(_channels(params, b0, b1, i, Cs)), _ptr(mask),
                          _ptr(gout[b0:b1, i]), _ptr(glogj[b0:b1]),
                          _ptr(gin[b0:b1, i]), _ptr(_channels(gpar, b0, b1, i, Cs)), b1 - b0, V,
                          C.byref(opts), C.byref(st), _dtype_code(x), _stream()), "nf_rqs_vjp (multi)")
        return gin, gpar, (glogj if ctx.has_log0 else None), None, None, None


# ============================================================================ affine
def affine_sites(v, params, mask, log0, layout, inverse):
    """nf_affine_sites: (value, logJ, per-site log-derivative) of an affine / shift layer; inference only."""
    _require_device(v, params, mask, log0)
    if v.dtype not in (torch.float32, torch.float64) or params.dtype != v.dtype:
        raise TypeError(f"per-site densities are built for float32 / float64 fields; got {v.dtype} / {params.dtype}")
    B, V = v.shape
    v, params = v.detach().contiguous(), params.detach().contiguous()
    out, sites = torch.empty_like(v), torch.empty_like(v)
    logj = torch.empty(B, dtype=v.dtype, device=v.device)
    ws = _workspace(min(B, MAX_B), V, v.device)
    for b0, b1 in _slabs(B):
        _check(load().nf_affine_sites(_ptr(v[b0:b1]), _ptr(params[b0:b1]), _ptr(mask), _ptr(_slab(log0, b0, b1)), _ptr(out[b0:b1]),
                                      _ptr(logj[b0:b1]), _ptr(sites[b0:b1]), b1 - b0, V, params.shape[1], layout,
                                      int(bool(inverse)), _ptr(ws), ws.numel(), _dtype_code(v), _stream()),
               "nf_affine_sites")
    return out, logj, sites


class AffineCouplingFn(torch.autograd.Function):
    """Affine (n_ch = 2) or shift (n_ch = 1) coupling on the active sublattice."""

    @staticmethod
    def forward(ctx, v, params, log0, mask, layout, inverse):
        _require_device(v, params, mask, log0)
        B, V = v.shape
        v, params = v.contiguous(), params.contiguous()
        if v.dtype == torch.float16:
            # fp16 field storage (BASELINE config 5): params either half as well (NF_F16) or the fp32 a conv layer wrote
            # (NF_F16_FIELD); fp32 arithmetic, fp32 log-det
            if params.dtype == torch.float16:
                code = NF_F16
            elif params.dtype == torch.float32:
                code = NF_F16_FIELD
            else:
                raise TypeError(f"half field with {params.dtype} parameters")
            ldt = torch.float32
        else:
            if params.dtype != v.dtype:
                raise TypeError(f"field is {v.dtype} but net output is {params.dtype}")
            code, ldt = _dtype_code(v), v.dtype
        if log0 is not None and log0.dtype != ldt:
            raise TypeError(f"log0 must be {ldt} for a {v.dtype} field")
        n_ch = params.shape[1]
        lib = load()
        out = torch.empty_like(v)
        logj = torch.empty(B, dtype=ldt, device=v.device)
        ws = _workspace(min(B, MAX_B), V, v.device)
        fn = lib.nf_affine_inv if inverse else lib.nf_affine_fwd
        for b0, b1 in _slabs(B):
            _check(fn(_ptr(v[b0:b1]), _ptr(params[b0:b1]), _ptr(mask), _ptr(_slab(log0, b0, b1)), _ptr(out[b0:b1]),
                      _ptr(logj[b0:b1]), b1 - b0, V, n_ch, layout, _ptr(ws), ws.numel(), code,
                      _stream()), "nf_affine")
        ctx.save_for_backward(v, params, mask)
        ctx.layout, ctx.inverse, ctx.has_log0 = layout, inverse, log0 is not None
        return out, logj

    @staticmethod
    def backward(ctx, gout, glogj):
        v, params, mask = ctx.saved_tensors
        if v.dtype == torch.float16:
            raise NotImplementedError("fp16 storage is an inference path (nf_affine_fwd / nf_affine_inv); train in fp32")
        B, V = v.shape
        gout, glogj = gout.contiguous(), glogj.contiguous()
        gin, gpar = torch.empty_like(v), torch.empty_like(params)
        lib = load()
        for b0, b1 in _slabs(B):
            _check(lib.nf_affine_vjp(_ptr(v[b0:b1]), _ptr(params[b0:b1]), _ptr(mask), _ptr(gout[b0:b1]),
                                     _ptr(glogj[b0:b1]), _ptr(gin[b0:b1]), _ptr(gpar[b0:b1]), b1 - b0, V,
                                     params.shape[1], ctx.layout, int(ctx.inverse), _dtype_code(v),
                                     _stream()), "nf_affine_vjp")
        return gin, gpar, (glogj if ctx.has_log0 else None), None, None, None


# ========================================================================== distconv
STAGE_EXPIT, STAGE_SPLINE, STAGE_LOGIT = 1, 2, 4


class DistConvFn(torch.autograd.Function):
    """Expit_ -> shared-knot spline -> Logit_ (any subset, `stages` bit mask) in one pass.

    v: (B, V); knots: (3, K) augmented knots (x | y | d), differentiable.
    """

    @staticmethod
    def forward(ctx, v, knots, log0, stages, inverse):
        _require_device(v, knots, log0)
        B, V = v.shape
        v = v.contiguous()
        if knots is not None:
            knots = knots.to(v.dtype).contiguous()
        K = knots.shape[1] if knots is not None else 0
        lib = load()
        out = torch.empty_like(v)
        logj = torch.empty(B, dtype=v.dtype, device=v.device)
        ws = _workspace(min(B, MAX_B), V, v.device)
        for b0, b1 in _slabs(B):
            _check(lib.nf_distconv(_ptr(v[b0:b1]), _ptr(knots), K, _ptr(_slab(log0, b0, b1)), _ptr(out[b0:b1]),
                                   _ptr(logj[b0:b1]), b1 - b0, V, stages, int(inverse), _ptr(ws),
                                   ws.numel(), _dtype_code(v), _stream()), "nf_distconv")
        ctx.save_for_backward(out if inverse else v, knots)
        ctx.stages, ctx.inverse, ctx.has_log0 = stages, inverse, log0 is not None
        return out, logj

    @staticmethod
    def backward(ctx, gout, glogj):
        x, knots = ctx.saved_tensors
        B, V = x.shape
        K = knots.shape[1] if knots is not None else 0
        gout, glogj = gout.contiguous(), glogj.contiguous()
        gin = torch.empty_like(x)
        gk = torch.zeros(3, max(K, 1), dtype=torch.float64, device=x.device)
        lib = load()
        ws = _workspace(min(B, MAX_B), V, x.device)
        for b0, b1 in _slabs(B):
            part = torch.zeros(3, max(K, 1), dtype=torch.float64, device=x.device)
            _check(lib.nf_distconv_vjp(_ptr(x[b0:b1]), _ptr(knots), K, _ptr(gout[b0:b1]), _ptr(glogj[b0:b1]),
                                       _ptr(gin[b0:b1]), _ptr(part), b1 - b0, V, ctx.stages,
                                       int(ctx.inverse), _ptr(ws), ws.numel(), _dtype_code(x), _stream()),
                   "nf_distconv_vjp")
            gk += part
        gk = gk.to(knots.dtype) if knots is not None else None
        return gin, gk, (glogj if ctx.has_log0 else None), None, None


DC_SUM, DC_SITES = 0, 1      # nf_distconv_mode


class DistConvSitesFn(torch.autograd.Function):
    """nf_distconv_sites: the stages of DistConvFn with an optional (V,) uint8 activity mask (inactive sites: y = x,
    density 0) and, with per_site, the per-site log-density log0 + log|f'| (B, V) instead of the per-sample sum over the
    active sites (B).  log0: None, (B, V) (per_site) or (B,).  Differentiable in v, knots and log0."""

    @staticmethod
    def forward(ctx, v, knots, log0, mask, stages, inverse, per_site):
        _require_device(v, knots, log0, mask)
        if v.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"per-site densities are built for float32 / float64 fields, got {v.dtype}")
        B, V = v.shape
        v = v.contiguous()
        if knots is not None:
            knots = knots.to(v.dtype).contiguous()
        if mask is not None and (mask.dtype != torch.uint8 or mask.numel() != V):
            raise ValueError(f"the activity mask must be {V} uint8 bytes, got {mask.numel()} {mask.dtype}")
        K = knots.shape[1] if knots is not None else 0
        lib = load()
        out = torch.empty_like(v)
        dens = torch.empty_like(v) if per_site else torch.empty(B, dtype=v.dtype, device=v.device)
        ws = None if per_site else _workspace(min(B, MAX_B), V, v.device)
        mode = DC_SITES if per_site else DC_SUM
        for b0, b1 in _slabs(B):
            _check(lib.nf_distconv_sites(_ptr(v[b0:b1]), _ptr(knots), K, _ptr(_slab(log0, b0, b1)), _ptr(mask), _ptr(out[b0:b1]),
                                         _ptr(dens[b0:b1]) if per_site else None,
                                         None if per_site else _ptr(dens[b0:b1]), b1 - b0, V, stages, int(inverse),
                                         mode, _ptr(ws), ws.numel() if ws is not None else 0, _dtype_code(v),
                                         _stream()), "nf_distconv_sites")
        ctx.save_for_backward(out if inverse else v, knots, mask)
        ctx.stages, ctx.inverse, ctx.mode, ctx.has_log0 = stages, inverse, mode, log0 is not None
        return out, dens

    @staticmethod
    def backward(ctx, gout, gdens):
        x, knots, mask = ctx.saved_tensors
        B, V = x.shape
        K = knots.shape[1] if knots is not None else 0
        gout, gdens = gout.contiguous(), gdens.contiguous()
        gin = torch.empty_like(x)
        gk = torch.zeros(3, max(K, 1), dtype=torch.float64, device=x.device)
        lib = load()
        ws = _workspace(min(B, MAX_B), V, x.device)
        for b0, b1 in _slabs(B):
            part = torch.zeros(3, max(K, 1), dtype=torch.float64, device=x.device)
            _check(lib.nf_distconv_sites_vjp(_ptr(x[b0:b1]), _ptr(knots), K, _ptr(mask), _ptr(gout[b0:b1]),
                                             _ptr(gdens[b0:b1]), _ptr(gin[b0:b1]), _ptr(part), b1 - b0, V, ctx.stages,
                                             int(ctx.inverse), ctx.mode, _ptr(ws), ws.numel(), _dtype_code(x),
                                             _stream()), "nf_distconv_sites_vjp")
            gk += part
        gk = gk.to(knots.dtype) if knots is not None else None
        return gin, gk, (gdens if ctx.has_log0 else None), None, None, None, None


# ============================================================================== pade
TANH, PADE11, PADE22, PADE32 = 1, 11, 22, 32      # nf_pade_kind


def _pade_workspace(layout, device):
    need = load().nf_pade_workspace_bytes(*layout)
    return torch.empty(max(int(need), 256), dtype=torch.uint8, device=device)


class PadeFn(torch.autograd.Function):
    """Pade11_ / Pade22_ / Pade32_ / Tanh_ (nf_pade) forward or inverse, differentiable in the field and in the per-channel
    parameters.

    v: the field (any shape, contiguous); d0, d1: (C,) parameters as the kernel takes them (softplus_ln2 of the Pade11_ /
    Pade22_ weights, 3 expit(w0) for Pade32_; d1 only for Pade22_; both None for TANH, which has no parameter gradient);
    layout: (B, outer, C, inner) of nf_pade; log0: None, (B,) or (per_site) the shape of v."""

    @staticmethod
    def forward(ctx, v, d0, d1, log0, kind, inverse, per_site, layout):
        _require_device(v, d0, d1, log0)
        if v.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"the nf_pade maps run on float32 / float64 fields, got {v.dtype}")
        if kind not in (TANH, PADE11, PADE22, PADE32):
            raise ValueError(f"PadeFn: unknown kind {kind}")
        if (d0 is None) != (kind == TANH) or (d1 is None) != (kind != PADE22):
            raise ValueError(f"PadeFn: kind {kind} takes {'no parameters' if kind == TANH else 'd0 and d1' if kind == PADE22 else 'd0 only'}")
        v = v.contiguous()
        out = torch.empty_like(v)
        logj = torch.empty_like(v) if per_site else torch.empty(layout[0], dtype=v.dtype, device=v.device)
        ws = None if per_site else _pade_workspace(layout, v.device)
        _check(load().nf_pade(_ptr(v), _ptr(d0), _ptr(d1), _ptr(log0), _ptr(out), _ptr(logj), *layout, kind,
                              int(bool(inverse)), int(bool(per_site)), _ptr(ws), ws.numel() if ws is not None else 0,
                              _dtype_code(v), _stream()), "nf_pade")
        ctx.save_for_backward(out if inverse else v, d0, d1)
        ctx.kind, ctx.inverse, ctx.per_site, ctx.layout = kind, inverse, per_site, layout
        ctx.has_log0 = log0 is not None
        return out, logj

    @staticmethod
    def backward(ctx, gout, glogj):
        x, d0, d1 = ctx.saved_tensors
        gout, glogj = gout.contiguous(), glogj.contiguous()
        gin = torch.empty_like(x)
        gd = torch.empty(2, d0.numel() if d0 is not None else 1, dtype=torch.float64, device=x.device)
        ws = _pade_workspace(ctx.layout, x.device)
        _check(load().nf_pade_vjp(_ptr(x), _ptr(d0), _ptr(d1), _ptr(gout), _ptr(glogj), _ptr(gin), _ptr(gd),
                                  *ctx.layout, ctx.kind, int(bool(ctx.inverse)), int(bool(ctx.per_site)), _ptr(ws),
                                  ws.numel(), _dtype_code(x), _stream()), "nf_pade_vjp")
        gd = gd.to(x.dtype)
        return (gin, gd[0] if d0 is not None else None, gd[1] if d1 is not None else None, glogj if ctx.has_log0 else None,
                None, None, None, None)


# ========================================================================== spectral
def spectral_supported(lat, dtype, for_vjp=False):
    """nf_spectral_supported for a lattice and a torch dtype: (True, '') or (False, the library's reason)."""
    code = {torch.float32: NF_F32, torch.float64: NF_F64}.get(dtype)
    if code is None:
        return False, f"the Hartley filter runs on float32 / float64 fields, got {dtype}"
    lib = load()
    if lib.nf_spectral_supported(_c_ints(list(lat)), len(lat), code, int(bool(for_vjp))):
        return True, ""
    return False, lib.nf_last_error_string().decode("utf-8", "replace")


def spectral_require(x, lat, for_vjp=False):
    """Raise NormflowHipError unless `x` is a field the Hartley filter takes: on the device, float32 / float64, trailing
    axes == lat, and a lattice nf_spectral_supported accepts."""
    _require_device(x)
    if tuple(x.shape[-len(lat):]) != tuple(lat) or x.dim() < len(lat) + 1:
        raise NormflowHipError(f"the Hartley filter of a {tuple(lat)} lattice got a field of shape {tuple(x.shape)}")
    ok, why = spectral_supported(lat, x.dtype, for_vjp)
    if not ok:
        raise NormflowHipError(f"transform='hartley' cannot take this field: {why}")


class SpectralFilterFn(torch.autograd.Function):
    """y_b = T D_b T x_b in the separable Hartley basis T (nf_spectral_filter): irfftn(rfftn(x) * w_half, s=lattice) for a
    weight that is even in every k_mu, in one launch with the sample resident in LDS.

    x: (B, *lattice); w_half: the weight on the rfftn grid (*lattice[:-1], N/2 + 1); zero_new: None or (B,), the value
    the zero-mode coefficient sum(x_b) / sqrt(V) is replaced by.  Differentiable in all three.  The cotangent of w_half
    is the Hartley-basis one: summed over each symmetry orbit (+-k_1, .., +-k_d) it equals autograd's through rfftn, entry
    by entry it does not (d >= 2) -- exact for every parameter behind a weight that depends on k through khat^2."""

    @staticmethod
    def forward(ctx, x, w_half, zero_new):
        lat = tuple(x.shape[1:])
        spectral_require(x, lat)
        _require_device(w_half, zero_new)
        B = x.shape[0]
        if tuple(w_half.shape) != lat[:-1] + (lat[-1] // 2 + 1,):
            raise ValueError(f"w_half must be on the rfftn grid of {lat}, got {tuple(w_half.shape)}")
        if zero_new is not None and zero_new.numel() != B:
            raise ValueError(f"zero_new must hold one value per sample ({B}), got {tuple(zero_new.shape)}")
        x = x.contiguous()
        w_half = w_half.to(x.dtype).contiguous()
        zero_new = None if zero_new is None else zero_new.to(x.dtype).contiguous()
        y = torch.empty_like(x)
        _check(load().nf_spectral_filter(_ptr(x), _ptr(w_half), _ptr(zero_new), _ptr(y), None, _c_ints(list(lat)),
                                         len(lat), B, _dtype_code(x), _stream()), "nf_spectral_filter")
        ctx.save_for_backward(x, w_half)
        ctx.replaced = zero_new is not None
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        x, w_half = ctx.saved_tensors
        lat, B = tuple(x.shape[1:]), x.shape[0]
        spectral_require(x, lat, for_vjp=True)
        gy = gy.contiguous()
        gx = torch.empty_like(x)
        gw = torch.empty_like(w_half)
        gzero = torch.empty(B, dtype=x.dtype, device=x.device) if ctx.replaced else None
        lat_c = _c_ints(list(lat))
        need = load().nf_spectral_workspace_bytes(lat_c, len(lat), B, _dtype_code(x))
        ws = torch.empty(max(int(need), 256), dtype=torch.uint8, device=x.device)
        _check(load().nf_spectral_filter_vjp(_ptr(x), _ptr(gy), _ptr(w_half), int(ctx.replaced), _ptr(gx), _ptr(gw),
                                             _ptr(gzero), _ptr(ws), ws.numel(), lat_c, len(lat), B, _dtype_code(x),
                                             _stream()), "nf_spectral_filter_vjp")
        return gx, gw, gzero


def spectral_filter(x, w_half, zero_new=None):
    """SpectralFilterFn on a (..., *lattice) field (leading axes flattened into the batch), refusing up front a field
    whose backward pass would not fit."""
    lat = tuple(w_half.shape[:-1]) + (x.shape[-1],)
    grads = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, w_half, zero_new))
    spectral_require(x, lat, for_vjp=grads)
    y = SpectralFilterFn.apply(x.reshape((-1,) + lat), w_half.to(x.dtype), zero_new)
    return y.reshape(x.shape)


# ============================================================================== conv
ACT_CODES = {None: 0, 'none': 0, 'tanh': 1, 'relu': 2, 'leaky_relu': 3, 'softplus': 4, 'abs': 5, 'expit': 6}
_TORCH_ACT = {0: lambda t: t, 1: torch.tanh, 2: torch.relu,
              3: lambda t: torch.nn.functional.leaky_relu(t), 4: lambda t: torch.nn.functional.softplus(t),
              5: torch.abs, 6: torch.sigmoid}


def pack_conv_weight(w):
    """(Cout, Cin, *k) -> MFMA fragment order [tap][cin/4][cout/16][4][16] (zero padded)."""
    cout, cin = w.shape[:2]
    ntaps = _sites(w.shape[2:])
    nt = (cout + 15) // 16
    ns = load().nf_conv_packed_steps(cin, ntaps)
    if ns:      # cin % 4 != 0: K = (tap, ci) flattened, 4 per step
        wk = w.new_zeros(nt * 16, 4 * ns)
        wk[:cout, :cin * ntaps] = w.reshape(cout, cin, ntaps).permute(0, 2, 1).reshape(cout, ntaps * cin)
        return wk.reshape(nt, 16, ns, 4).permute(2, 0, 3, 1).contiguous()
    cin_pad = (cin + 3) // 4 * 4
    wp = w.new_zeros(nt * 16, cin_pad, ntaps)
    wp[:cout, :cin] = w.reshape(cout, cin, ntaps)
    return wp.reshape(nt, 16, cin_pad // 4, 4, ntaps).permute(4, 2, 0, 3, 1).contiguous()


def conv_weight_for_layer(w, lat4, k4, cin, cout, compact, fused, dtype_code):
    """Pack (Cout', Cin, *k) weights (already two-site expanded where that applies) in the layout the
    library will read for this layer (nf_conv_weight_layout): fragment order, or row-packed for the
    persistent kernel -- [row][cin/4][lane][K3*ntiles -> multiple of 4]."""
    frag = pack_conv_weight(w)
    code = load().nf_conv_weight_layout(lat4, k4, cin, cout, int(compact), int(fused), dtype_code)
    if code < 0:
        raise RuntimeError("nf_conv_weight_layout: invalid layer description")
    if code == 0:
        return frag
    if code == 2:
        return pack_conv_weight_split16(w)
    ntaps, kq, nt = frag.shape[:3]
    k3 = w.shape[-1]
    rows = ntaps // k3
    vals = frag.reshape(rows, k3, kq, nt, 64).permute(0, 2, 4, 1, 3).reshape(rows, kq, 64, k3 * nt)
    nv = (k3 * nt + 3) // 4 * 4
    out = vals.new_zeros(rows, kq, 64, nv)
    out[..., :k3 * nt] = vals
    return out.contiguous()


# The weights are scaled by 2^10 before the split (the kernel scales the accumulators back, exactly): typical |w| ~ 0.1
# would put the lo parts into fp16's subnormal range -- absolute resolution 6e-8, i.e. 5e-7 RELATIVE to w and, unlike
# activation rounding, the same error at every site: it showed up as a coherent 1.7e-5 shift of log|J| on 32^4.
SPLIT16_WEIGHT_SCALE = 1024.0
# The split-fp16 kernels take weights with max|w| BELOW this (`_weights_fit_fp16`; graphs.GraphedTrainStep's guard): 1024 w
# then stays under 3.0e4, well inside fp16 (65504), and hi = fp16(1024 w) is finite.  29.296875: 29.29 fits, 29.30 does not.
SPLIT16_WEIGHT_LIMIT = 3.0e4 / SPLIT16_WEIGHT_SCALE


def pack_conv_weight_split16(w):
    """(46, 8, 3, 3, 3, 3) fp32 weights -> NF_WLAYOUT_SPLIT16 (include/normflow_hip.h): fp16 hi / lo pairs in the
    B-fragment order of v_mfma_f32_16x16x32_f16, [column tile (3)][K slice (21)][hi|lo][lane (64)][8]:
    slice 7*j3 + i = tap j3 of kernel rows 4i..4i+3; lane 16*g + n holds the 8 input channels of row 4i+g for
    column 16*tile + n (zero for row 27 and for columns >= cout)."""
    cout, cin = w.shape[:2]
    assert cin == 8 and tuple(w.shape[2:]) == (3, 3, 3, 3) and cout <= 48
    wp = w.new_zeros(48, 8, 28, 3, dtype=torch.float32)
    wp[:cout, :, :27] = w.reshape(cout, 8, 27, 3).float() * SPLIT16_WEIGHT_SCALE
    hi = wp.half()
    lo = (wp - hi.float()).half()
    out = torch.empty(3, 21, 2, 64, 8, dtype=torch.float16, device=w.device)
    for k, part in enumerate((hi, lo)):
        # part[co = 16 t + n, ch, row = 4 i + g, j3]  ->  [t, j3, i, g, n, ch]
        v = part.reshape(3, 16, 8, 7, 4, 3).permute(0, 5, 3, 4, 1, 2)       # t, j3, i, g, n, ch
        out[:, :, k] = v.reshape(3, 21, 64, 8)
    return out.contiguous()


def pack_conv_weight_split16_two_site(w):
    """(8, 8, 3, 3, 3, 3) fp32 weights of a hidden layer -> the B fragments of conv_g_kernel (include/normflow_hip.h,
    nf_conv_fwd_split16): [kernel row (27)][hi|lo][lane (64)][8]; lane 16*g + n: column n = 8*shift + co, tap g - shift."""
    assert tuple(w.shape) == (8, 8, 3, 3, 3, 3)
    wr = w.reshape(8, 8, 27, 3).float() * SPLIT16_WEIGHT_SCALE          # co, ch, row, j3
    w2 = wr.new_zeros(16, 8, 27, 4)                                     # column, ch, row, tap g
    w2[:8, :, :, :3] = wr
    w2[8:, :, :, 1:] = wr
    hi = w2.half()
    lo = (w2 - hi.float()).half()
    out = torch.empty(27, 2, 64, 8, dtype=torch.float16, device=w.device)
    for k, part in enumerate((hi, lo)):
        out[:, k] = part.permute(2, 3, 0, 1).reshape(27, 64, 8)         # row, (g, n), ch
    return out.contiguous()


def pack_conv_weight_split16_stacked(w):
    """(8, 8, 3, 3, 3, 3) fp32 weights of a hidden layer -> the A fragments of conv_g2_kernel (include/normflow_hip.h,
    nf_conv_fwd_split16): 18 STACKED fragments [set (2)][j2 (3)][dx (3)][lane (64)][8], then the two-site fragments of
    `pack_conv_weight_split16_two_site` (27 x [hi|lo]); 72 fragments of 64 lanes x 8 halfs.  Stacked: lane 16*g + n holds, for
    row n = 8*part + co (part 0: hi, 1: lo of the split), the 8 input channels of kernel row (j0, j1, j2) with 3 j0 + j1 =
    4*set + g, fastest-axis tap j3 = dx."""
    assert tuple(w.shape) == (8, 8, 3, 3, 3, 3)
    wr = w.reshape(8, 8, 9, 3, 3).float() * SPLIT16_WEIGHT_SCALE       # co, ch, combo (j0, j1), j2, j3
    hi = wr.half()
    lo = (wr - hi.float()).half()
    parts = torch.stack((hi, lo))[:, :, :, :8]                          # part, co, ch, combo (0..7), j2, j3
    v = parts.reshape(2, 8, 8, 2, 4, 3, 3).permute(3, 5, 6, 4, 0, 1, 2)  # set, j2, j3, g, part, co, ch
    stacked = v.reshape(18, 64, 8)
    return torch.cat((stacked, pack_conv_weight_split16_two_site(w).reshape(54, 64, 8))).contiguous()


def pack_conv_weight_split16_first(w):
    """(8, 1, 3, 3, 3, 3) fp32 weights of a first ConvAct layer -> the B fragments of conv_c2_kernel (include/normflow_hip.h,
    nf_conv_first_split16): [K slice (4)][hi|lo][lane (64)][8]; K index = 4 r + t with r the kernel row (j0, j1, j2) row-major
    (27, zero-padded to 32) and t the tap of the site pair; lane 16*g + n (column n = 8*shift + co) holds rows 8*slice + 2*g + h
    (h = 0, 1), taps t = 0..3, as value 4*h + t = W[co][r][t - shift] (zero outside 0..2), scaled by 2^10 and split."""
    assert tuple(w.shape) == (8, 1, 3, 3, 3, 3)
    wr = w.reshape(8, 27, 3).float() * SPLIT16_WEIGHT_SCALE              # co, row, j3
    w2 = wr.new_zeros(16, 32, 4)                                         # column, row (padded), tap
    w2[:8, :27, :3] = wr
    w2[8:, :27, 1:] = wr
    hi = w2.half()
    lo = (w2 - hi.float()).half()
    out = torch.empty(4, 2, 64, 8, dtype=torch.float16, device=w.device)
    for k, part in enumerate((hi, lo)):
        # part[n, r = 8 sl + 2 g + h, t] -> [sl, g, n, h, t]
        v = part.reshape(16, 4, 4, 2, 4).permute(1, 2, 0, 3, 4)          # sl, g, n, h, t
        out[:, k] = v.reshape(4, 64, 8)
    return out.contiguous()


def _first_parity_taps():
    """j3[sigma, shift, r, t'] = the kernel tap W[co][r][j3] that column 8*shift + co multiplies at live tap t' of kernel row r
    (3 = none: a zero) -- include/normflow_hip.h, nf_conv_first_split16: live taps t = 1 - e + 2 t' of the pair's four,
    e = sigma ^ (j0 + j1 + j2 + 1) & 1, j3 = t - shift."""
    j3 = torch.full((2, 2, 32, 2), 3, dtype=torch.long, device='cpu')
    for sigma in range(2):
        for r in range(27):
            e = sigma ^ ((r // 9 + (r // 3) % 3 + r % 3 + 1) & 1)
            for shift in range(2):
                for tp in range(2):
                    j = 1 - e + 2 * tp - shift
                    if 0 <= j <= 2:
                        j3[sigma, shift, r, tp] = j
    return j3


_FIRST_PARITY_TAPS = []
FIRST_FROZEN_FLAG = (0x100, 0x200)        # NF_FIRST_FROZEN_EVEN, NF_FIRST_FROZEN_ODD
FIRST_PARITY_FRAGS = 16 << 16             # NF_FIRST_FRAGS(16): the blob of pack_conv_weight_split16_first_parity


def pack_conv_weight_split16_first_parity(w):
    """(8, 1, 3, 3, 3, 3) fp32 weights of a first ConvAct layer -> the blob a frozen-parity call of nf_conv_first_split16
    takes (include/normflow_hip.h): the 8 dense fragments of `pack_conv_weight_split16_first`, then the parity fragments
    [sigma (2)][K slice (2)][hi|lo][lane (64)][8]: K index = 2 r + t'; lane 16*g + n (column n = 8*shift + co) holds rows
    16*slice + 4*g + h (h = 0..3), live taps t' = 0, 1, as value 2*h + t' = W[co][r][t - shift] with t = 1 - e + 2 t',
    e = sigma ^ (j0 + j1 + j2 + 1) & 1 (zero outside 0..2 and for r >= 27), scaled by 2^10 and split."""
    assert tuple(w.shape) == (8, 1, 3, 3, 3, 3)
    if not _FIRST_PARITY_TAPS:
        _FIRST_PARITY_TAPS.append(_first_parity_taps())
    j3 = _FIRST_PARITY_TAPS[0].to(w.device)
    wr = w.new_zeros(8, 32, 4, dtype=torch.float32)                      # co, row (padded), j3 (3 = the zero)
    wr[:, :27, :3] = w.reshape(8, 27, 3).float() * SPLIT16_WEIGHT_SCALE
    rows = torch.arange(32, device=w.device).view(1, 1, 32, 1).expand_as(j3)
    w2 = wr[:, rows, j3].permute(1, 2, 0, 3, 4).reshape(2, 16, 32, 2)    # sigma, n = 8 shift + co, row, t'
    hi = w2.half()
    lo = (w2 - hi.float()).half()
    out = torch.empty(2, 2, 2, 64, 8, dtype=torch.float16, device=w.device)
    for k, part in enumerate((hi, lo)):
        # part[sigma, n, r = 16 sl + 4 g + h, t'] -> [sigma, sl, g, n, h, t']
        v = part.reshape(2, 16, 2, 4, 4, 2).permute(0, 2, 3, 1, 4, 5)
        out[:, :, k] = v.reshape(2, 2, 64, 8)
    return torch.cat((pack_conv_weight_split16_first(w).reshape(8, 64, 8), out.reshape(8, 64, 8))).contiguous()


def conv_first_split16(x, weight, bias, act, weight_src=None, frozen_parity=None):
    """First ConvAct layer 1 -> 8 on the split-fp16 kernel (nf_conv_first_split16): x (B, 1, *L) fp32 -> the fp16 pair
    tensor (B, V, 16); inference only.  frozen_parity 0 / 1: the caller states that x is non-zero only at the sites whose
    coordinate sum has that parity (the frozen half of a checkerboard coupling); the library then reads those sites only
    where it has the parity-compact instance."""
    lib = load()
    B = x.shape[0]
    lat4 = _lat4(x.shape[2:])
    V = _sites(x.shape[2:])
    if frozen_parity is None:
        wsp = _cached_pack(weight if weight_src is None else weight_src, 'first16', pack_conv_weight_split16_first)
    else:
        wsp = _cached_pack(weight if weight_src is None else weight_src, 'first16p', pack_conv_weight_split16_first_parity)
        act = int(act) | FIRST_FROZEN_FLAG[int(frozen_parity) & 1] | FIRST_PARITY_FRAGS
    bias = None if bias is None else bias.detach().float().contiguous()
    out = torch.empty((B, V, 16), dtype=torch.float16, device=x.device)
    for b0, b1 in _slabs(B, max(1, min(MAX_B, ((1 << 31) - 1) // V))):
        _check(lib.nf_conv_first_split16(_ptr(x[b0:b1]), _ptr(wsp), _ptr(bias), _ptr(out[b0:b1]), b1 - b0, lat4,
                                         int(act), _stream()), "nf_conv_first_split16")
    return out


def _split16_site_index(L3, device):
    """idx[par, slot] = the site x3 of a lattice row stored in slot `slot` of parity block `par` of the fp16 pair layout
    (include/normflow_hip.h, NF_OUT_SPLIT16): even sites in order, odd sites rotated by one slot (slot s holds site 2s-1)."""
    slot = torch.arange(L3 // 2, device=device)
    return torch.stack((2 * slot, (2 * slot - 1) % L3))


def to_split16(h):
    """(B, 8, *L) fp32 hidden activations (|h| <= 1) -> the fp16 pair tensor the split-fp16 kernels exchange, shape
    (B, V, 16) halfs = per lattice row (fastest axis, L3 sites) [hi | lo][even sites | odd sites][L3/2 slots][8 channels]
    with hi = fp16(h), lo = fp16(h - hi) (layout: include/normflow_hip.h, NF_OUT_SPLIT16).  Host-side helper for tests and
    benches: in the pipeline the producing kernel's epilogue writes this format itself."""
    B, Cc = h.shape[:2]
    L3 = h.shape[-1]
    if Cc != 8 or L3 % 2:
        raise NormflowHipError("to_split16: 8 channels and an even fastest axis expected")
    hp = h.reshape(B, 8, -1, L3).float()
    idx = _split16_site_index(L3, h.device)                           # (2, L3/2)
    g = hp[..., idx].permute(0, 2, 3, 4, 1)                           # (B, R, par, slot, channel)
    hi = g.half()
    lo = (g - hi.float()).half()
    return torch.stack((hi, lo), dim=2).reshape(B, -1, 16).contiguous()


def from_split16(h16, lattice):
    """Inverse of to_split16 up to the split's rounding: (B, V, 16) halfs -> (B, 8, *L) fp32 (hi + lo)."""
    B = h16.shape[0]
    L3 = lattice[-1]
    t = h16.reshape(B, -1, 2, 2, L3 // 2, 8).float()
    v = t[:, :, 0] + t[:, :, 1]                                       # (B, R, par, slot, channel)
    idx = _split16_site_index(L3, h16.device)
    out = torch.empty((B, v.shape[1], L3, 8), dtype=torch.float32, device=h16.device)
    out[:, :, idx.reshape(-1)] = v.reshape(B, v.shape[1], L3, 8)
    return out.permute(0, 3, 1, 2).reshape((B, 8) + tuple(lattice)).contiguous()


def conv_layer_split16(h16, weight, bias, act, lattice):
    """Hidden 8 -> 8 layer on fp16 (hi, lo) pairs in and out (nf_conv_fwd_split16); inference only."""
    lib = load()
    B = h16.shape[0]
    lat4 = _lat4(lattice)
    wsp = _cached_pack(weight, 'stacked16', pack_conv_weight_split16_stacked)
    bias = None if bias is None else bias.detach().float().contiguous()
    out = torch.empty_like(h16)
    for b0, b1 in _slabs(B):
        _check(lib.nf_conv_fwd_split16(_ptr(h16[b0:b1]), _ptr(wsp), _ptr(bias), _ptr(out[b0:b1]), b1 - b0, lat4,
                                       int(act), _stream()), "nf_conv_fwd_split16")
    return out


class _PerTensorCache(dict):
    """Values cached per live tensor OBJECT (the parameter a view like Conv4d.weight is based on), `kind` and `state` (the
    caller's tuple of version, address, ...).  The tensor is held by weak reference: when it dies its entries go with it, so a
    new tensor that reuses the freed address never inherits one, and a detached alias or a temporary (a flipped / transposed
    copy made for one call) has no live base and is never found."""
    MISS = object()

    def lookup(self, w, kind, state):
        base = w._base if w._base is not None else w
        hit = self.get((id(base), kind))
        return hit[2] if hit is not None and hit[0]() is base and hit[1] == state else self.MISS

    def store(self, w, kind, state, value):
        base = w._base if w._base is not None else w
        key = (id(base), kind)
        self[key] = (weakref.ref(base, lambda _, k=key: self.pop(k, None)), state, value)
        return value


_UNIT_OK = _PerTensorCache()
_WEIGHT_EPOCH = [0]


def invalidate_weight_checks():
    """Forget every cached verdict of `_weights_fit_fp16` and every cached fragment packing (call after editing weights
    through `.data`, which does not bump a tensor's version counter), and start a new `weight_epoch()`: the per-module
    caches (ConvAct's widened / padded / packed weights) and GraphedFlow's capture key on it."""
    _UNIT_OK.clear()
    _PACKED.clear()
    _WEIGHT_EPOCH[0] += 1


def weight_epoch():
    """Counts the `invalidate_weight_checks()` calls: a cache keyed on (tensor version, data_ptr) must also key on this, since
    a write through `.data` changes neither."""
    return _WEIGHT_EPOCH[0]


_PACKED = _PerTensorCache()
_PACK_IN_CAPTURE = [False]


class pack_inside_capture:
    """While active, a stream capture never takes a cached fragment packing: the repacking kernels are captured with the
    pass, so a graph that is replayed across optimiser steps (graphs.GraphedTrainStep) always multiplies by the CURRENT
    weights.  (GraphedFlow, an inference graph, keeps the cached packing out of its graph and re-captures instead.)"""

    def __enter__(self):
        self._old = _PACK_IN_CAPTURE[0]
        _PACK_IN_CAPTURE[0] = True

    def __exit__(self, *exc):
        _PACK_IN_CAPTURE[0] = self._old
        return False


def _cached_pack(w, kind, fn):
    """fn(w.detach()) -- a weight tensor repacked into a kernel's fragment layout -- cached per live tensor and version
    (`_PerTensorCache`), so that an inference pass does not repack (a dozen small torch kernels per layer and launch) weights
    that have not changed.  A detached alias or a temporary has no live base: it is packed every time."""
    if _PACK_IN_CAPTURE[0] and torch.cuda.is_current_stream_capturing():
        return fn(w.detach())          # a training graph: the packing is part of the graph, replayed on the current values
    state = (w._version, w.data_ptr(), tuple(w.shape), w.dtype)
    out = _PACKED.lookup(w, kind, state)
    if out is _PACKED.MISS:
        out = _PACKED.store(w, kind, state, fn(w.detach()))
    return out


def _weights_fit_fp16(w):
    """finite and inside the fp16 range (the split-fp16 kernel's precondition on the weights); cached per
    parameter version so that the device->host sync happens once per optimiser step, not per launch.
    An entry belongs to one live tensor (`_PerTensorCache`): temporaries are checked every time.
    In-place ops under no_grad (optimizers, `p.copy_`) bump the version; writes through `p.data` do NOT -- after
    those call `invalidate_weight_checks()` (ModelDeviceHandler.broadcast_parameters does).  Under stream capture
    (GraphedFlow) the check cannot run: only an already cached verdict is accepted, so GraphedFlow validates the
    weights eagerly before it captures and must be re-captured after the weights change."""
    state = (w._version, w.data_ptr(), tuple(w.shape))
    ok = _UNIT_OK.lookup(w, None, state)
    if ok is not _UNIT_OK.MISS:
        return ok
    if w.is_cuda and torch.cuda.is_current_stream_capturing():
        return False            # cannot synchronise here; the fp32 kernels are always valid
    ok = bool(torch.isfinite(w.detach()).all()) and float(w.detach().abs().max()) < SPLIT16_WEIGHT_LIMIT
    return _UNIT_OK.store(w, None, state, ok)


def conv_supported(x, weight):
    return (x.is_cuda and x.dtype in (torch.float32, torch.float64) and weight.dtype == x.dtype
            and 1 <= x.dim() - 2 <= 4)


_GATHER_MAPS = {}


def _gather_map(shape, device, build, key):
    """(source index of every element, shape) of build(w) for weights w of this shape -- a pure re-arrangement of the weights
    with zero padding (two-site expansion, fragment order, row packing: a dozen small torch kernels) -- found once per `key` by
    running `build` on a tensor of element numbers.  `key` must name everything `build` depends on besides the shape."""
    key = (tuple(shape), device) + key
    ent = _GATHER_MAPS.get(key)
    if ent is None:
        n = _sites(shape)
        probe = torch.arange(1, n + 1, dtype=torch.float64, device=device).reshape(shape)
        packed = build(probe)
        idx = (packed.reshape(-1).round().to(torch.int64) - 1).to(torch.int32).contiguous()      # -1: a zero of the padding
        ent = (idx, tuple(packed.shape))
        _GATHER_MAPS[key] = ent
    return ent


def _pack_by_gather(weight, gather_map):
    """The packing a `_gather_map` describes, as ONE nf_gather_pad launch.  (A training step re-packs every layer's weights
    twice, forward and flipped / transposed for the input gradient: on small lattices those launches were a quarter of the
    step.)"""
    idx, shape = gather_map
    w = weight.contiguous()
    out = torch.empty(shape, dtype=w.dtype, device=w.device)
    _check(load().nf_gather_pad(_ptr(w), _ptr(idx), _ptr(out), idx.numel(), w.numel(), w.element_size(), _stream()), "nf_gather_pad")
    return out


def _conv_weight_map(shape, device, lat4, k4, cin, cout, compact, two_site, transposed, dtype_code):
    """The `_gather_map` that packs (cout, cin, *k) weights (transposed: the input gradient's flipped / transposed weights of a
    (cin, cout, *k) tensor) in the layout nf_conv_fwd reads for this layer.  That layout depends on the library's options
    (NF_OPT_PIPE: row-packed for the persistent kernel, fragment order without it), so the layout code is part of the key."""
    layout = load().nf_conv_weight_layout(lat4, k4, cin, cout, int(compact), 0, dtype_code)
    ksize = list(shape[2:])

    def build(w):
        """the layer's weights (or its flipped / transposed weights: the input gradient's) in the library's fragment layout"""
        if transposed:
            w = w.flip(list(range(2, w.dim()))).transpose(0, 1)
        if two_site:
            # 16 columns: [0, cout) = the layer at site 2p (taps 0..k3-1), [8, 8+cout) = the same
            # channels at site 2p+1 (taps 1..k3): one extra tap along the fastest axis
            w2 = w.new_zeros((16, cin) + tuple(ksize[:-1]) + (ksize[-1] + 1,))
            w2[:cout, ..., :ksize[-1]] = w
            w2[8:8 + cout, ..., 1:] = w
            w = w2
        return conv_weight_for_layer(w, lat4, k4, cin, cout, compact, False, dtype_code)

    return _gather_map(shape, device, build, (transposed, two_site, tuple(lat4), tuple(k4), cin, cout, int(compact), dtype_code,
                                              layout))


def _conv_launch(x, weight, bias, act, compact, parity, weight_src=None, transposed=False, frozen_parity=None):
    """One launch sequence of nf_conv_fwd for a (cout, cin, *k) weight tensor; packs the weights in
    the fragment layout the library will use (two-site column packing for cout <= 8).  transposed: the layer is the INPUT
    GRADIENT of the layer with these weights (flipped taps, channels exchanged)."""
    lib = load()
    B, cin = x.shape[:2]
    lat = list(x.shape[2:])
    cout, ksize = weight.shape[1 if transposed else 0], list(weight.shape[2:])
    d = len(lat)
    lat4, k4 = _lat4(lat, ksize)
    split16 = compact == 2                 # NF_OUT_SPLIT16: the fp16 (hi, lo) pair tensor, (B, V, 16) halfs
    if (split16 and cin == 1 and cout == 8 and d == 4 and x.dtype == torch.float32
            and _weights_fit_fp16(weight if weight_src is None else weight_src)     # (the caller's tensor: its verdict is cached)
            and lib.nf_conv_first_split16_supported(lat4, k4, cout, act)):
        return conv_first_split16(x, weight, bias, act, weight_src, frozen_parity)
    if split16 and not (lib.nf_conv_two_site(cout, 0, lat[-1], ksize[-1]) and cout == 8 and x.dtype == torch.float32):
        raise NormflowHipError("split-fp16 output needs an fp32 two-site layer with 8 output channels")
    two_site = bool(lib.nf_conv_two_site(cout, 0 if split16 else int(compact), lat[-1], ksize[-1]))
    eff_compact = False if (two_site and split16) else compact
    wfrag = _pack_by_gather(weight, _conv_weight_map(weight.shape, weight.device, lat4, k4, cin, cout, eff_compact, two_site,
                                                     transposed, _dtype_code(x)))
    V = _sites(lat)
    if split16:
        out = torch.empty((B, V, 16), dtype=torch.float16, device=x.device)
    else:
        out = torch.empty((B, cout, V // 2) if compact else (B, cout) + tuple(lat), dtype=x.dtype, device=x.device)
    for b0, b1 in _slabs(B):
        _check(lib.nf_conv_fwd(_ptr(x[b0:b1]), _ptr(wfrag), _ptr(bias), _ptr(out[b0:b1]), b1 - b0, lat4, k4,
                               cin, cout, act, int(compact), int(parity), _dtype_code(x), _stream()), "nf_conv_fwd")
    return out


def _compact_to_full(t, lattice, parity):
    """(B, C, V/2) pair-compact -> (B, C, *L) with zeros at the other sites (nf_expand_pairs: the checkerboard is
    rebuilt from the coordinate sum)."""
    _require_device(t)
    B, Cc, Vh = t.shape
    t = t.contiguous()
    full = torch.empty((B, Cc) + tuple(lattice), dtype=t.dtype, device=t.device)
    _check(load().nf_expand_pairs(_ptr(t), _ptr(full), B * Cc, _lat4(lattice), int(parity), _dtype_code(t), _stream()),
           "nf_expand_pairs")
    return full


def absmax_bits(t):
    """nf_absmax_bits: max |t| of an fp32 tensor as float bits in a 1-element int32 device tensor (no host sync)."""
    bits = torch.empty(1, dtype=torch.int32, device=t.device)
    _check(load().nf_absmax_bits(_ptr(t), t.numel(), _ptr(bits), _stream()), "nf_absmax_bits")
    return bits


def conv_weight_grad(x, gz, ksize, bits=None, compact_parity=-1):
    """(grad_weight (cout, cin, *k), grad_bias (cout)) of a circular conv layer from its input x
    (B, cin, *L) and the full-lattice pre-activation cotangent gz (B, cout, *L): nf_conv_wgrad_split16 (4-D lattice networks;
    `bits`: absmax_bits(gz) if the caller has it already), nf_conv_wgrad_sites (layers of few columns: 1- to 3-D kernels;
    bitwise reproducible) or nf_conv_wgrad.  compact_parity 0 / 1: gz is the pair-compact (B, cout, V/2) cotangent of an
    active-site-only layer; the first two kernels read that form: None is returned when the shape does not qualify (the
    caller expands gz and calls again)."""
    lib = load()
    B, cin = x.shape[:2]
    cout = gz.shape[1]
    ntaps = _sites(ksize)
    lat4, k4 = _lat4(x.shape[2:], ksize)
    ncols = lib.nf_conv_wgrad_cols(cin, ntaps)
    gws, gbs = [], []
    for c0 in range(0, cout, 48):
        c1 = min(cout, c0 + 48)
        part = gz if (c0 == 0 and c1 == cout) else gz[:, c0:c1]
        part = part.contiguous()
        buf = torch.zeros(((c1 - c0 + 15) // 16) * 16, ncols, dtype=x.dtype, device=x.device)
        split = (x.dtype == torch.float32 and lib.nf_get_option(OPT_SPLIT16)
                 and lib.nf_conv_wgrad_split16_supported(lat4, k4, cin, c1 - c0))
        sites = not split and bool(lib.nf_conv_wgrad_sites_supported(lat4, k4, cin, c1 - c0, _dtype_code(x)))
        if compact_parity >= 0 and not (split or sites):
            return None
        if compact_parity >= 0 and sites and x.shape[-1] % 2:
            return None
        for b0, b1 in _slabs(B):
            if split:       # fp16 matrix cores, three products per fp32 product (nf_conv_w.hip)
                need = lib.nf_conv_wgrad_split16_workspace(b1 - b0, lat4, cin)
                ws = torch.empty(int(need), dtype=torch.uint8, device=x.device)
                if bits is None:
                    bits = absmax_bits(gz)      # (of the whole cotangent: any power of two that fits the maximum will do)
                _check(lib.nf_conv_wgrad_split16(_ptr(x[b0:b1]), _ptr(part[b0:b1]), _ptr(buf), b1 - b0, lat4, k4, cin,
                                                 c1 - c0, _ptr(bits), int(compact_parity), _ptr(ws), ws.numel(), _stream()),
                       "nf_conv_wgrad_split16")
            elif sites:     # few columns (1- to 3-D kernels): the waves split the sites, fixed-order sums (nf_conv.hip)
                need = lib.nf_conv_wgrad_sites_workspace(k4, cin, c1 - c0, _dtype_code(x))
                ws = torch.empty(int(need), dtype=torch.uint8, device=x.device)
                _check(lib.nf_conv_wgrad_sites(_ptr(x[b0:b1]), _ptr(part[b0:b1]), _ptr(buf), b1 - b0, lat4, k4, cin,
                                               c1 - c0, int(compact_parity), _ptr(ws), ws.numel(), _dtype_code(x), _stream()),
                       "nf_conv_wgrad_sites")
            else:
                _check(lib.nf_conv_wgrad(_ptr(x[b0:b1]), _ptr(part[b0:b1]), _ptr(buf), b1 - b0, lat4, k4, cin,
                                         c1 - c0, _dtype_code(x), _stream()), "nf_conv_wgrad")
        gws.append(buf[:c1 - c0, :ntaps * cin])
        gbs.append(buf[:c1 - c0, ntaps * cin])
    gw = torch.cat(gws) if len(gws) > 1 else gws[0]
    gb = torch.cat(gbs) if len(gbs) > 1 else gbs[0]
    gw = gw.reshape(cout, ntaps, cin).permute(0, 2, 1).reshape((cout, cin) + tuple(ksize))
    return gw, gb


def conv_input_grad_split16(gz, wt, bits=None, compact_parity=-1, lattice=None, weight=None):
    """Gradient w.r.t. the input of a 3^4 layer with up to 8 input channels on the split-fp16 chain: gz (B, C, *L) fp32 cotangent
    of the layer's pre-activation, wt (cin, C, 3, 3, 3, 3) its weights flipped and transposed.  The C channels go through the
    hidden-layer kernel in groups of 8 (nf_planes_to_split16 + nf_conv_dgrad_split16).  None when the shape does not qualify
    (the caller then runs the fp32 kernel)."""
    lib = load()
    cin = wt.shape[0]                  # channels of the layer's input = of the gradient (fewer than 8: zero weight rows)
    if compact_parity < 0:
        lattice = tuple(gz.shape[2:])
    if (gz.dtype != torch.float32 or lattice is None or len(lattice) != 4 or cin > 8 or tuple(wt.shape[2:]) != (3, 3, 3, 3)
            or not lib.nf_get_option(OPT_SPLIT16)):
        return None
    B, Cc = gz.shape[:2]
    lat4, k4 = _lat4(lattice, (3, 3, 3, 3))
    if not lib.nf_conv_split16_supported(lat4, k4, 8, 8, ACT_CODES['tanh']) or B > 65535:
        return None
    if not _weights_fit_fp16(wt if weight is None else weight):      # (`weight`: the layer's parameter, whose verdict is cached)
        return None
    G = (Cc + 7) // 8
    V = _sites(lattice)
    gz = gz.contiguous()
    g16 = torch.empty((G, B, V, 16), dtype=torch.float16, device=gz.device)
    if bits is None:
        bits = absmax_bits(gz)
    _check(lib.nf_planes_to_split16(_ptr(gz), _ptr(g16), _ptr(bits), B, Cc, lat4, int(compact_parity), _stream()),
           "nf_planes_to_split16")
    gx = torch.empty((B, 8) + tuple(lattice), dtype=torch.float32, device=gz.device)
    wpad = wt.new_zeros((8, 8 * G, 3, 3, 3, 3), dtype=torch.float32)
    wpad[:cin, :Cc] = wt.float()
    for g in range(G):
        wsp = pack_conv_weight_split16_stacked(wpad[:, 8 * g:8 * g + 8].contiguous())
        _check(lib.nf_conv_dgrad_split16(_ptr(g16[g]), _ptr(wsp), None, _ptr(gx), B, lat4, _ptr(bits), int(g > 0), 0,
                                         _stream()), "nf_conv_dgrad_split16")
    return gx if cin == 8 else gx[:, :cin].contiguous()


def conv_hidden_planes_split16(x, weight, bias, act):
    """A forward 8 -> 8 layer (3^4, tanh or no activation) on the split-fp16 chain with fp32 planes in and out -- the form
    autograd keeps (ConvFn): nf_absmax_bits + nf_planes_to_split16 + nf_conv_dgrad_split16.  None when the shape does not qualify."""
    lib = load()
    if (x.dtype != torch.float32 or x.dim() != 6 or tuple(weight.shape) != (8, 8, 3, 3, 3, 3) or act not in (0, ACT_CODES['tanh'])
            or not lib.nf_get_option(OPT_SPLIT16)):
        return None
    B = x.shape[0]
    lattice = tuple(x.shape[2:])
    lat4, k4 = _lat4(lattice, (3, 3, 3, 3))
    if not lib.nf_conv_split16_supported(lat4, k4, 8, 8, ACT_CODES['tanh']) or B > 65535 or not _weights_fit_fp16(weight):
        return None
    V = x[0, 0].numel()
    x16 = torch.empty((1, B, V, 16), dtype=torch.float16, device=x.device)
    bits = absmax_bits(x)                        # (any input range: the pair tensor is scaled like a cotangent's)
    _check(lib.nf_planes_to_split16(_ptr(x), _ptr(x16), _ptr(bits), B, 8, lat4, -1, _stream()), "nf_planes_to_split16")
    wsp = pack_conv_weight_split16_stacked(weight.detach().float())
    out = torch.empty_like(x)
    b = None if bias is None else bias.detach().float().contiguous()
    _check(lib.nf_conv_dgrad_split16(_ptr(x16[0]), _ptr(wsp), _ptr(b), _ptr(out), B, lat4, _ptr(bits), 0, int(act), _stream()),
           "nf_conv_dgrad_split16")
    return out


def conv_last_logits_split16(x, weight, bias, parity):
    """The forward 8 -> 46 layer at the active sites of parity `parity` on the split-fp16 kernel, logits pair-compact
    (B, 46, V/2) -- the form autograd keeps (ConvFn with compact=True): nf_absmax_bits + nf_conv_last_logits_split16.  None
    when the shape does not qualify (a fastest axis of 32 + 16 n sites; other than 32: through a pair tensor)."""
    lib = load()
    if (x.dtype != torch.float32 or x.dim() != 6 or tuple(weight.shape) != (46, 8, 3, 3, 3, 3) or x.shape[1] != 8
            or x.shape[-1] < 32 or x.shape[-1] % 16 or any(n < 2 or n % 2 for n in x.shape[2:5])
            or not lib.nf_get_option(OPT_SPLIT16) or not _weights_fit_fp16(weight)):
        return None
    B = x.shape[0]
    lat4 = _lat4(x.shape[2:])
    V = x[0, 0].numel()
    bits = absmax_bits(x)
    wsp = pack_conv_weight_split16(weight.detach().float())
    b = None if bias is None else bias.detach().float().contiguous()
    out = torch.empty((B, 46, V // 2), dtype=torch.float32, device=x.device)
    src, is16 = FusedLastRqsFn._source(x, bits, lat4)
    _check(lib.nf_conv_last_logits_split16(_ptr(src), is16, _ptr(wsp), _ptr(b), _ptr(out), B, lat4, int(parity), _ptr(bits),
                                           _stream()), "nf_conv_last_logits_split16")
    return out


def pack_wide_split16(w1, b1, w2, b2, w3, b3):
    """Weights of a stack 1 -> h -> h -> C with 8 < h <= 16 (3^4 kernels) for `conv_wide_logits_split16`: the hidden channels
    zero-padded to 16 and cut into two groups of 8 -- [first-layer fragments x 2, biases x 2], [two-site fragments of the four
    8 x 8 blocks of the hidden layer (stacked + two-site), biases x 2], [last-layer fragments x 2, bias]."""
    h, cout = w1.shape[0], w3.shape[0]
    f = lambda t: t.detach().float()
    w1p = f(w1).new_zeros((16, 1, 3, 3, 3, 3)); w1p[:h] = f(w1)
    w2p = f(w2).new_zeros((16, 16, 3, 3, 3, 3)); w2p[:h, :h] = f(w2)
    w3p = f(w3).new_zeros((cout, 16, 3, 3, 3, 3)); w3p[:, :h] = f(w3)
    padb = lambda b, n: None if b is None else torch.nn.functional.pad(f(b), (0, n - b.shape[0]))
    b1p, b2p = padb(b1, 16), padb(b2, 16)
    cut = lambda b, g: None if b is None else b[8 * g:8 * g + 8].contiguous()
    first = [(pack_conv_weight_split16_first(w1p[8 * g:8 * g + 8].contiguous()), cut(b1p, g)) for g in (0, 1)]
    hidden = [[pack_conv_weight_split16_stacked(w2p[8 * go:8 * go + 8, 8 * gi:8 * gi + 8].contiguous()) for gi in (0, 1)] for go in (0, 1)]
    last = [pack_conv_weight_split16(w3p[:, 8 * gi:8 * gi + 8].contiguous()) for gi in (0, 1)]
    return first, (hidden, [cut(b2p, 0), cut(b2p, 1)]), (last, None if b3 is None else f(b3).contiguous()), cout


def conv_wide_logits_split16(x, packed, act1, parity):
    """The raw output (B, C, V/2) at the active sites of a ConvAct stack 1 -> h -> h -> C with hidden widths 9 .. 16 and tanh
    hidden activations on a 4-D lattice, composed from the split-fp16 kernels in groups of 8 channels: the first layer twice
    (nf_conv_first_split16), the four 8 x 8 blocks of the hidden layer through nf_conv_dgrad_split16 (fp32 planes out, the second
    block of a group added to the first, tanh of the sum) + nf_planes_to_split16, the last layer twice (nf_conv_last_logits_split16,
    the second group added).  x: (B, 1, *L) fp32.  Twice as fast as the fp32 MFMA kernels on this shape (tools/hidden16_bench.py)."""
    lib = load()
    first, (hidden, hb), (last, b3), cout = packed
    B = x.shape[0]
    lattice = tuple(x.shape[2:])
    lat4 = _lat4(lattice)
    V = x[0, 0].numel()
    x = x.contiguous()
    tanh = ACT_CODES['tanh']
    h1 = []
    for wsp, b in first:
        out = torch.empty((B, V, 16), dtype=torch.float16, device=x.device)
        _check(lib.nf_conv_first_split16(_ptr(x), _ptr(wsp), _ptr(b), _ptr(out), B, lat4, int(act1), _stream()), "nf_conv_first_split16")
        h1.append(out)
    h2 = []
    z = torch.empty((B, 8) + lattice, dtype=torch.float32, device=x.device)
    for go in (0, 1):
        for gi in (0, 1):
            _check(lib.nf_conv_dgrad_split16(_ptr(h1[gi]), _ptr(hidden[go][gi]), _ptr(hb[go]) if gi == 0 else None, _ptr(z), B, lat4, None,
                                             int(gi > 0), tanh if gi == 1 else 0, _stream()), "nf_conv_dgrad_split16")
        out = torch.empty((1, B, V, 16), dtype=torch.float16, device=x.device)
        _check(lib.nf_planes_to_split16(_ptr(z), _ptr(out), None, B, 8, lat4, -1, _stream()), "nf_planes_to_split16")
        h2.append(out)
    del h1
    logits = torch.empty((B, cout, V // 2), dtype=torch.float32, device=x.device)
    for gi in (0, 1):
        _check(lib.nf_conv_last_logits_split16_acc(_ptr(h2[gi]), 1, _ptr(last[gi]), _ptr(b3) if gi == 0 else None, _ptr(logits), B, lat4,
                                                   int(parity), None, int(gi > 0), int(cout), _stream()), "nf_conv_last_logits_split16_acc")
    return logits


class ConvFn(torch.autograd.Function):
    """One circular conv layer + activation, forward and backward on the MFMA kernels:
    forward nf_conv_fwd; backward nf_act_vjp, nf_conv_fwd with flipped / transposed weights
    (grad_input) and the persistent nf_conv_wgrad kernel (grad_weight, grad_bias)."""

    @staticmethod
    def forward(ctx, x, weight, bias, act, compact, parity):
        _require_device(x, weight, bias)
        x = x.contiguous()
        out = None
        if not compact and x.dim() == 6 and x.shape[1] == 8 and weight.shape[0] == 8:
            out = conv_hidden_planes_split16(x, weight, bias, act)      # 8 -> 8 layer of a lattice network: the split-fp16 kernel
        elif compact and act == 0 and x.dim() == 6 and weight.shape[0] == 46:
            out = conv_last_logits_split16(x, weight, bias, parity)     # ... and its 8 -> 46 layer at the active sites
        if out is None:
            out = _conv_launch(x, weight.detach(), bias, act, compact, parity, weight_src=weight)
        ctx.save_for_backward(x, weight, out if act else None)
        ctx.act, ctx.compact, ctx.parity, ctx.has_bias = act, compact, parity, bias is not None
        return out

    @staticmethod
    def backward(ctx, gout):
        x, weight, y = ctx.saved_tensors
        lib = load()
        gout = gout.contiguous()
        gz = gout
        if ctx.act:
            gz = torch.empty_like(gout)
            _check(lib.nf_act_vjp(_ptr(gout), _ptr(y), _ptr(gz), gout.numel(), ctx.act, _dtype_code(gout),
                                  _stream()), "nf_act_vjp")
        lattice = tuple(x.shape[2:])
        split_ok = gz.dtype == torch.float32 and len(lattice) == 4 and bool(lib.nf_get_option(OPT_SPLIT16))
        bits = absmax_bits(gz) if split_ok else None
        want_w = ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2])
        kdims = list(range(2, weight.dim()))
        # the input gradient's weights (flipped taps, channels exchanged), made when a kernel needs them as a tensor
        wt = (lambda: weight.detach().flip(kdims).transpose(0, 1).contiguous()) if ctx.needs_input_grad[0] else None
        gx = gw = gb = None
        if ctx.compact:
            # the pair-compact cotangent as it is: the split-fp16 kernels and the few-column weight-gradient kernel read that
            # form, no expanded copy
            gzc = gz.reshape(x.shape[0], weight.shape[0], -1).contiguous()
            if wt is not None and split_ok:
                gx = conv_input_grad_split16(gzc, wt(), bits, ctx.parity, lattice, weight)
            if want_w:
                got = conv_weight_grad(x, gzc, weight.shape[2:], bits, ctx.parity)
                if got is not None:
                    gw, gb = got
        need_full = (wt is not None and gx is None) or (want_w and gw is None)
        if need_full:
            if ctx.compact:
                gz = _compact_to_full(gz, lattice, ctx.parity)
            gz = gz.reshape((x.shape[0], weight.shape[0]) + lattice).contiguous()
            if wt is not None and gx is None:
                gx = conv_input_grad_split16(gz, wt(), bits, weight=weight) if split_ok else None
                if gx is None:
                    gx = _conv_launch(gz, weight.detach(), None, 0, False, 0, transposed=True)
            if want_w and gw is None:
                gw, gb = conv_weight_grad(x, gz, weight.shape[2:], bits)
        if not ctx.has_bias:
            gb = None
        return gx, gw, gb, None, None, None


def fused_last_rqs_trainable(h, weight):
    """Does the differentiable fused node (FusedLastRqsFn) take this last layer?  h: (B, 8, *L) fp32 hidden activations."""
    lib = load()
    if (h.dtype != torch.float32 or h.dim() != 6 or h.shape[1] != 8 or weight.dim() != 6 or weight.shape[1] != 8
            or tuple(weight.shape[2:]) != (3, 3, 3, 3) or weight.shape[0] > 46 or (weight.shape[0] + 2) % 3
            or not lib.nf_get_option(OPT_SPLIT16)):
        return False
    lat4 = _lat4(h.shape[2:])
    return bool(lib.nf_conv_rqs_split16_supported(lat4, weight.shape[0], (weight.shape[0] + 2) // 3)) and _weights_fit_fp16(weight)


class FusedLastRqsFn(torch.autograd.Function):
    """The last ConvAct layer (8 -> 3m-2 at the active sites) and the RQ-spline coupling as ONE differentiable node on the
    split-fp16 kernel: forward nf_conv_rqs_split16_train, backward nf_conv_rqs_split16_vjp (logits recomputed in the
    kernel, cotangents through the spline) + the weight / input gradient kernels on the pair-compact logit cotangent.
    The (B, 3m-2, V/2) logits are never materialised -- only their cotangent is, once, in the backward pass."""

    @staticmethod
    def _source(h, bits, lat4):
        """The kernel's view of the hidden activations: fp32 planes for whole-row segments, else the pair tensor."""
        if h.shape[-1] == 32:
            return h, 0
        B, V = h.shape[0], h[0, 0].numel()
        src = torch.empty((1, B, V, 16), dtype=torch.float16, device=h.device)
        _check(load().nf_planes_to_split16(_ptr(h), _ptr(src), _ptr(bits), B, 8, lat4, -1, _stream()), "nf_planes_to_split16")
        return src, 1

    @staticmethod
    def forward(ctx, h, weight, bias, x_active, log0, parity, opts, inverse):
        _require_device(h, weight, bias, x_active, log0)
        lib = load()
        h, x_active = h.contiguous(), x_active.contiguous()
        B, V = x_active.shape
        lat4 = _lat4(h.shape[2:])
        bits = absmax_bits(h)
        src, is16 = FusedLastRqsFn._source(h, bits, lat4)
        wsp = pack_conv_weight_split16(weight.detach().float())
        b = None if bias is None else bias.detach().float().contiguous()
        y = torch.empty_like(x_active)
        logj = torch.empty(B, dtype=torch.float32, device=h.device)
        ws = _workspace(B, V, h.device)        # ONE launch over the whole batch (batch x boxes work items): no slabs here
        _check(lib.nf_conv_rqs_split16_train(_ptr(src), is16, _ptr(wsp), _ptr(b), weight.shape[0], _ptr(x_active), _ptr(log0),
                                             _ptr(y), _ptr(logj), B, lat4, int(parity), _ptr(bits), C.byref(opts),
                                             int(bool(inverse)), _ptr(ws), ws.numel(), _stream()), "nf_conv_rqs_split16_train")
        ctx.save_for_backward(h, weight, bias, y if inverse else x_active)
        ctx.parity, ctx.opts, ctx.inverse, ctx.has_log0 = parity, opts, inverse, log0 is not None
        return y, logj

    @staticmethod
    def backward(ctx, gy, glogj):
        h, weight, bias, xpt = ctx.saved_tensors
        lib = load()
        B, V = xpt.shape
        if ctx.needs_input_grad[0] and B > 65535:      # before anything is launched: nf_conv_dgrad_split16 takes no more
            raise NormflowHipError(f"FusedLastRqsFn.backward: batch {B} > 65535, the limit of the split-fp16 input-gradient "
                                   "kernel (nf_conv_dgrad_split16): split the batch")
        lattice = tuple(h.shape[2:])
        lat4 = _lat4(lattice)
        cout = weight.shape[0]
        bits = absmax_bits(h)
        src, is16 = FusedLastRqsFn._source(h, bits, lat4)
        wsp = pack_conv_weight_split16(weight.detach().float())
        b = None if bias is None else bias.detach().float().contiguous()
        gz = torch.empty((B, cout, V // 2), dtype=torch.float32, device=h.device)
        gx = torch.empty_like(xpt)
        # The logit cotangent gz is a materialised fp32 tensor of products cotangent x spline derivative: below cotangents of
        # ~1e-30 its entries are subnormal and lose bits.  Everything here is linear in (gy, glogj): run it on the cotangents
        # times the power of two that brings their largest entry to [1, 2) and scale the gradients back (exact, no sync).
        gy, glogj = gy.contiguous(), glogj.contiguous()
        work = torch.empty(4, dtype=torch.float32, device=h.device)           # [bits of the two maxima][2^c][2^-c]
        _check(lib.nf_cotangent_pow2(_ptr(gy), gy.numel(), _ptr(glogj), glogj.numel(), _ptr(work), _stream()), "nf_cotangent_pow2")
        gys, gls = torch._foreach_mul([gy, glogj], work[2])
        _check(lib.nf_conv_rqs_split16_vjp(_ptr(src), is16, _ptr(wsp), _ptr(b), cout, _ptr(xpt), _ptr(gys),
                                           _ptr(gls), _ptr(gz), _ptr(gx), B, lat4, int(ctx.parity), _ptr(bits),
                                           C.byref(ctx.opts), int(bool(ctx.inverse)), _stream()), "nf_conv_rqs_split16_vjp")
        gh = gw = gb = None
        gbits = absmax_bits(gz)
        if ctx.needs_input_grad[0]:
            wt = weight.detach().flip([2, 3, 4, 5]).transpose(0, 1).contiguous()
            gh = conv_input_grad_split16(gz, wt, gbits, ctx.parity, lattice, weight)
        if ctx.needs_input_grad[1] or (bias is not None and ctx.needs_input_grad[2]):
            got = conv_weight_grad(h, gz, weight.shape[2:], gbits, ctx.parity)
            if got is not None:
                gw, gb = got
        if (ctx.needs_input_grad[0] and gh is None) or ((ctx.needs_input_grad[1] or ctx.needs_input_grad[2]) and gw is None):
            raise NormflowHipError("FusedLastRqsFn.backward: the split-fp16 gradient kernels refused a layer the forward pass took")
        if bias is None:
            gb = None
        torch._foreach_mul_([t for t in (gh, gw, gb, gx) if t is not None], work[3])
        return gh, gw, gb, gx, (glogj if ctx.has_log0 else None), None, None, None


def conv_layer(x, weight, bias, act=0, compact=False, parity=0, frozen_parity=None):
    """Circular 'same' conv + activation on the HIP kernel; differentiable.  frozen_parity (0 / 1, inference with compact=2
    only): x is zero off the sites of that coordinate-sum parity -- `conv_first_split16`; ignored by every other path, which
    reads x as it is."""
    if torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad or (bias is not None and bias.requires_grad)):
        if act == 5:      # |.| hides the sign its derivative needs: keep the activation outside
            return torch.abs(ConvFn.apply(x, weight, bias, 0, compact, parity))
        return ConvFn.apply(x, weight, bias, act, compact, parity)
    x = x.contiguous()
    return _conv_launch(x, weight.detach(), None if bias is None else bias.detach(), act, compact, parity, weight_src=weight,
                        frozen_parity=frozen_parity if compact == 2 else None)


def conv_affine_split16(h16, weight, bias, x_active, log0, parity, inverse, lattice, out=None):
    """Fused last layer of an affine coupling's net + the coupling (nf_conv_affine_split16); inference only.
    h16: the (B, V, 16) fp16 pair tensor of hidden activations; weight (2, 8, 3, 3, 3, 3), bias (2) | None; x_active (B, V)
    fp32 or half; returns (y (B, V), logJ (B) fp32 / the field's fp32-or-wider dtype)."""
    _require_device(h16, weight, bias, x_active, log0)
    lib = load()
    B, V = x_active.shape
    x_active = x_active.contiguous()
    lat4 = _lat4(lattice)
    def pack_affine(w):
        w8 = w.new_zeros((8, 8, 3, 3, 3, 3), dtype=torch.float32)
        w8[:2] = w.float()
        return pack_conv_weight_split16_stacked(w8)
    wsp = _cached_pack(weight, 'affine16s', pack_affine)
    b8 = torch.zeros(8, dtype=torch.float32, device=x_active.device)
    if bias is not None:
        b8[:2] = bias.detach().float()
    field16 = x_active.dtype == torch.float16
    if out is None:
        y = torch.empty_like(x_active)
        logj = torch.empty(B, dtype=torch.float32, device=x_active.device)
    else:
        y, logj = out
    ws = _workspace(min(B, MAX_B), V, x_active.device)
    for b0, b1 in _slabs(B):
        _check(lib.nf_conv_affine_split16(_ptr(h16[b0:b1]), _ptr(wsp), _ptr(b8), _ptr(x_active[b0:b1]), _ptr(_slab(log0, b0, b1)),
                                          _ptr(y[b0:b1]), _ptr(logj[b0:b1]), b1 - b0, lat4, int(parity), int(inverse),
                                          4 if field16 else 0, _ptr(ws), ws.numel(), _stream()), "nf_conv_affine_split16")
    return y, logj


def conv_rqs(h, weight, bias, x_active, log0, parity, opts, inverse, unit_input=False, lattice=None, out=None):
    """Fused last conv layer + RQ-spline coupling (nf_conv_rqs); inference only.
    h: (B, cin, *L) fp32 hidden activations, or -- with `lattice` given -- the (B, V, 16) fp16 (hi, lo) pairs a
    previous conv_layer(..., compact=2) wrote; x_active: (B, V); returns (y (B, V), logJ (B)).  `out` = (y, logJ)
    tensors to fill instead of new ones (contiguous slices of a caller's batch: no concatenation afterwards)."""
    _require_device(h, weight, bias, x_active, log0)
    lib = load()
    h, x_active = h.contiguous(), x_active.contiguous()
    split_in = lattice is not None
    B = h.shape[0]
    cin = weight.shape[1] if split_in else h.shape[1]
    lat = list(lattice) if split_in else list(h.shape[2:])
    lat4, k4 = _lat4(lat, weight.shape[2:])
    V = x_active.shape[1]
    flags = 1 if (unit_input and _weights_fit_fp16(weight)) else 0          # NF_CONV_UNIT_INPUT: |h| <= 1 (tanh outputs)
    field16 = x_active.dtype == torch.float16                                # NF_CONV_FIELD_F16: fp16 field storage
    if field16:
        flags |= 4
    ldt = torch.float32 if field16 else x_active.dtype
    if split_in:
        if not flags or h.dtype != torch.float16 or tuple(h.shape) != (B, V, 16):
            raise NormflowHipError("split-fp16 hidden activations need unit_input and a (B, V, 16) half tensor")
        flags |= 2                                                           # NF_CONV_SPLIT16_INPUT
    fused_code = 1 | ((flags & 1) << 1) | ((flags & 2) << 1)
    kind = ('fused_last', tuple(lat4), tuple(k4), cin, fused_code, lib.nf_get_option(OPT_SPLIT16), lib.nf_get_option(OPT_PIPE))
    wfrag = _cached_pack(weight, kind, lambda w: conv_weight_for_layer(w, lat4, k4, cin, w.shape[0], True, fused_code, NF_F32))
    bias = None if bias is None else bias.detach().contiguous()
    if out is None:
        y = torch.empty_like(x_active)
        logj = torch.empty(B, dtype=ldt, device=x_active.device)
    else:
        y, logj = out
        if (tuple(y.shape) != (B, V) or tuple(logj.shape) != (B,) or y.dtype != x_active.dtype or logj.dtype != ldt
                or not y.is_contiguous() or not logj.is_contiguous()):
            raise NormflowHipError("conv_rqs: `out` must be contiguous (B, V) and (B,) tensors of the input's dtype (log|J| fp32 for a half field)")
        _require_device(y, logj)
    ws = _workspace(min(B, MAX_B), V, h.device)
    for b0, b1 in _slabs(B):
        _check(lib.nf_conv_rqs(_ptr(h[b0:b1]), _ptr(wfrag), _ptr(bias), _ptr(x_active[b0:b1]), _ptr(_slab(log0, b0, b1)),
                               _ptr(y[b0:b1]), _ptr(logj[b0:b1]), b1 - b0, lat4, k4, cin, weight.shape[0],
                               int(parity), C.byref(opts), int(inverse), flags, _ptr(ws), ws.numel(), NF_F32,
                               _stream()), "nf_conv_rqs")
    return y, logj


# ============================================================ small lattices: one kernel per layer
def _split_hi_lo(w):
    w = w.float() * SPLIT16_WEIGHT_SCALE
    hi = w.half()
    return hi, (w - hi.float()).half()


def pack_small3d_weights(w1, w2, w3):
    """(8, 1, 3, 3, 3), (8, 8, 3, 3, 3), (cout <= 48, 8, 3, 3, 3) fp32 weights -> the three fragment tensors of
    nf_small_lattice_coupling (include/normflow_hip.h): scaled by 2^10, split into fp16 (hi, lo)."""
    dev = w1.device
    cout = w3.shape[0]
    assert tuple(w1.shape) == (8, 1, 3, 3, 3) and tuple(w2.shape) == (8, 8, 3, 3, 3) and tuple(w3.shape[1:]) == (8, 3, 3, 3) and cout <= 48
    # w1: A operand rows = output channel (16, 8 used), K = tap (32, 27 used); lane 16 g + row holds k = 8g .. 8g+7
    a1 = torch.zeros(16, 32, device=dev)
    a1[:8, :27] = w1.reshape(8, 27).float()
    p1 = torch.stack([t.reshape(16, 4, 8).permute(1, 0, 2).reshape(64, 8) for t in _split_hi_lo(a1)])            # (2, 64, 8)
    # w2: per kernel row (j0, j1): rows = (site-in-pair s, co), K = (tap g of the pair, ci): w[co][ci][j0][j1][g - s]
    a2 = torch.zeros(9, 16, 4, 8, device=dev)                       # row, m = 8 s + co, g, ci
    wr = w2.float().permute(2, 3, 0, 4, 1).reshape(9, 8, 3, 8)      # (j0 j1), co, j2, ci
    a2[:, :8, 0:3] = wr
    a2[:, 8:, 1:4] = wr
    p2 = torch.stack([t.permute(0, 2, 1, 3).reshape(9, 64, 8) for t in _split_hi_lo(a2)], dim=1)                  # (9, 2, 64, 8)
    # w3: per column tile t and slice i: cols = channel 16 t + n, K = (tap 4 i + g, ci)
    b3 = torch.zeros(48, 28, 8, device=dev)                         # channel, tap, ci
    b3[:cout, :27] = w3.float().reshape(cout, 8, 27).permute(0, 2, 1)
    p3 = torch.stack([t.reshape(3, 16, 7, 4, 8).permute(0, 2, 3, 1, 4).reshape(3, 7, 64, 8) for t in _split_hi_lo(b3)], dim=2)
    return p1.contiguous(), p2.contiguous(), p3.contiguous()        # (2,64,8), (9,2,64,8), (3,7,2,64,8)


def small_lattice_coupling(kind, x_frozen, x_active, packed, biases, log0, parity, cout, acts, opts, inverse, out=None):
    """One launch per coupling layer of a small lattice (nf_small_lattice_coupling): kind 0 RQ-spline, 1 affine;
    x_frozen, x_active: (B, L0, L1, 16) or (B, L1, 16) fp32; packed = pack_small3d_weights(...); biases = (b1, b2, b3) fp32 or
    None each; `out` = (y, logJ) tensors to fill instead of new ones.  Inference only."""
    _require_device(x_frozen, x_active, log0, *packed)
    lib = load()
    B = x_active.shape[0]
    lat = tuple(x_active.shape[1:])
    x_frozen, x_active = x_frozen.contiguous(), x_active.contiguous()
    if out is None:
        y = torch.empty_like(x_active)
        logj = torch.empty(B, dtype=torch.float32, device=x_active.device)
    else:
        y, logj = out
    b1, b2, b3 = (None if b is None else b.detach().float().contiguous() for b in biases)
    _check(lib.nf_small_lattice_coupling(int(kind), _ptr(x_frozen), _ptr(x_active), _ptr(packed[0]), _ptr(b1), _ptr(packed[1]),
                                         _ptr(b2), _ptr(packed[2]), _ptr(b3), _ptr(log0), _ptr(y), _ptr(logj), B, _c_ints(lat), len(lat),
                                         int(parity), int(cout), int(acts[0]), int(acts[1]),
                                         C.byref(opts) if opts is not None else None, int(bool(inverse)), _stream()),
           "nf_small_lattice_coupling")
    return y, logj


# ========================================================================= end points
def endpoint_supported(t):
    return t.is_cuda and t.dtype in (torch.float32, torch.float64) and 1 <= t.dim() - 1 <= 4


class Phi4ActionFn(torch.autograd.Function):
    """Per-sample phi^4 action of (B, *L) configurations, one pass (nf_phi4_action)."""

    @staticmethod
    def forward(ctx, cfgs, w0, w2, w4):
        cfgs = cfgs.contiguous()
        B, lat4 = cfgs.shape[0], _lat4(cfgs.shape[1:])
        out = torch.empty(B, dtype=cfgs.dtype, device=cfgs.device)
        ws = _workspace(min(B, MAX_B), cfgs[0].numel(), cfgs.device)
        for b0, b1 in _slabs(B):
            _check(load().nf_phi4_action(_ptr(cfgs[b0:b1]), _ptr(out[b0:b1]), b1 - b0, lat4, w0, w2, w4, _ptr(ws),
                                         ws.numel(), _dtype_code(cfgs), _stream()), "nf_phi4_action")
        ctx.save_for_backward(cfgs)
        ctx.w = (w0, w2, w4)
        return out

    @staticmethod
    def backward(ctx, g):
        (cfgs,) = ctx.saved_tensors
        B, lat4 = cfgs.shape[0], _lat4(cfgs.shape[1:])
        g = g.contiguous()
        gc = torch.empty_like(cfgs)
        for b0, b1 in _slabs(B):
            _check(load().nf_phi4_action_vjp(_ptr(cfgs[b0:b1]), _ptr(g[b0:b1]), _ptr(gc[b0:b1]), b1 - b0, lat4,
                                             *ctx.w, _dtype_code(cfgs), _stream()), "nf_phi4_action_vjp")
        return gc, None, None, None


class Phi4ActionDensityFn(torch.autograd.Function):
    """Per-site phi^4 action density of (B, *L) configurations, one stencil pass (nf_phi4_action_density); wm = w2 - d w0."""

    @staticmethod
    def forward(ctx, cfgs, w0, wm, w4):
        cfgs = cfgs.contiguous()
        B, lat4 = cfgs.shape[0], _lat4(cfgs.shape[1:])
        out = torch.empty_like(cfgs)
        for b0, b1 in _slabs(B):
            _check(load().nf_phi4_action_density(_ptr(cfgs[b0:b1]), _ptr(out[b0:b1]), b1 - b0, lat4, w0, wm, w4,
                                                 _dtype_code(cfgs), _stream()), "nf_phi4_action_density")
        ctx.save_for_backward(cfgs)
        ctx.w = (w0, wm, w4)
        return out

    @staticmethod
    def backward(ctx, g):
        (cfgs,) = ctx.saved_tensors
        B, lat4 = cfgs.shape[0], _lat4(cfgs.shape[1:])
        g = g.contiguous()
        gc = torch.empty_like(cfgs)
        for b0, b1 in _slabs(B):
            _check(load().nf_phi4_action_density_vjp(_ptr(cfgs[b0:b1]), _ptr(g[b0:b1]), _ptr(gc[b0:b1]), b1 - b0,
                                                     lat4, *ctx.w, _dtype_code(cfgs), _stream()),
                   "nf_phi4_action_density_vjp")
        return gc, None, None, None


class NormalLogProbFn(torch.autograd.Function):
    """Per-sample log-density of independent normals (nf_normal_logprob); loc/scale (V) or None."""

    @staticmethod
    def forward(ctx, x, loc, scale):
        x = x.contiguous()
        B = x.shape[0]
        V = x[0].numel() if B else 0
        out = torch.empty(B, dtype=x.dtype, device=x.device)
        ws = _workspace(min(B, MAX_B), V, x.device)
        for b0, b1 in _slabs(B):
            _check(load().nf_normal_logprob(_ptr(x[b0:b1]), _ptr(loc), _ptr(scale), _ptr(out[b0:b1]), b1 - b0, V,
                                            _ptr(ws), ws.numel(), _dtype_code(x), _stream()), "nf_normal_logprob")
        ctx.save_for_backward(x, loc, scale)
        return out

    @staticmethod
    def backward(ctx, g):
        x, loc, scale = ctx.saved_tensors
        B = x.shape[0]
        V = x[0].numel() if B else 0
        g = g.contiguous()
        gx = torch.empty_like(x)
        for b0, b1 in _slabs(B):
            _check(load().nf_normal_logprob_vjp(_ptr(x[b0:b1]), _ptr(loc), _ptr(scale), _ptr(g[b0:b1]),
                                                _ptr(gx[b0:b1]), b1 - b0, V, _dtype_code(x), _stream()),
                   "nf_normal_logprob_vjp")
        return gx, None, None


def _philox_positions(device, n, generator=None):
    """(seed, first kernel offset) for a launch of a Philox kernel that consumes n consecutive kernel offsets, taken from
    torch's CUDA generator of `device` (or `generator`), which is advanced past all n: torch.manual_seed governs these
    kernels as it does torch's own."""
    gen = generator if generator is not None else torch.cuda.default_generators[device.index if device.index is not None
                                                                                  else torch.cuda.current_device()]
    seed, offset = gen.initial_seed(), gen.get_offset()
    gen.set_offset(offset + 4 * int(n))   # torch keeps offsets in multiples of 4
    return seed & (2 ** 64 - 1), offset // 4


def _philox_position(device, generator=None):
    """(seed, kernel offset) for one call of a Philox kernel: `_philox_positions` with n = 1."""
    return _philox_positions(device, 1, generator)


def normal_sample(loc, scale, batch_size, shape, dtype, device, generator=None):
    """(x (B, *shape), logr (B)) of a NormalPrior in one launch per slab (nf_normal_sample_rows), one stream for the whole
    batch (row b draws the groups b * ngroups + q whatever the slabs), at the `_philox_position` of torch's generator:
    torch.manual_seed(s) makes this kernel reproducible exactly as it does torch's own samplers."""
    seed, offset = _philox_position(device, generator)
    V = _sites(shape)
    x = torch.empty((batch_size,) + tuple(shape), dtype=dtype, device=device)
    logr = torch.empty(batch_size, dtype=dtype, device=device)
    ws = _workspace(min(batch_size, MAX_B), V, device)
    loc = None if loc is None else loc.to(device=device, dtype=dtype).contiguous()
    scale = None if scale is None else scale.to(device=device, dtype=dtype).contiguous()
    for b0, b1 in _slabs(batch_size):
        # one call is one stream at one offset: a slab draws the rows b0 .. b1 of it
        _check(load().nf_normal_sample_rows(_ptr(x[b0:b1]), _ptr(logr[b0:b1]), _ptr(loc), _ptr(scale), b1 - b0, V, b0,
                                            seed, offset, _ptr(ws), ws.numel(), _dtype_code(x), _stream()),
               "nf_normal_sample_rows")
    return x, logr


# ========================================================================= blocked Metropolis (nf_mcmc.hip)
def _block_args(x, backup, block_len, block_ind):
    _require_device(x, backup)
    if not x.is_contiguous() or not backup.is_contiguous():
        raise NormflowHipError("blocked Metropolis kernels need contiguous x and backup")
    Cn = x.shape[0]
    V = x[0].numel() if Cn else x.numel()
    if backup.dtype != x.dtype or backup.numel() != Cn * block_len:
        raise NormflowHipError(f"backup must hold ({Cn}, {block_len}) values of {x.dtype}")
    return Cn, V


def block_propose(x, backup, loc, scale, block_len, block_ind, generator=None):
    """nf_block_propose: block `block_ind` of every chain of x (C, *L) is saved into backup (C, block_len) and redrawn
    from the normal prior (loc / scale (V) or None), in place."""
    Cn, V = _block_args(x, backup, block_len, block_ind)
    for t in (loc, scale):
        if t is not None and (t.dtype != x.dtype or t.device != x.device or t.numel() != V or not t.is_contiguous()):
            raise NormflowHipError("loc / scale must be contiguous (V) tensors of the field's dtype and device")
    seed, offset = _philox_position(x.device, generator)
    _check(load().nf_block_propose(_ptr(x), _ptr(backup), _ptr(loc), _ptr(scale), Cn, V, int(block_len), int(block_ind),
                                   seed, offset, _dtype_code(x), _stream()), "nf_block_propose")


def block_accept(x, backup, logq, logp, logqp_ref, accept_out, block_len, block_ind, force_accept=False, generator=None):
    """nf_block_accept: the Metropolis decision of every chain on the device; logqp_ref (C) float64 is updated where
    accepted, the block of x is restored from backup where rejected, accept_out (C) uint8 gets the flags."""
    Cn, V = _block_args(x, backup, block_len, block_ind)
    _require_device(logq, logp, logqp_ref, accept_out)
    for t, dt in ((logq, x.dtype), (logp, x.dtype), (logqp_ref, torch.float64), (accept_out, torch.uint8)):
        if t.dtype != dt or t.numel() != Cn or not t.is_contiguous():
            raise NormflowHipError(f"block_accept: expected a contiguous ({Cn},) {dt} tensor, got {tuple(t.shape)} {t.dtype}")
    seed, offset = _philox_position(x.device, generator)
    _check(load().nf_block_accept(_ptr(x), _ptr(backup), _ptr(logq), _ptr(logp), _ptr(logqp_ref), _ptr(accept_out), Cn, V,
                                  int(block_len), int(block_ind), int(bool(force_accept)), seed, offset, _dtype_code(x),
                                  _stream()), "nf_block_accept")


# ========================================================================= independence Metropolis, C chains (nf_mcmc.hip)
def _expect(what, t, n, dtype):
    if t.dtype != dtype or t.numel() != n or not t.is_contiguous():
        raise NormflowHipError(f"{what}: expected a contiguous tensor of {n} {dtype} values, got {tuple(t.shape)} {t.dtype}"
                               f"{'' if t.is_contiguous() else ' (not contiguous)'}")


def metropolis_chains(logq, logp, logqp_ref, ref_logq, ref_logp, accept, keep, logq_sel, logp_sel, n_chains, fresh=False,
                      generator=None):
    """nf_metropolis_chains: the decisions of n_chains chains over S = len(logq) // n_chains steps in one launch (row
    r = s C + c).  logqp_ref (C) float64, ref_logq, ref_logp (C) are the chains' stored state, updated in place (not read
    when `fresh`); accept (S C) uint8, keep (S C) int64, logq_sel, logp_sel (S C) are written."""
    Cn = int(n_chains)
    B = logq.numel()
    if logq.dtype not in (torch.float32, torch.float64):
        raise NormflowHipError(f"metropolis_chains: log q must be float32 or float64, got {logq.dtype}")
    if Cn < 1 or B % Cn != 0:
        raise NormflowHipError(f"metropolis_chains: {B} rows are not a multiple of n_chains ({Cn})")
    tensors = (logq, logp, logqp_ref, ref_logq, ref_logp, accept, keep, logq_sel, logp_sel)
    _require_device(*tensors)
    for t, n, dt in ((logq, B, logq.dtype), (logp, B, logq.dtype), (logqp_ref, Cn, torch.float64), (ref_logq, Cn, logq.dtype),
                     (ref_logp, Cn, logq.dtype), (accept, B, torch.uint8), (keep, B, torch.int64), (logq_sel, B, logq.dtype),
                     (logp_sel, B, logq.dtype)):
        _expect("metropolis_chains", t, n, dt)
    seed, offset = _philox_position(logq.device, generator)
    _check(load().nf_metropolis_chains(*(_ptr(t) for t in tensors), B // Cn, Cn, int(bool(fresh)), seed, offset,
                                       _dtype_code(logq), _stream()), "nf_metropolis_chains")


def metropolis_select(y, ref_sample, accept, keep, n_chains):
    """nf_metropolis_select: the rejected rows of y (S C, *L) are overwritten in place with the row keep[r], or with
    ref_sample[r % C] (C, *L; None for fresh chains) while the chain holds its stored sample.  Any field dtype."""
    Cn = int(n_chains)
    B = y.shape[0]
    if Cn < 1 or B % Cn != 0:
        raise NormflowHipError(f"metropolis_select: {B} rows are not a multiple of n_chains ({Cn})")
    _require_device(y, ref_sample, accept, keep)
    if not y.is_contiguous():
        raise NormflowHipError("metropolis_select needs a contiguous y")
    V = y[0].numel() if B else 0
    if ref_sample is not None:
        _expect("metropolis_select (ref_sample)", ref_sample, Cn * V, y.dtype)
    _expect("metropolis_select (accept)", accept, B, torch.uint8)
    _expect("metropolis_select (keep)", keep, B, torch.int64)
    _check(load().nf_metropolis_select(_ptr(y), _ptr(ref_sample), _ptr(accept), _ptr(keep), B // Cn, Cn, V,
                                       y.element_size(), _stream()), "nf_metropolis_select")


# ========================================================================= hybrid Monte Carlo, phi^4 (nf_hmc.hip)
HMC_MAX_WORK = 1 << 26        # NF_HMC_MAX_WORK: the cap on n_md * s * n_traj * max(V, 256) * ceil(C / 1024) of one launch
HMC_MAX_STAGES = 8            # NF_HMC_MAX_STAGES
HMC_SCHEMES = {'leapfrog': 0, 'omelyan': 1, 'omf4': 2}      # NF_HMC_LEAPFROG, NF_HMC_OMELYAN2, NF_HMC_OMF4


class HmcScheme(C.Structure):
    """nf_hmc_scheme (include/normflow_hip.h, "integration schemes"): `stages`, the drift weights `a` and the kick weights
    `b` as tuples, and `name` (one of HMC_SCHEMES, or None for a scheme given by its weights)."""
    _fields_ = [("stages", C.c_int32), ("_a", C.c_double * HMC_MAX_STAGES), ("_b", C.c_double * HMC_MAX_STAGES)]
    name = None

    @property
    def a(self):
        return tuple(self._a[:self.stages])

    @property
    def b(self):
        return tuple(self._b[:self.stages])

    def label(self):
        """What the samplers record in `last['integrator']`: the name, or the pair of weight tuples."""
        return self.name if self.name is not None else (self.a, self.b)

    def __repr__(self):
        return f"HmcScheme({self.name!r}, a={self.a}, b={self.b})"


class _NullScheme:
    """`scheme=NULL_SCHEME`: call the _scheme entry point with a NULL scheme (the library's leapfrog)."""
    stages = 1


NULL_SCHEME = _NullScheme()


def hmc_scheme(which):
    """A validated `HmcScheme`: 'leapfrog', 'omelyan' (the second-order minimum-norm scheme, 2 stages) or 'omf4' (the
    fourth-order one, 5 stages) as the LIBRARY states them (nf_hmc_scheme_named), or a pair (a, b) of sequences of drift
    and kick weights, checked by nf_hmc_scheme_check, which names the broken condition.  An `HmcScheme` is returned as it
    is.  Pure host code."""
    if isinstance(which, HmcScheme):
        return which
    out = HmcScheme()
    if isinstance(which, str):
        if which not in HMC_SCHEMES:
            raise ValueError(f"integrator must be one of {sorted(HMC_SCHEMES)} or a pair (a, b) of weights, got {which!r}")
        _check(load().nf_hmc_scheme_named(HMC_SCHEMES[which], C.byref(out)), "nf_hmc_scheme_named")
        out.name = which
        return out
    try:
        a, b = which
        a, b = [float(x) for x in a], [float(x) for x in b]
    except (TypeError, ValueError):
        raise ValueError(f"integrator must be one of {sorted(HMC_SCHEMES)} or a pair (a, b) of weights, got {which!r}") from None
    if len(a) != len(b):
        raise NormflowHipError(f"hmc_scheme: {len(a)} drift weights and {len(b)} kick weights: one of each per stage")
    out.stages = len(a)
    for j in range(min(len(a), HMC_MAX_STAGES)):          # more stages than the struct holds: refused below by their count
        out._a[j], out._b[j] = a[j], b[j]
    _check(load().nf_hmc_scheme_check(C.byref(out)), "nf_hmc_scheme_check")
    return out


def hmc_fused_budget(V, Cn):
    """The force evaluations (n_md * s * n_traj, s the stages of the scheme, and NF_HMC_MEASURE_MD_STEPS per measured
    trajectory) that one launch of nf_phi4_hmc and its measuring and ladder forms may hold for Cn chains of V sites:
    hmc_entry's rule (nf_hmc.hip)."""
    return HMC_MAX_WORK // (max(int(V), 256) * ((int(Cn) + 1023) // 1024))


def _planner_supported(symbol, lat, dtype):
    """True if the planner `symbol` of the library takes the lattice `lat` (1 to 4 extents) in `dtype`: pure host code."""
    if dtype not in (torch.float32, torch.float64) or not 1 <= len(lat) <= 4:
        return False
    return bool(getattr(load(), symbol)(_lat4(lat), NF_F32 if dtype == torch.float32 else NF_F64))


def _planner_plan(what, symbol, lat, dtype, out):
    """`out` filled by the planner `symbol` for the lattice `lat` (1 to 4 axes) in `dtype`; a dtype that is neither float32
    nor float64 goes down as NF_F16, which the planners refuse in their own words."""
    if not 1 <= len(lat) <= 4:
        raise NormflowHipError(f"{what}: lattices of 1 to 4 axes, got {tuple(lat)}")
    code = NF_F32 if dtype == torch.float32 else NF_F64 if dtype == torch.float64 else NF_F16
    _check(getattr(load(), symbol)(_lat4(lat), code, C.byref(out)), symbol)
    return out


HMC_MEASURE_MD_STEPS = 16     # NF_HMC_MEASURE_MD_STEPS: the MD steps a measured trajectory counts as under the cap


class HmcPlan(C.Structure):
    """nf_hmc_plan (include/normflow_hip.h)."""
    _fields_ = [("sites_per_lane", C.c_int32), ("lanes", C.c_int32), ("lds_bytes", C.c_int64),
                ("lds_bytes_measure", C.c_int64)]


def hmc_plan(lat, dtype):
    """What nf_phi4_hmc will do on the lattice `lat` in `dtype`: dict(sites_per_lane, lanes (of a chain's workgroup),
    lds_bytes, lds_bytes_measure (of nf_phi4_hmc_measure)).  Pure host code."""
    out = _planner_plan("hmc_plan", "nf_phi4_hmc_plan", lat, dtype, HmcPlan())
    return dict(sites_per_lane=out.sites_per_lane, lanes=out.lanes, lds_bytes=out.lds_bytes,
                lds_bytes_measure=out.lds_bytes_measure)


class ConvPlan(C.Structure):
    """nf_conv_layer_plan (include/normflow_hip.h)."""
    _fields_ = [("path", C.c_int32), ("weight_layout", C.c_int32), ("mt", C.c_int32), ("two_site", C.c_int32),
                ("packed", C.c_int32), ("box", C.c_int32 * 4), ("nbox", C.c_int32 * 4), ("plane_stride", C.c_int32),
                ("channels_per_pass", C.c_int32), ("launches", C.c_int32), ("lds_bytes", C.c_int64),
                ("partials", C.c_int64)]


def conv_plan(lat, ksize, cin, cout, compact=0, fused=0, dtype=torch.float32, B=1):
    """What nf_conv_fwd (fused = 0; compact 0, 1 or 2 = NF_OUT_SPLIT16) or nf_conv_rqs (fused = 1, | 2 unit input, | 4
    pair-tensor input: nf_conv_weight_layout's bits) will do with a layer of `cin` -> `cout` channels and kernel extents
    `ksize` on the lattice `lat` (1 to 4 axes) for a batch of B, under the library's current options: dict(path (the
    nf_conv_last_path code), weight_layout, mt, two_site, packed, box, nbox, plane_stride, channels_per_pass, launches,
    lds_bytes, partials (log-det partials per sample)).  A layer the library refuses raises with its message.  Pure host
    code."""
    if not 1 <= len(lat) <= 4 or len(ksize) != len(lat):
        raise NormflowHipError(f"conv_plan: lattices of 1 to 4 axes and one kernel extent per axis, got {tuple(lat)}, {tuple(ksize)}")
    code = NF_F32 if dtype == torch.float32 else NF_F64 if dtype == torch.float64 else NF_F16
    lat4, k4 = _lat4(list(lat), list(ksize))
    out = ConvPlan()
    _check(load().nf_conv_plan(lat4, k4, int(cin), int(cout), int(compact), int(fused), code, int(B), C.byref(out)),
           "nf_conv_plan")
    return {name: (list(getattr(out, name)) if name in ("box", "nbox") else getattr(out, name)) for name, _ in ConvPlan._fields_}


def hmc_supported(lat, dtype):
    """True if nf_phi4_hmc takes chains on the lattice `lat` (1 to 4 extents) in `dtype`: the launcher's own planner,
    pure host code."""
    return _planner_supported("nf_phi4_hmc_supported", lat, dtype)


def _ladder_tensors(what, coef, rung, Cn, dev):
    """(K, the ctypes arguments (coef, K, rung)) of a ladder call after the checks the library cannot make: device, dtype,
    shape and contiguity of the table coef (K, 3) float64 and of rung (C) int32."""
    for name, t, dt in (("coef", coef, torch.float64), ("rung", rung, torch.int32)):
        if not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != dt or not t.is_contiguous():
            raise NormflowHipError(f"{what}: {name} must be a contiguous {dt} tensor on {dev}, got "
                                   f"{getattr(t, 'dtype', type(t).__name__)} on {getattr(t, 'device', None)}")
    if coef.ndim != 2 or coef.shape[1] != 3 or coef.shape[0] < 1:
        raise NormflowHipError(f"{what}: coef must be (K, 3) with K >= 1: (w0, w2, w4) per rung, got {tuple(coef.shape)}")
    K = coef.shape[0]
    if tuple(rung.shape) != (Cn,):
        raise NormflowHipError(f"{what}: rung must be ({Cn},), one rung per chain, got {tuple(rung.shape)}")
    if Cn % K != 0:
        raise NormflowHipError(f"{what}: the {Cn} chains are not a multiple of the K = {K} rungs")
    return K, (_ptr(coef), K, _ptr(rung))


def _phi4_hmc_call(what, phi, w0, w2, w4, n_md, dt, *, n_traj, record_every, pi_in, want_pi, force_accept, position,
                   generator, workspace=None, record=True, ladder=None, measure=False, scheme=None):
    """The body of `phi4_hmc` and `phi4_hmc_tiled` (`what`; the library's entry point is nf_<what>; "phi4_hmc_measure" is
    `phi4_hmc(measure=True)`) and of their ladder forms ("phi4_hmc_ladder", "phi4_hmc_tiled_ladder": `ladder` = (coef,
    rung) replaces the three scalars): the argument checks, the output tensors, the Philox positions, the call and the
    dict.  Only the tiled kernels have a workspace; only the measuring entry points have `measure` (the fused ladder
    where asked: `measure`), and rows only where `record`.  `scheme`: None calls nf_<what> (leapfrog, the call as it
    always was); an `HmcScheme` (or what `hmc_scheme` takes) or NULL_SCHEME calls nf_<what>_scheme."""
    tiled = what in ("phi4_hmc_tiled", "phi4_hmc_tiled_ladder")
    has_measure_arg = what in ("phi4_hmc_measure", "phi4_hmc_ladder")
    measures = what == "phi4_hmc_measure" or (what == "phi4_hmc_ladder" and measure)
    _require_device(phi, pi_in)
    if not phi.is_contiguous() or (pi_in is not None and (not pi_in.is_contiguous() or pi_in.dtype != phi.dtype
                                                            or pi_in.shape != phi.shape)):
        raise NormflowHipError(f"{what} needs contiguous phi (C, *L) and pi_in of its shape and dtype")
    Cn, lat, dev = phi.shape[0], tuple(phi.shape[1:]), phi.device
    if not 1 <= len(lat) <= 4:
        raise NormflowHipError(f"{what}: lattices of 1 to 4 axes, got {lat}")
    n_traj = int(n_traj)
    dh = torch.empty((max(n_traj, 0), Cn), dtype=torch.float64, device=dev)
    accept = torch.empty((max(n_traj, 0), Cn), dtype=torch.uint8, device=dev)
    action = torch.empty(Cn, dtype=torch.float64, device=dev)
    rows = None if record_every is None else (n_traj // int(record_every), Cn)
    want_record, record = record, None
    if rows is not None and want_record:
        record = torch.empty(rows + lat, dtype=phi.dtype, device=dev)
    measure = None
    if measures:
        if rows is None:
            raise NormflowHipError("phi4_hmc(measure=True) needs record_every: which trajectories to measure")
        measure = torch.empty(rows + (measure_n_out(lat),), dtype=torch.float64, device=dev)
    pi_out = torch.empty_like(phi) if want_pi else None
    if tiled and workspace is None:
        workspace = torch.empty(max(hmc_tiled_workspace(Cn, lat, phi.dtype), 256), dtype=torch.uint8, device=dev)
    ws = (_ptr(workspace), workspace.numel()) if tiled else ()
    couplings = (float(w0), float(w2), float(w4)) if ladder is None else _ladder_tensors(what, *ladder, Cn, dev)[1]
    symbol, tail = "nf_" + what, ()
    if scheme is not None:
        if scheme is not NULL_SCHEME:
            scheme = hmc_scheme(scheme)
        symbol, tail = symbol + "_scheme", (None if scheme is NULL_SCHEME else C.byref(scheme),)
    seed, offset = position if position is not None else _philox_positions(dev, 2 * max(n_traj, 1), generator)
    _check(getattr(load(), symbol)(_ptr(phi), _ptr(action), _ptr(pi_in), _ptr(pi_out), _ptr(dh), _ptr(accept),
                                         _ptr(record), *((_ptr(measure),) if has_measure_arg else ()),
                                         1 if record_every is None else int(record_every), Cn, _lat4(lat),
                                         *couplings, int(n_md), float(dt), n_traj,
                                         int(bool(force_accept)), seed, offset, *ws, _dtype_code(phi), _stream(), *tail),
           symbol)
    out = dict(action=action, dh=dh, accept=accept, record=record, pi=pi_out)
    if measures:
        out['measure'] = measure
    return out


def phi4_hmc(phi, w0, w2, w4, n_md, dt, n_traj=1, record_every=None, pi_in=None, want_pi=False, force_accept=False,
             position=None, generator=None, measure=False, record=True, scheme=None):
    """nf_phi4_hmc: n_traj HMC trajectories of the C chains phi (C, *L), in place, in ONE launch.  (w0, w2, w4) are the
    kernel's coefficients (a user axis of extent 1 already folded into w2).  Returns a dict with action (C) float64 of
    the final states, dh (n_traj, C) float64, accept (n_traj, C) uint8, record (n_traj // record_every, C, *L) or None,
    pi (C, *L) or None.  The launch takes 2 n_traj Philox positions from torch's CUDA generator, or starts at
    `position` = (seed, offset) and leaves the generator alone.
    measure=True: nf_phi4_hmc_measure -- the dict gains measure (n_traj // record_every, C, n_out) float64, the rows that
    `lattice_measure` gives for the recorded states, taken inside the launch; with record=False no rows are allocated
    (record is None).
    scheme: None = leapfrog by nf_phi4_hmc[_measure]; an `HmcScheme`, a name or a pair of weights (`hmc_scheme`) runs
    nf_phi4_hmc[_measure]_scheme: n_md steps of the scheme's s stages, n_md * s force evaluations per trajectory."""
    return _phi4_hmc_call("phi4_hmc_measure" if measure else "phi4_hmc", phi, w0, w2, w4, n_md, dt, n_traj=n_traj,
                          record_every=record_every, pi_in=pi_in, want_pi=want_pi, force_accept=force_accept,
                          position=position, generator=generator, record=record, scheme=scheme)


# ========================================================================= Fourier-accelerated HMC (nf_hmc_fa.hip)
HMC_FA_MD_STEPS = 8           # NF_HMC_FA_MD_STEPS: the MD steps a filter counts as under the cap (measured: 6.2 to 6.6)


class HmcFaPlan(C.Structure):
    """nf_hmc_fa_plan (include/normflow_hip.h)."""
    _fields_ = [("sites_per_lane", C.c_int32), ("lanes", C.c_int32), ("phi_in_lds", C.c_int32), ("pi_in_lds", C.c_int32),
                ("lds_bytes", C.c_int64), ("matrix_bytes", C.c_int64), ("filters", C.c_int64)]


def hmc_fa_supported(lat, dtype):
    """True if nf_phi4_hmc_fa takes chains on the lattice `lat` (1 to 4 extents) in `dtype`: the launcher's own planner,
    pure host code; the reason of a refusal is in `last_error()`."""
    return _planner_supported("nf_phi4_hmc_fa_supported", lat, dtype)


def last_error():
    """nf_last_error_string: the message of the library's last refusal."""
    return load().nf_last_error_string().decode("utf-8", "replace")


def hmc_fa_plan(lat, dtype, n_md=1, stages=1):
    """What nf_phi4_hmc_fa will do on the lattice `lat` in `dtype` with n_md steps of a scheme of `stages` stages:
    dict(sites_per_lane, lanes, phi ('lds' or 'registers'), pi (likewise), lds_bytes, matrix_bytes, filters (per
    trajectory: n_md * stages + 3)).  Pure host code."""
    if not 1 <= len(lat) <= 4:
        raise NormflowHipError(f"hmc_fa_plan: lattices of 1 to 4 axes, got {tuple(lat)}")
    code = NF_F32 if dtype == torch.float32 else NF_F64 if dtype == torch.float64 else NF_F16
    out = HmcFaPlan()
    _check(load().nf_phi4_hmc_fa_plan(_lat4(lat), code, int(n_md), int(stages), C.byref(out)), "nf_phi4_hmc_fa_plan")
    where = lambda flag: 'lds' if flag else 'registers'
    return dict(sites_per_lane=out.sites_per_lane, lanes=out.lanes, phi=where(out.phi_in_lds), pi=where(out.pi_in_lds),
                lds_bytes=out.lds_bytes, matrix_bytes=out.matrix_bytes, filters=out.filters)


def hmc_fa_table(lat):
    """nf_phi4_hmc_fa_table: the list of per-axis tensors shat_mu(k) = 4 sin^2(pi k / L_mu), k = 0 .. L_mu - 1, float64 on
    the CPU, one per axis of `lat` -- the one table the kernel and the composed path share.  Pure host code."""
    lat = tuple(int(n) for n in lat)
    if not 1 <= len(lat) <= 4 or min(lat) < 1:
        raise NormflowHipError(f"hmc_fa_table: lattices of 1 to 4 axes of extent >= 1, got {lat}")
    pad = 4 - len(lat)
    buf = (C.c_double * (pad + sum(lat)))()
    _check(load().nf_phi4_hmc_fa_table(_lat4(lat), buf), "nf_phi4_hmc_fa_table")
    flat = torch.tensor(list(buf)[pad:], dtype=torch.float64)
    return list(torch.split(flat, list(lat)))


def hmc_fa_denominator(lat, w0, fa_mass_sq):
    """w0 sum_mu shat_mu(k_mu) + M^2 on the momentum lattice `lat`, float64 on the CPU, the axes summed left to right:
    a(k) is its reciprocal and a^(-1/2)(k) its square root (include/normflow_hip.h)."""
    table = hmc_fa_table(lat)
    d = len(lat)
    s = None
    for mu, t in enumerate(table):
        term = t.reshape((1,) * mu + (-1,) + (1,) * (d - 1 - mu))
        s = term if s is None else s + term
    return float(w0) * s.expand(tuple(lat)) + float(fa_mass_sq)


def hmc_fa_cost(evals):
    """The MD steps that a trajectory of `evals` = n_md * s force evaluations of nf_phi4_hmc_fa counts as under
    NF_HMC_MAX_WORK: its force evaluations and NF_HMC_FA_MD_STEPS per filter, evals + 3 filters."""
    return int(evals) + HMC_FA_MD_STEPS * (int(evals) + 3)


def phi4_hmc_fa(phi, w0, w2, w4, n_md, dt, fa_mass_sq, n_traj=1, record_every=None, pi_in=None, want_pi=False,
                force_accept=False, position=None, generator=None, record=True, scheme=None):
    """nf_phi4_hmc_fa: `phi4_hmc` with the kinetic term pi^T A pi / 2, a(k) = 1 / (w0 khat^2 + fa_mass_sq) (include/
    normflow_hip.h, "Fourier-accelerated hybrid Monte Carlo"); the same arguments and the same dict, `pi_in` and pi being
    pi (not the drawn eta).  scheme: None = leapfrog, else what `hmc_scheme` takes."""
    _require_device(phi, pi_in)
    if not phi.is_contiguous() or (pi_in is not None and (not pi_in.is_contiguous() or pi_in.dtype != phi.dtype
                                                            or pi_in.shape != phi.shape)):
        raise NormflowHipError("phi4_hmc_fa needs contiguous phi (C, *L) and pi_in of its shape and dtype")
    Cn, lat, dev = phi.shape[0], tuple(phi.shape[1:]), phi.device
    if not 1 <= len(lat) <= 4:
        raise NormflowHipError(f"phi4_hmc_fa: lattices of 1 to 4 axes, got {lat}")
    n_traj = int(n_traj)
    dh = torch.empty((max(n_traj, 0), Cn), dtype=torch.float64, device=dev)
    accept = torch.empty((max(n_traj, 0), Cn), dtype=torch.uint8, device=dev)
    action = torch.empty(Cn, dtype=torch.float64, device=dev)
    rec = None
    if record_every is not None and record:
        rec = torch.empty((n_traj // int(record_every), Cn) + lat, dtype=phi.dtype, device=dev)
    pi_out = torch.empty_like(phi) if want_pi else None
    if scheme is not None and scheme is not NULL_SCHEME:
        scheme = hmc_scheme(scheme)
    sc = None if scheme is None or scheme is NULL_SCHEME else C.byref(scheme)
    seed, offset = position if position is not None else _philox_positions(dev, 2 * max(n_traj, 1), generator)
    _check(load().nf_phi4_hmc_fa(_ptr(phi), _ptr(action), _ptr(pi_in), _ptr(pi_out), _ptr(dh), _ptr(accept), _ptr(rec),
                                 1 if record_every is None else int(record_every), Cn, _lat4(lat), float(w0), float(w2),
                                 float(w4), int(n_md), float(dt), n_traj, int(bool(force_accept)), seed, offset,
                                 _dtype_code(phi), _stream(), sc, float(fa_mass_sq)), "nf_phi4_hmc_fa")
    return dict(action=action, dh=dh, accept=accept, record=rec, pi=pi_out)


# ========================================================================= the same, chains in HBM (nf_hmc_tiled.hip)
HMC_TILED_MAX_LAUNCHES = 65536      # NF_HMC_TILED_MAX_LAUNCHES: the cap on (n_md * s + 2) * n_traj of one call


def hmc_tiled_budget(n_md):
    """The trajectories that one call of nf_phi4_hmc_tiled and its ladder form may hold; `n_md` counts the force
    evaluations of a trajectory: n_md * s for a scheme of s stages."""
    return HMC_TILED_MAX_LAUNCHES // (int(n_md) + 2)


def hmc_tiled_workspace(Cn, lat, dtype):
    """nf_phi4_hmc_tiled_workspace: the bytes of the workspace of a call on Cn chains on `lat` in `dtype`; pure host code."""
    code = NF_F32 if dtype == torch.float32 else NF_F64 if dtype == torch.float64 else NF_F16
    return int(load().nf_phi4_hmc_tiled_workspace(int(Cn), _lat4(tuple(lat)), code))


class HmcTiledPlan(C.Structure):
    """nf_hmc_tiled_plan (include/normflow_hip.h)."""
    _fields_ = [("tile", C.c_int32 * 4), ("ntiles", C.c_int32 * 4), ("tiles", C.c_int32), ("march_axis", C.c_int32),
                ("ring_depth", C.c_int32), ("lanes", C.c_int32), ("vec", C.c_int32), ("reserved", C.c_int32),
                ("lds_bytes", C.c_int64), ("lds_budget", C.c_int64)]


def hmc_tiled_supported(lat, dtype):
    """True if nf_phi4_hmc_tiled takes chains on the lattice `lat` (1 to 4 extents) in `dtype`: the launcher's own planner,
    pure host code."""
    return _planner_supported("nf_phi4_hmc_tiled_supported", lat, dtype)


def hmc_tiled_plan(lat, dtype):
    """What nf_phi4_hmc_tiled will do on the lattice `lat` in `dtype`, per axis of `lat`: dict(tile, ntiles, tiles (per
    chain), march_axis (None when no axis is marched), ring_depth, lanes, vec, lds_bytes, lds_budget).  Pure host code."""
    out = _planner_plan("hmc_tiled_plan", "nf_phi4_hmc_tiled_plan", lat, dtype, HmcTiledPlan())
    pad = 4 - len(lat)
    return dict(tile=tuple(out.tile)[pad:], ntiles=tuple(out.ntiles)[pad:], tiles=out.tiles,
                march_axis=None if out.march_axis < 0 else out.march_axis - pad, ring_depth=out.ring_depth, lanes=out.lanes,
                vec=out.vec, lds_bytes=out.lds_bytes, lds_budget=out.lds_budget)


def phi4_hmc_tiled(phi, w0, w2, w4, n_md, dt, n_traj=1, record_every=None, pi_in=None, want_pi=False, force_accept=False,
                   position=None, generator=None, workspace=None, scheme=None):
    """nf_phi4_hmc_tiled: `phi4_hmc` for chains that live in HBM, any lattice of 1 to 4 axes; the same arguments, the same
    Philox positions and the same dict.  (n_md * s + 2) * n_traj launches on the current stream (s = 1 without `scheme`).  The workspace comes from
    torch's caching allocator per call (stream-aware and graph-pool safe, like `_workspace`), or is `workspace`: a uint8
    tensor of at least nf_phi4_hmc_tiled_workspace bytes."""
    return _phi4_hmc_call("phi4_hmc_tiled", phi, w0, w2, w4, n_md, dt, n_traj=n_traj, record_every=record_every,
                          pi_in=pi_in, want_pi=want_pi, force_accept=force_accept, position=position, generator=generator,
                          workspace=workspace, scheme=scheme)


# ========================================================================= Fourier-accelerated HMC, chains in HBM (nf_hmc_fa_tiled.hip)
class HmcFaTiledPlan(C.Structure):
    """nf_hmc_fa_tiled_plan (include/normflow_hip.h)."""
    _fields_ = [("cut", C.c_int32), ("groups", C.c_int32), ("passes", C.c_int32), ("reserved", C.c_int32),
                ("first", C.c_int32 * 4), ("last", C.c_int32 * 4), ("run", C.c_int32 * 4), ("run_inner", C.c_int32 * 4),
                ("panels", C.c_int32 * 4), ("lanes", C.c_int32 * 4), ("panel_sites", C.c_int64 * 4),
                ("lds_bytes", C.c_int64 * 4), ("matrix_bytes", C.c_int64 * 4), ("filters", C.c_int64),
                ("launches", C.c_int64), ("step", HmcTiledPlan)]


def _fa_cut(what, lat, cut):
    """The library's `cut` for the lattice `lat` of 1 to 4 axes: -1 for None, else the mask of the boundaries between the
    axes of `lat` (bit mu: between axis mu and mu + 1) moved onto the four-extent lattice."""
    if cut is None:
        return -1
    cut = int(cut)
    if not 0 <= cut < 1 << (len(lat) - 1):
        raise NormflowHipError(f"{what}: cut must be None or a mask of the {len(lat) - 1} boundaries between the axes of "
                               f"{tuple(lat)}, got {cut}")
    return cut << (4 - len(lat))


def hmc_fa_tiled_supported(lat, dtype):
    """True if nf_phi4_hmc_fa_tiled takes chains on the lattice `lat` (1 to 4 extents) in `dtype`: the launcher's own
    planner, pure host code; the reason of a refusal is in `last_error()`."""
    return _planner_supported("nf_phi4_hmc_fa_tiled_supported", lat, dtype)


def hmc_fa_tiled_plan(lat, dtype, cut=None, n_md=1, stages=1):
    """What nf_phi4_hmc_fa_tiled will do on the lattice `lat` in `dtype` under `cut` (None: the planner's choice; else a
    mask, bit mu = a group boundary between the axes mu and mu + 1 of `lat`) with n_md steps of a scheme of `stages`
    stages: dict(cut (the mask used, in the axes of `lat`), groups (a list, the slowest first, of dict(axes, run,
    run_inner, panels (per chain), panel_sites, lanes, lds_bytes, matrix_bytes)), passes (per filter: 2 g - 1), filters
    and launches (per trajectory), step (`hmc_tiled_plan`'s dict of the step kernel)).  Pure host code."""
    if not 1 <= len(lat) <= 4:
        raise NormflowHipError(f"hmc_fa_tiled_plan: lattices of 1 to 4 axes, got {tuple(lat)}")
    code = NF_F32 if dtype == torch.float32 else NF_F64 if dtype == torch.float64 else NF_F16
    out = HmcFaTiledPlan()
    _check(load().nf_phi4_hmc_fa_tiled_plan(_lat4(lat), code, _fa_cut("hmc_fa_tiled_plan", lat, cut), int(n_md), int(stages),
                                            C.byref(out)), "nf_phi4_hmc_fa_tiled_plan")
    pad = 4 - len(lat)
    groups = [dict(axes=tuple(range(max(out.first[i] - pad, 0), out.last[i] - pad + 1)), run=out.run[i],
                   run_inner=out.run_inner[i], panels=out.panels[i], panel_sites=out.panel_sites[i], lanes=out.lanes[i],
                   lds_bytes=out.lds_bytes[i], matrix_bytes=out.matrix_bytes[i]) for i in range(out.groups)]
    st = out.step
    step = dict(tile=tuple(st.tile)[pad:], ntiles=tuple(st.ntiles)[pad:], tiles=st.tiles,
                march_axis=None if st.march_axis < 0 else st.march_axis - pad, ring_depth=st.ring_depth, lanes=st.lanes,
                vec=st.vec, lds_bytes=st.lds_bytes, lds_budget=st.lds_budget)
    return dict(cut=out.cut >> pad, groups=groups, passes=out.passes, filters=out.filters, launches=out.launches, step=step)


def hmc_fa_tiled_workspace(Cn, lat, dtype):
    """nf_phi4_hmc_fa_tiled_workspace: the bytes of the workspace of a call on Cn chains on `lat` in `dtype` (whatever the
    cut); pure host code."""
    code = NF_F32 if dtype == torch.float32 else NF_F64 if dtype == torch.float64 else NF_F16
    return int(load().nf_phi4_hmc_fa_tiled_workspace(int(Cn), _lat4(tuple(lat)), code))


def hmc_fa_tiled_budget(evals, passes=7):
    """The trajectories that one call of nf_phi4_hmc_fa_tiled may hold under NF_HMC_TILED_MAX_LAUNCHES: a trajectory of
    `evals` = n_md * s force evaluations is (evals + 3) * passes + evals + 4 launches, `passes` = 2 g - 1 of the plan (the
    default is the most there can be: four groups)."""
    evals, passes = int(evals), int(passes)
    return HMC_TILED_MAX_LAUNCHES // ((evals + 3) * passes + evals + 4)


def phi4_hmc_fa_tiled(phi, w0, w2, w4, n_md, dt, fa_mass_sq, n_traj=1, record_every=None, pi_in=None, want_pi=False,
                      force_accept=False, position=None, generator=None, workspace=None, scheme=None, cut=None):
    """nf_phi4_hmc_fa_tiled: `phi4_hmc_fa` for chains that live in HBM -- the same arguments, Philox positions and rule, the
    dict of `phi4_hmc_tiled`.  `workspace`: a uint8 tensor of at least nf_phi4_hmc_fa_tiled_workspace bytes, else one from
    torch's caching allocator per call.  `cut`: None (the planner's choice) or the mask of `hmc_fa_tiled_plan`; phi and pi
    do not depend on it."""
    what = "phi4_hmc_fa_tiled"
    _require_device(phi, pi_in)
    if not phi.is_contiguous() or (pi_in is not None and (not pi_in.is_contiguous() or pi_in.dtype != phi.dtype
                                                            or pi_in.shape != phi.shape)):
        raise NormflowHipError(f"{what} needs contiguous phi (C, *L) and pi_in of its shape and dtype")
    Cn, lat, dev = phi.shape[0], tuple(phi.shape[1:]), phi.device
    if not 1 <= len(lat) <= 4:
        raise NormflowHipError(f"{what}: lattices of 1 to 4 axes, got {lat}")
    n_traj = int(n_traj)
    dh = torch.empty((max(n_traj, 0), Cn), dtype=torch.float64, device=dev)
    accept = torch.empty((max(n_traj, 0), Cn), dtype=torch.uint8, device=dev)
    action = torch.empty(Cn, dtype=torch.float64, device=dev)
    rec = None
    if record_every is not None:
        rec = torch.empty((n_traj // int(record_every), Cn) + lat, dtype=phi.dtype, device=dev)
    pi_out = torch.empty_like(phi) if want_pi else None
    if workspace is None:
        workspace = torch.empty(max(hmc_fa_tiled_workspace(Cn, lat, phi.dtype), 256), dtype=torch.uint8, device=dev)
    if scheme is not None and scheme is not NULL_SCHEME:
        scheme = hmc_scheme(scheme)
    sc = None if scheme is None or scheme is NULL_SCHEME else C.byref(scheme)
    seed, offset = position if position is not None else _philox_positions(dev, 2 * max(n_traj, 1), generator)
    _check(load().nf_phi4_hmc_fa_tiled(_ptr(phi), _ptr(action), _ptr(pi_in), _ptr(pi_out), _ptr(dh), _ptr(accept), _ptr(rec),
                                       1 if record_every is None else int(record_every), Cn, _lat4(lat), float(w0),
                                       float(w2), float(w4), int(n_md), float(dt), n_traj, int(bool(force_accept)), seed,
                                       offset, _ptr(workspace), workspace.numel(), _dtype_code(phi), _stream(), sc,
                                       float(fa_mass_sq), _fa_cut(what, lat, cut)), "nf_phi4_hmc_fa_tiled")
    return dict(action=action, dh=dh, accept=accept, record=rec, pi=pi_out)


# ========================================================================= coupling ladders (nf_hmc.hip, nf_hmc_tiled.hip, nf_ladder.hip)
LADDER_MAX_K = 1024           # the rungs nf_phi4_ladder_exchange takes


def phi4_hmc_ladder(phi, coef, rung, n_md, dt, n_traj=1, record_every=None, pi_in=None, want_pi=False, force_accept=False,
                    position=None, generator=None, measure=False, record=True, scheme=None):
    """nf_phi4_hmc_ladder: `phi4_hmc` with per-chain couplings.  coef (K, 3) float64 holds (w0, w2, w4) per rung (a user
    axis of extent 1 folded into w2), rung (C) int32 the rung of every chain; chain c is in replica set c // K.  The dict
    is `phi4_hmc`'s, with dh, accept, record and measure RUNG-ORDERED (column (c // K) K + rung[c]) and action, pi per
    chain.  The same Philox positions."""
    return _phi4_hmc_call("phi4_hmc_ladder", phi, None, None, None, n_md, dt, n_traj=n_traj, record_every=record_every,
                          pi_in=pi_in, want_pi=want_pi, force_accept=force_accept, position=position, generator=generator,
                          record=record, ladder=(coef, rung), measure=measure, scheme=scheme)


def phi4_hmc_tiled_ladder(phi, coef, rung, n_md, dt, n_traj=1, record_every=None, pi_in=None, want_pi=False,
                          force_accept=False, position=None, generator=None, workspace=None, scheme=None):
    """nf_phi4_hmc_tiled_ladder: `phi4_hmc_tiled` with per-chain couplings, as `phi4_hmc_ladder`."""
    return _phi4_hmc_call("phi4_hmc_tiled_ladder", phi, None, None, None, n_md, dt, n_traj=n_traj,
                          record_every=record_every, pi_in=pi_in, want_pi=want_pi, force_accept=force_accept,
                          position=position, generator=generator, workspace=workspace, ladder=(coef, rung), scheme=scheme)


def ladder_exchange(rows, coef, rung, parity, action=None, position=None, generator=None):
    """nf_phi4_ladder_exchange: one replica-exchange sweep of parity 0 / 1.  rows (C, n >= 7) float64 are the chains'
    `lattice_measure` rows (indexed by chain; a view with a row stride is taken as it is), coef (K, 3) float64, rung (C)
    int32 is updated in place, and so is action (C) float64 when given.  Returns swapped (C // K, K - 1) uint8.  One Philox
    position from torch's CUDA generator, or `position` = (seed, offset)."""
    what = "ladder_exchange"
    _require_device(rows, coef, rung, action)
    if not isinstance(rung, torch.Tensor) or rung.ndim != 1:
        raise NormflowHipError(f"{what}: rung must be a (C,) int32 tensor")
    Cn, dev = rung.shape[0], rung.device
    K, (pc, _, pr) = _ladder_tensors(what, coef, rung, Cn, dev)
    if K > LADDER_MAX_K:
        raise NormflowHipError(f"{what}: K = {K} rungs exceed the {LADDER_MAX_K} of one workgroup's map")
    if Cn < 1:
        raise NormflowHipError(f"{what}: no chains")
    if (rows.device != dev or rows.dtype != torch.float64 or rows.ndim != 2 or rows.shape[0] != Cn or rows.shape[1] < 7
            or rows.stride(1) != 1 or rows.stride(0) < 7):
        raise NormflowHipError(f"{what}: rows must be ({Cn}, n >= 7) float64 on {dev} with unit stride along a row, got "
                               f"{tuple(rows.shape)} {rows.dtype} strides {rows.stride()}")
    if action is not None and (action.device != dev or action.dtype != torch.float64 or tuple(action.shape) != (Cn,)
                               or not action.is_contiguous()):
        raise NormflowHipError(f"{what}: action must be a contiguous ({Cn},) float64 tensor on {dev}")
    if int(parity) not in (0, 1):
        raise NormflowHipError(f"{what}: parity must be 0 or 1, got {parity}")
    swapped = torch.zeros((Cn // K, K - 1), dtype=torch.uint8, device=dev)
    seed, offset = position if position is not None else _philox_position(dev, generator)
    _check(load().nf_phi4_ladder_exchange(_ptr(rows), rows.stride(0), pc, K, pr, _ptr(action), _ptr(swapped), Cn,
                                          int(parity), seed, offset, _stream()), "nf_phi4_ladder_exchange")
    return swapped


# ========================================================================= cluster sweeps of phi^4 chains (nf_cluster.hip)
class ClusterPlan(C.Structure):
    """nf_cluster_plan (include/normflow_hip.h)."""
    _fields_ = [("sites_per_lane", C.c_int32), ("lanes", C.c_int32), ("lds_bytes", C.c_int64)]


def cluster_supported(lat, dtype):
    """True if nf_phi4_cluster takes chains on the lattice `lat` (1 to 4 extents) in `dtype`: the launcher's own planner,
    pure host code."""
    return _planner_supported("nf_phi4_cluster_supported", lat, dtype)


def cluster_plan(lat, dtype):
    """What nf_phi4_cluster will do on the lattice `lat` in `dtype`: dict(sites_per_lane, lanes (of a chain's workgroup),
    lds_bytes).  Pure host code."""
    out = _planner_plan("cluster_plan", "nf_phi4_cluster_plan", lat, dtype, ClusterPlan())
    return dict(sites_per_lane=out.sites_per_lane, lanes=out.lanes, lds_bytes=out.lds_bytes)


def phi4_cluster(phi, w0, position=None, want_labels=False, generator=None):
    """nf_phi4_cluster: one Swendsen-Wang sweep of the signs of the C chains phi (C, *L), in place, in ONE launch.  w0 is
    the action's hopping coefficient.  Returns dict(stats (C, 4) int32 = clusters, sites flipped, size of the largest
    cluster, rounds; labels (C, *L) int32 or None).  The sweep takes 2 Philox positions from torch's CUDA generator, or
    starts at `position` = (seed, offset) and leaves the generator alone."""
    _require_device(phi)
    if not phi.is_contiguous():
        raise NormflowHipError("phi4_cluster needs contiguous phi (C, *L)")
    Cn, lat, dev = phi.shape[0], tuple(phi.shape[1:]), phi.device
    if not 1 <= len(lat) <= 4:
        raise NormflowHipError(f"phi4_cluster: lattices of 1 to 4 axes, got {lat}")
    stats = torch.empty((Cn, 4), dtype=torch.int32, device=dev)
    labels = torch.empty((Cn,) + lat, dtype=torch.int32, device=dev) if want_labels else None
    seed, offset = position if position is not None else _philox_positions(dev, 2, generator)
    _check(load().nf_phi4_cluster(_ptr(phi), _ptr(stats), _ptr(labels), Cn, _lat4(lat), float(w0), seed, offset,
                                  _dtype_code(phi), _stream()), "nf_phi4_cluster")
    return dict(stats=stats, labels=labels)


def phi4_cluster_draws(Cn, lattice, device, position=None, generator=None):
    """nf_phi4_cluster_draws: (u (C, V, 4) float64, flip (C, V) uint8), the bond uniforms and the flip bits of the sweep
    that `phi4_cluster` makes of C chains on `lattice` from the same position; 2 positions, taken as `phi4_cluster`
    takes them."""
    lat, device = tuple(lattice), torch.device(device)
    if device.type != 'cuda':
        raise NormflowHipError(f"phi4_cluster_draws writes on an MI355X (torch device 'cuda'), got {device}")
    if not 1 <= len(lat) <= 4:
        raise NormflowHipError(f"phi4_cluster_draws: lattices of 1 to 4 axes, got {lat}")
    Cn, V = int(Cn), _sites(lat)
    u = torch.empty((max(Cn, 0), V, 4), dtype=torch.float64, device=device)
    flip = torch.empty((max(Cn, 0), V), dtype=torch.uint8, device=device)
    seed, offset = position if position is not None else _philox_positions(device, 2, generator)
    _check(load().nf_phi4_cluster_draws(_ptr(u), _ptr(flip), Cn, _lat4(lat), seed, offset, _stream()),
           "nf_phi4_cluster_draws")
    return u, flip


# ========================================================================= the same, chains in HBM (nf_cluster_tiled.hip)
class ClusterTiledPlan(C.Structure):
    """nf_cluster_tiled_plan (include/normflow_hip.h)."""
    _fields_ = [("tiles", C.c_int64), ("tile_sites", C.c_int32), ("lanes", C.c_int32), ("lds_bytes", C.c_int64)]


def _tile_sites(tile_sites):
    """None / 0: the library's default tile."""
    t = 0 if tile_sites is None else int(tile_sites)
    if t < 0:
        raise NormflowHipError(f"tile_sites must be None or >= 0, got {tile_sites}")
    return t


def cluster_tiled_supported(lat, dtype, tile_sites=0):
    """True if nf_phi4_cluster_tiled takes chains on the lattice `lat` (1 to 4 extents) in `dtype` with tiles of
    `tile_sites` sites (0: the default): the launcher's own planner, pure host code."""
    if dtype not in (torch.float32, torch.float64) or not 1 <= len(lat) <= 4:
        return False
    return bool(load().nf_phi4_cluster_tiled_supported(_lat4(lat), NF_F32 if dtype == torch.float32 else NF_F64,
                                                       _tile_sites(tile_sites)))


def cluster_tiled_plan(lat, dtype, tile_sites=0):
    """What nf_phi4_cluster_tiled will do on the lattice `lat` in `dtype` with tiles of `tile_sites` sites (0: the
    default): dict(tiles (per chain), tile_sites (in force), lanes (of a tile's workgroup), lds_bytes, workspace_bytes (ONE
    chain's share of nf_phi4_cluster_tiled_workspace, without its 8 bytes of flags)).  Pure host code."""
    if not 1 <= len(lat) <= 4:
        raise NormflowHipError(f"cluster_tiled_plan: lattices of 1 to 4 axes, got {tuple(lat)}")
    code = NF_F32 if dtype == torch.float32 else NF_F64 if dtype == torch.float64 else NF_F16
    out = ClusterTiledPlan()
    _check(load().nf_phi4_cluster_tiled_plan(_lat4(lat), code, _tile_sites(tile_sites), C.byref(out)),
           "nf_phi4_cluster_tiled_plan")
    return dict(tiles=out.tiles, tile_sites=out.tile_sites, lanes=out.lanes, lds_bytes=out.lds_bytes,
                workspace_bytes=cluster_tiled_workspace(1, lat, tile_sites) - 8)


def cluster_tiled_workspace(Cn, lat, tile_sites=0):
    """nf_phi4_cluster_tiled_workspace: the bytes of the workspace of a sweep of Cn chains on `lat`; pure host code."""
    return int(load().nf_phi4_cluster_tiled_workspace(int(Cn), _lat4(tuple(lat)), _tile_sites(tile_sites)))


def phi4_cluster_tiled(phi, w0, position=None, want_labels=False, tile_sites=0, workspace=None, generator=None):
    """nf_phi4_cluster_tiled: `phi4_cluster` for chains that live in HBM, any lattice of 1 to 4 axes; the same Philox
    positions and the same dict, with stats[:, 3] = the tiles of a chain.  Four launches and one memset on the
    current stream.  `tile_sites`: the sites of a tile (0: the default).  The workspace comes from torch's caching
    allocator per call (stream-aware and graph-pool safe, like `_workspace`), or is `workspace`: a uint8 tensor of at least
    nf_phi4_cluster_tiled_workspace bytes."""
    _require_device(phi)
    if not phi.is_contiguous():
        raise NormflowHipError("phi4_cluster_tiled needs contiguous phi (C, *L)")
    Cn, lat, dev = phi.shape[0], tuple(phi.shape[1:]), phi.device
    if not 1 <= len(lat) <= 4:
        raise NormflowHipError(f"phi4_cluster_tiled: lattices of 1 to 4 axes, got {lat}")
    ts = _tile_sites(tile_sites)
    if workspace is None:
        need = load().nf_phi4_cluster_tiled_workspace(Cn, _lat4(lat), ts)
        workspace = torch.empty(max(int(need), 256), dtype=torch.uint8, device=dev)
    stats = torch.empty((Cn, 4), dtype=torch.int32, device=dev)
    labels = torch.empty((Cn,) + lat, dtype=torch.int32, device=dev) if want_labels else None
    seed, offset = position if position is not None else _philox_positions(dev, 2, generator)
    _check(load().nf_phi4_cluster_tiled(_ptr(phi), _ptr(stats), _ptr(labels), Cn, _lat4(lat), float(w0), seed, offset,
                                        _dtype_code(phi), ts, _ptr(workspace), workspace.numel(), _stream()),
           "nf_phi4_cluster_tiled")
    return dict(stats=stats, labels=labels)


# ========================================================================= the two sweeps on a coupling ladder
def _phi4_cluster_ladder_call(what, phi, coef, rung, position, want_labels, generator, tiled=None):
    """The body of `phi4_cluster_ladder` and `phi4_cluster_tiled_ladder` (`what`; the entry point is nf_<what>): the
    checks, the outputs, the 2 Philox positions, the call and the dict.  `tiled` = (tile_sites, workspace) or None."""
    _require_device(phi)
    if not phi.is_contiguous():
        raise NormflowHipError(f"{what} needs contiguous phi (C, *L)")
    Cn, lat, dev = phi.shape[0], tuple(phi.shape[1:]), phi.device
    if not 1 <= len(lat) <= 4:
        raise NormflowHipError(f"{what}: lattices of 1 to 4 axes, got {lat}")
    ladder = _ladder_tensors(what, coef, rung, Cn, dev)[1]
    tail = ()
    if tiled is not None:
        ts, workspace = _tile_sites(tiled[0]), tiled[1]
        if workspace is None:
            need = load().nf_phi4_cluster_tiled_workspace(Cn, _lat4(lat), ts)
            workspace = torch.empty(max(int(need), 256), dtype=torch.uint8, device=dev)
        tail = (ts, _ptr(workspace), workspace.numel())
    stats = torch.empty((Cn, 4), dtype=torch.int32, device=dev)
    labels = torch.empty((Cn,) + lat, dtype=torch.int32, device=dev) if want_labels else None
    seed, offset = position if position is not None else _philox_positions(dev, 2, generator)
    _check(getattr(load(), "nf_" + what)(_ptr(phi), _ptr(stats), _ptr(labels), Cn, _lat4(lat), *ladder, seed, offset,
                                         _dtype_code(phi), *tail, _stream()), "nf_" + what)
    return dict(stats=stats, labels=labels)


def phi4_cluster_ladder(phi, coef, rung, position=None, want_labels=False, generator=None):
    """nf_phi4_cluster_ladder: `phi4_cluster` with a hopping coefficient per chain.  coef (K, 3) float64 holds (w0, w2, w4)
    per rung, of which the sweep reads w0; rung (C) int32 is the rung of every chain, C a multiple of K.  A chain on rung k
    gets `phi4_cluster`'s bits at w0_k.  The same dict and the same 2 Philox positions; phi and labels stay at the chain's
    index, stats (C, 4) is RUNG-ORDERED: the row of chain c is (c // K) K + rung[c]."""
    return _phi4_cluster_ladder_call("phi4_cluster_ladder", phi, coef, rung, position, want_labels, generator)


def phi4_cluster_tiled_ladder(phi, coef, rung, position=None, want_labels=False, tile_sites=0, workspace=None,
                              generator=None):
    """nf_phi4_cluster_tiled_ladder: `phi4_cluster_tiled` with a hopping coefficient per chain, as `phi4_cluster_ladder`;
    `tile_sites` and `workspace` as `phi4_cluster_tiled` takes them."""
    return _phi4_cluster_ladder_call("phi4_cluster_tiled_ladder", phi, coef, rung, position, want_labels, generator,
                                     tiled=(tile_sites, workspace))


# ========================================================================= cluster-improved estimators (nf_cluster_moments.hip)
class MomentsPlan(C.Structure):
    """nf_moments_plan (include/normflow_hip.h)."""
    _fields_ = [("sites_per_lane", C.c_int32), ("lanes", C.c_int32), ("quantities", C.c_int32), ("passes", C.c_int32),
                ("per_pass", C.c_int32), ("lds_bytes", C.c_int64)]


def cluster_moments_supported(lat, dtype):
    """True if nf_cluster_moments takes chains on the lattice `lat` (1 to 4 extents) in `dtype`: the launcher's own
    planner, pure host code."""
    return _planner_supported("nf_cluster_moments_supported", lat, dtype)


def cluster_moments_plan(lat, dtype):
    """What nf_cluster_moments will do on the lattice `lat` in `dtype`: dict(sites_per_lane, lanes (of a chain's
    workgroup), quantities (1 + 2 x the axes of extent > 1), passes, per_pass (quantities per pass), lds_bytes).  Pure
    host code."""
    out = _planner_plan("cluster_moments_plan", "nf_cluster_moments_plan", lat, dtype, MomentsPlan())
    return {name: getattr(out, name) for name, _ in MomentsPlan._fields_}


def cluster_moments_limit(V):
    """The range of the improved estimators' fixed point: a site is in range iff |phi| < 2^min(16, 30 - ceil(log2 V))."""
    return 2.0 ** min(16, 30 - (int(V) - 1).bit_length())


_TWIDDLES = {}


def twiddle_table(lat, device=None):
    """The table tw (sum of the four padded extents, 2) float64 of nf_cluster_moments for the lattice `lat` (1 to 4 axes):
    rows off_mu + t = (cos, sin)(2 pi t / L_mu), computed once on the host (math.cos / math.sin of the double
    2 pi t / L_mu) and cached per (lattice, device), so that every path uses the same numbers bit for bit."""
    lat = tuple(int(n) for n in lat)
    key = (lat, None if device is None else str(torch.device(device)))
    if key not in _TWIDDLES:
        if device is not None:
            _TWIDDLES[key] = twiddle_table(lat).to(device)
        else:
            rows = [(math.cos(2.0 * math.pi * t / n), math.sin(2.0 * math.pi * t / n))
                    for n in (1,) * (4 - len(lat)) + lat for t in range(n)]
            _TWIDDLES[key] = torch.tensor(rows, dtype=torch.float64, device='cpu')
    return _TWIDDLES[key]


def cluster_moments(phi, labels, want_moments=False):
    """nf_cluster_moments: the sign-averaged sums of the C chains phi (C, *L) under the cluster decomposition labels
    (C, *L) int32 (any keys in 0 .. V - 1; the sweeps' labels are), in ONE launch with no slab loop (C <= 65535, as the
    sweeps).  Returns dict(out (C, 2 + d) float64 = sum_C M_C^2, sum_C M_C^4 and per axis of `L` sum_C |M~_C(p_min)|^2, with
    M_C = the cluster's sum of phi; status (C) int32, 1 = refused (a site out of range or a label outside 0 .. V - 1: the
    out row is NaN, the moments row 0); moments (C, *L) int64 = the clusters' fixed-point sums A_C = M_C 2^32 at slot =
    label, or None).  The rule is stated in include/normflow_hip.h.
    Graph capture: the launch itself neither allocates nor synchronises, but the FIRST call for a (lattice, device) copies
    the twiddle table to the device.  Call `twiddle_table(lat, device)` (or this function once) before capturing."""
    _require_device(phi, labels)
    lat = tuple(phi.shape[1:])
    if not phi.is_contiguous() or not 1 <= len(lat) <= 4:
        raise NormflowHipError(f"cluster_moments needs contiguous phi (C, *L) with 1 to 4 lattice axes, got {tuple(phi.shape)}")
    if labels.shape != phi.shape or labels.dtype != torch.int32 or not labels.is_contiguous() or labels.device != phi.device:
        raise NormflowHipError(f"cluster_moments: labels must be a contiguous int32 tensor {tuple(phi.shape)} on {phi.device}, "
                               f"got {tuple(labels.shape)} {labels.dtype} on {labels.device}")
    Cn, dev = phi.shape[0], phi.device
    out = torch.empty((Cn, 6), dtype=torch.float64, device=dev)
    status = torch.empty((Cn,), dtype=torch.int32, device=dev)
    moments = torch.empty((Cn,) + lat, dtype=torch.int64, device=dev) if want_moments else None
    tw = twiddle_table(lat, dev)
    _check(load().nf_cluster_moments(_ptr(phi), _ptr(labels), _ptr(out), _ptr(status), _ptr(moments), Cn, _lat4(lat),
                                     _ptr(tw), _dtype_code(phi), _stream()), "nf_cluster_moments")
    pad = 4 - len(lat)
    return dict(out=torch.cat([out[:, :2], out[:, 2 + pad:]], dim=1), status=status, moments=moments)


# ========================================================================= cluster spectrum (nf_cluster_spectrum.hip)
class SpectrumPlan(C.Structure):
    """nf_spectrum_plan (include/normflow_hip.h)."""
    _fields_ = [("sites_per_lane", C.c_int32), ("lanes", C.c_int32), ("kmax", C.c_int32 * 4), ("columns", C.c_int32),
                ("quantities", C.c_int32), ("passes", C.c_int32), ("per_pass", C.c_int32), ("lds_bytes", C.c_int64)]


def spectrum_kmax(momenta):
    """`momenta` ('all' or an int >= 1) as the library's kmax: 0 means all."""
    if isinstance(momenta, str):
        if momenta != 'all':
            raise NormflowHipError(f"momenta must be 'all' or an int >= 1, got {momenta!r}")
        return 0
    if isinstance(momenta, bool) or not isinstance(momenta, int) or momenta < 1:
        raise NormflowHipError(f"momenta must be 'all' or an int >= 1, got {momenta!r}")
    return int(momenta)


def spectrum_momenta(lat, momenta='all'):
    """K_mu of the axes of `lat` under `momenta`: 0 for an axis of extent 1, else floor(L / 2) or min(momenta, floor(L / 2))."""
    kmax = spectrum_kmax(momenta)
    return tuple(0 if n == 1 else (n // 2 if kmax == 0 else min(kmax, n // 2)) for n in lat)


def cluster_spectrum_supported(lat, dtype, momenta='all'):
    """True if nf_cluster_spectrum takes chains on the lattice `lat` (1 to 4 extents) in `dtype`: the launcher's own
    planner, pure host code."""
    if dtype not in (torch.float32, torch.float64) or not 1 <= len(lat) <= 4:
        return False
    return bool(load().nf_cluster_spectrum_supported(_lat4(lat), _dtype_code_of(dtype), spectrum_kmax(momenta)))


def cluster_spectrum_plan(lat, dtype, momenta='all'):
    """What nf_cluster_spectrum will do on the lattice `lat` in `dtype`: dict(sites_per_lane, lanes, kmax (K_mu of the
    four padded axes), columns, quantities, passes, per_pass, lds_bytes).  Pure host code."""
    if not 1 <= len(lat) <= 4:
        raise NormflowHipError(f"cluster_spectrum_plan: lattices of 1 to 4 axes, got {tuple(lat)}")
    out = SpectrumPlan()
    _check(load().nf_cluster_spectrum_plan(_lat4(lat), _dtype_code_of(dtype), spectrum_kmax(momenta), C.byref(out)),
           "nf_cluster_spectrum_plan")
    d = {name: getattr(out, name) for name, _ in SpectrumPlan._fields_}
    d['kmax'] = tuple(out.kmax)
    return d


def cluster_spectrum(phi, labels, momenta='all'):
    """nf_cluster_spectrum: `cluster_moments` at every on-axis momentum k = 1 .. K_mu, in ONE launch (C <= 65535).  Returns
    dict(out (C, 2 + sum K_mu) float64 = sum_C M_C^2, sum_C M_C^4, then per axis of `L` and per k ascending
    sum_C |M~_C(2 pi k / L_mu)|^2 (no column for an axis of extent 1); status (C) int32, 1 = refused (the out row is NaN);
    momenta = (K_mu of the axes of `L`)).  `momenta` is 'all' (K_mu = L_mu // 2) or an int >= 1 (K_mu = min of the two).
    The rule is stated in include/normflow_hip.h, "cluster spectrum".  Graph capture: as `cluster_moments`, call
    `twiddle_table(lat, device)` first."""
    _require_device(phi, labels)
    lat = tuple(phi.shape[1:])
    if not phi.is_contiguous() or not 1 <= len(lat) <= 4:
        raise NormflowHipError(f"cluster_spectrum needs contiguous phi (C, *L) with 1 to 4 lattice axes, got {tuple(phi.shape)}")
    if labels.shape != phi.shape or labels.dtype != torch.int32 or not labels.is_contiguous() or labels.device != phi.device:
        raise NormflowHipError(f"cluster_spectrum: labels must be a contiguous int32 tensor {tuple(phi.shape)} on {phi.device}, "
                               f"got {tuple(labels.shape)} {labels.dtype} on {labels.device}")
    kmax = spectrum_kmax(momenta)
    K = spectrum_momenta(lat, momenta)
    Cn, dev = phi.shape[0], phi.device
    out = torch.empty((Cn, 2 + sum(K)), dtype=torch.float64, device=dev)
    status = torch.empty((Cn,), dtype=torch.int32, device=dev)
    tw = twiddle_table(lat, dev)
    _check(load().nf_cluster_spectrum(_ptr(phi), _ptr(labels), _ptr(out), _ptr(status), Cn, _lat4(lat), kmax, _ptr(tw),
                                      _dtype_code(phi), _stream()), "nf_cluster_spectrum")
    return dict(out=out, status=status, momenta=K)


# ========================================================================= cluster modes (nf_cluster_modes.hip)
MODES_MAX = 512                         # momenta of one call
MODES_MAX_N = 65536                     # the lcm of the extents


class ModesPlan(C.Structure):
    """nf_modes_plan (include/normflow_hip.h)."""
    _fields_ = [("sites_per_lane", C.c_int32), ("lanes", C.c_int32), ("N", C.c_int32), ("columns", C.c_int32),
                ("quantities", C.c_int32), ("per_pass", C.c_int32), ("passes", C.c_int32), ("lds_bytes", C.c_int64)]


def modes_list(lat, modes):
    """`modes`, a sequence of P >= 1 integer vectors with one component per axis of `lat`, as a tuple of tuples of ints;
    anything else is a NormflowHipError.  The components are left as given (`modes_reduced` reduces them)."""
    lat = tuple(int(n) for n in lat)
    try:
        out = tuple(tuple(n for n in m) for m in modes)
    except TypeError:
        raise NormflowHipError(f"modes must be a sequence of integer vectors, one component per axis of {lat}, got {modes!r}")
    if not out:
        raise NormflowHipError(f"modes must hold at least one momentum, got {modes!r}")
    for m in out:
        if len(m) != len(lat) or any(isinstance(n, bool) or not isinstance(n, int) for n in m):
            raise NormflowHipError(f"modes: every momentum has {len(lat)} integer components on the lattice {lat}, got {m!r}")
        if any(abs(n) >= 2 ** 31 for n in m):
            raise NormflowHipError(f"modes: components are 32-bit integers, got {m!r}")
    return out


def modes_reduced(lat, modes):
    """The momenta with every component reduced to 0 .. L_mu - 1 (the rule's own reduction): a tuple of tuples."""
    lat = tuple(int(n) for n in lat)
    return tuple(tuple(n % L for n, L in zip(m, lat)) for m in modes_list(lat, modes))


def modes_lcm(lat):
    """N of the rule: the lcm of the extents (1 where every extent is 1)."""
    return math.lcm(*[int(n) for n in lat])


def _modes_array(lat, modes):
    """(the (P, 4) int32 array of the padded momenta, P) for the library."""
    lst = modes_list(lat, modes)
    flat = [n for m in lst for n in (0,) * (4 - len(lat)) + m]
    return _c_ints(flat), len(lst)


def cluster_modes_supported(lat, dtype, modes):
    """True if nf_cluster_modes takes chains on the lattice `lat` (1 to 4 extents) in `dtype` at the momenta `modes`: the
    launcher's own planner, pure host code (the reason for a False is `last_error()`)."""
    if dtype not in (torch.float32, torch.float64) or not 1 <= len(lat) <= 4:
        return False
    arr, P = _modes_array(lat, modes)
    return bool(load().nf_cluster_modes_supported(_lat4(lat), _dtype_code_of(dtype), arr, P))


def cluster_modes_plan(lat, dtype, modes):
    """What nf_cluster_modes will do on the lattice `lat` in `dtype` at `modes`: dict(sites_per_lane, lanes, N (the lcm of
    the extents), columns (2 + P), quantities, per_pass, passes, lds_bytes).  Pure host code."""
    if not 1 <= len(lat) <= 4:
        raise NormflowHipError(f"cluster_modes_plan: lattices of 1 to 4 axes, got {tuple(lat)}")
    arr, P = _modes_array(lat, modes)
    out = ModesPlan()
    _check(load().nf_cluster_modes_plan(_lat4(lat), _dtype_code_of(dtype), arr, P, C.byref(out)), "nf_cluster_modes_plan")
    return {name: getattr(out, name) for name, _ in ModesPlan._fields_}


def cluster_modes_describe(lat, modes):
    """nf_cluster_modes_describe: (desc (Q, 8) int32 on the host, N) of the momenta `modes` on `lat`; the rows are laid out
    in normflow__amd/csrc/nf_cluster_modes_core.h.  Pure host code; the table is checked by nf_cluster_modes_check."""
    if not 1 <= len(lat) <= 4:
        raise NormflowHipError(f"cluster_modes_describe: lattices of 1 to 4 axes, got {tuple(lat)}")
    arr, P = _modes_array(lat, modes)
    desc = torch.zeros((1 + 2 * max(P, 1), 8), dtype=torch.int32, device='cpu')       # host code fills it: never the default device
    Q, N = C.c_int32(0), C.c_int32(0)
    _check(load().nf_cluster_modes_describe(_lat4(lat), arr, P, _ptr(desc), C.byref(Q), C.byref(N)),
           "nf_cluster_modes_describe")
    desc = desc[:Q.value].clone()
    _check(load().nf_cluster_modes_check(_lat4(lat), _ptr(desc), Q.value, N.value), "nf_cluster_modes_check")
    return desc, N.value


_MODE_TWIDDLES = {}
_MODE_DESCS = {}
_MODE_CALLS = {}                        # (lattice, the list as given, device) -> (reduced, desc, N, twN) of `cluster_modes`


def mode_twiddle_table(lat, device=None):
    """The table twN (N, 2) float64 of nf_cluster_modes for the lattice `lat`, N = the lcm of its extents: row j =
    (cos, sin)(2 pi j / N), computed once on the host (math.cos / math.sin of the double 2 pi j / N, `twiddle_table`'s
    formula for an axis of extent N) and cached per (N, device), so that every path uses the same numbers bit for bit."""
    N = modes_lcm(lat)
    if not 2 <= N <= MODES_MAX_N:
        raise NormflowHipError(f"mode_twiddle_table: N, the lcm of the extents of {tuple(lat)}, is {N}: it must be in 2 .. {MODES_MAX_N}")
    key = (N, None if device is None else str(torch.device(device)))
    if key not in _MODE_TWIDDLES:
        if device is not None:
            _MODE_TWIDDLES[key] = mode_twiddle_table(lat).to(device)
        else:
            rows = [(math.cos(2.0 * math.pi * j / N), math.sin(2.0 * math.pi * j / N)) for j in range(N)]
            _MODE_TWIDDLES[key] = torch.tensor(rows, dtype=torch.float64, device='cpu')
    return _MODE_TWIDDLES[key]


def mode_descriptor(lat, modes, device=None):
    """(desc (Q, 8) int32, N) of `cluster_modes_describe`, cached per (lattice, reduced momenta, device) like
    `twiddle_table`; with a device the table lies there."""
    lat = tuple(int(n) for n in lat)
    key = (lat, modes_reduced(lat, modes), None if device is None else str(torch.device(device)))
    if key not in _MODE_DESCS:
        if device is not None:
            desc, N = mode_descriptor(lat, modes)
            _MODE_DESCS[key] = (desc.to(device), N)
        else:
            _MODE_DESCS[key] = cluster_modes_describe(lat, modes)
    return _MODE_DESCS[key]


def cluster_modes(phi, labels, modes):
    """nf_cluster_modes: `cluster_moments` at the momentum vectors `modes` -- a sequence of P <= 512 integer vectors with one
    component per lattice axis, on or off the axes, negative components allowed -- in ONE launch (C <= 65535).  Returns
    dict(out (C, 2 + P) float64 = sum_C M_C^2, sum_C M_C^4, then per momentum in list order sum_C |M~_C(p)|^2 with
    p_mu = 2 pi n_mu / L_mu; status (C) int32, 1 = refused (the out row is NaN); modes = the momenta reduced to
    0 .. L_mu - 1).  The rule is stated in include/normflow_hip.h, "cluster modes".
    Graph capture: the launch neither allocates nor synchronises, but the FIRST call for a (lattice, modes, device) copies
    the twiddle table and the quantity table to the device.  Call this function once (or `mode_twiddle_table(lat,
    device)` and `mode_descriptor(lat, modes, device)`) before capturing."""
    _require_device(phi, labels)
    lat = tuple(phi.shape[1:])
    if not phi.is_contiguous() or not 1 <= len(lat) <= 4:
        raise NormflowHipError(f"cluster_modes needs contiguous phi (C, *L) with 1 to 4 lattice axes, got {tuple(phi.shape)}")
    if labels.shape != phi.shape or labels.dtype != torch.int32 or not labels.is_contiguous() or labels.device != phi.device:
        raise NormflowHipError(f"cluster_modes: labels must be a contiguous int32 tensor {tuple(phi.shape)} on {phi.device}, "
                               f"got {tuple(labels.shape)} {labels.dtype} on {labels.device}")
    Cn, dev = phi.shape[0], phi.device
    # a list seen before costs one dictionary look-up: its validation, reduction and table take tens of microseconds of
    # Python, more than the kernel's run on a small lattice
    try:
        key = (lat, modes if isinstance(modes, tuple) else tuple(modes), dev)
        hit = _MODE_CALLS.get(key)
    except TypeError:                                         # momenta given as lists: not hashable, the slow way
        key = hit = None
    if hit is None:
        hit = (modes_reduced(lat, modes),) + mode_descriptor(lat, modes, dev) + (mode_twiddle_table(lat, dev),)
        if key is not None:
            _MODE_CALLS[key] = hit
    reduced, desc, N, tw = hit
    out = torch.empty((Cn, 2 + len(reduced)), dtype=torch.float64, device=dev)
    status = torch.empty((Cn,), dtype=torch.int32, device=dev)
    _check(load().nf_cluster_modes(_ptr(phi), _ptr(labels), _ptr(out), _ptr(status), Cn, _lat4(lat), _ptr(desc),
                                   desc.shape[0], _ptr(tw), N, _dtype_code(phi), _stream()), "nf_cluster_modes")
    return dict(out=out, status=status, modes=reduced)


# ========================================================================= the same, slots in HBM (nf_cluster_moments_tiled.hip)
class MomentsTiledPlan(C.Structure):
    """nf_moments_tiled_plan (include/normflow_hip.h)."""
    _fields_ = [("blocks", C.c_int64), ("block_sites", C.c_int32), ("quantities", C.c_int32), ("per_pass", C.c_int32),
                ("passes", C.c_int32), ("table_entries", C.c_int32), ("launches", C.c_int32), ("lds_bytes", C.c_int64)]


def _block_sites(block_sites):
    """None / 0: the library's default block."""
    b = 0 if block_sites is None else int(block_sites)
    if b < 0:
        raise NormflowHipError(f"block_sites must be None or >= 0, got {block_sites}")
    return b


def _dtype_code_of(dtype):
    return NF_F32 if dtype == torch.float32 else NF_F64 if dtype == torch.float64 else NF_F16


def cluster_moments_tiled_supported(lat, dtype, block_sites=0):
    """True if nf_cluster_moments_tiled takes chains on the lattice `lat` (1 to 4 extents) in `dtype` with blocks of
    `block_sites` sites (0: the default): the launcher's own planner, pure host code."""
    if dtype not in (torch.float32, torch.float64) or not 1 <= len(lat) <= 4:
        return False
    return bool(load().nf_cluster_moments_tiled_supported(_lat4(lat), _dtype_code_of(dtype), _block_sites(block_sites)))


def cluster_moments_tiled_plan(lat, dtype, block_sites=0, per_pass=0):
    """What nf_cluster_moments_tiled will do on the lattice `lat` in `dtype`: dict(blocks (per chain), block_sites (in
    force), quantities, per_pass (in force; 0 asks for all), passes, table_entries (H: labels k and k + H share an
    entry), launches (kernels: 2 + 2 passes), lds_bytes).  Pure host code."""
    if not 1 <= len(lat) <= 4:
        raise NormflowHipError(f"cluster_moments_tiled_plan: lattices of 1 to 4 axes, got {tuple(lat)}")
    out = MomentsTiledPlan()
    _check(load().nf_cluster_moments_tiled_plan(_lat4(lat), _dtype_code_of(dtype), _block_sites(block_sites),
                                                int(per_pass or 0), C.byref(out)), "nf_cluster_moments_tiled_plan")
    return {name: getattr(out, name) for name, _ in MomentsTiledPlan._fields_}


def cluster_moments_tiled_workspace(Cn, lat, block_sites=0, per_pass=0):
    """nf_cluster_moments_tiled_workspace: the bytes of the workspace of a call on Cn chains on `lat`; pure host code."""
    return int(load().nf_cluster_moments_tiled_workspace(int(Cn), _lat4(tuple(lat)), _block_sites(block_sites),
                                                         int(per_pass or 0)))


def moments_max_workspace():
    """The footprint that `cluster_moments_tiled(per_pass=None)` stays under: NF_MOMENTS_MAX_WORKSPACE bytes, 1 GiB unless
    the environment says otherwise.  A footprint policy, not a tuned number."""
    return int(os.environ.get("NF_MOMENTS_MAX_WORKSPACE", 1 << 30))


def cluster_moments_tiled_per_pass(Cn, lat, block_sites=0):
    """The `per_pass` that `cluster_moments_tiled(per_pass=None)` takes: the largest whose workspace stays under
    `moments_max_workspace()`, and at least 1.  The workspace is linear in per_pass, so two planner calls give it."""
    one = cluster_moments_tiled_workspace(Cn, lat, block_sites, 1)
    step = cluster_moments_tiled_workspace(Cn, lat, block_sites, 2) - one if _sites(lat) > 1 else 0
    nq = 1 + 2 * sum(1 for n in lat if n > 1)
    if one == 0 or step <= 0:
        return 1
    return int(max(1, min(nq, 1 + (moments_max_workspace() - one) // step)))


def cluster_moments_tiled(phi, labels, want_moments=False, block_sites=0, per_pass=None, workspace=None):
    """nf_cluster_moments_tiled: `cluster_moments` for chains that live in HBM, any lattice of 1 to 4 axes with fewer than
    2^31 sites; the same dict.  status and moments are `cluster_moments`' bit for bit, out differs in the order of the sums
    of squares alone (blocks of `block_sites` slots, 0: the default; include/normflow_hip.h).  The 1 + 2 d quantities go in
    passes of `per_pass` (None: `cluster_moments_tiled_per_pass`; it changes the footprint and the launches, never a bit).
    2 + 2 passes launches and 1 + passes memsets on the current stream.  The workspace comes from torch's caching
    allocator per call (stream-aware and graph-pool safe), or is `workspace`: a uint8 tensor of at least
    nf_cluster_moments_tiled_workspace bytes.  Graph capture: as `cluster_moments`, call `twiddle_table(lat, device)` first."""
    _require_device(phi, labels)
    lat = tuple(phi.shape[1:])
    if not phi.is_contiguous() or not 1 <= len(lat) <= 4:
        raise NormflowHipError("cluster_moments_tiled needs contiguous phi (C, *L) with 1 to 4 lattice axes, got "
                               f"{tuple(phi.shape)}")
    if labels.shape != phi.shape or labels.dtype != torch.int32 or not labels.is_contiguous() or labels.device != phi.device:
        raise NormflowHipError(f"cluster_moments_tiled: labels must be a contiguous int32 tensor {tuple(phi.shape)} on "
                               f"{phi.device}, got {tuple(labels.shape)} {labels.dtype} on {labels.device}")
    Cn, dev, bs = phi.shape[0], phi.device, _block_sites(block_sites)
    pp = cluster_moments_tiled_per_pass(Cn, lat, bs) if per_pass is None else int(per_pass)
    if workspace is None:
        need = load().nf_cluster_moments_tiled_workspace(Cn, _lat4(lat), bs, pp)
        workspace = torch.empty(max(int(need), 256), dtype=torch.uint8, device=dev)
    out = torch.empty((Cn, 6), dtype=torch.float64, device=dev)
    status = torch.empty((Cn,), dtype=torch.int32, device=dev)
    moments = torch.empty((Cn,) + lat, dtype=torch.int64, device=dev) if want_moments else None
    tw = twiddle_table(lat, dev)
    _check(load().nf_cluster_moments_tiled(_ptr(phi), _ptr(labels), _ptr(out), _ptr(status), _ptr(moments), Cn, _lat4(lat),
                                           _ptr(tw), _dtype_code(phi), bs, pp, _ptr(workspace), workspace.numel(),
                                           _stream()), "nf_cluster_moments_tiled")
    pad = 4 - len(lat)
    return dict(out=torch.cat([out[:, :2], out[:, 2 + pad:]], dim=1), status=status, moments=moments)


# ========================================================================= the spectrum, slots in HBM (nf_cluster_spectrum_tiled.hip)
SPECTRUM_TILED_MAX_PASS = 16            # quantities per pass: nf_cluster_spectrum's cap


class SpectrumTiledPlan(C.Structure):
    """nf_spectrum_tiled_plan (include/normflow_hip.h)."""
    _fields_ = [("blocks", C.c_int64), ("block_sites", C.c_int32), ("kmax", C.c_int32 * 4), ("columns", C.c_int32),
                ("quantities", C.c_int32), ("per_pass", C.c_int32), ("passes", C.c_int32), ("table_entries", C.c_int32),
                ("launches", C.c_int32), ("lds_bytes", C.c_int64)]


def cluster_spectrum_tiled_supported(lat, dtype, momenta='all', block_sites=0):
    """True if nf_cluster_spectrum_tiled takes chains on the lattice `lat` (1 to 4 extents) in `dtype` at `momenta` with
    blocks of `block_sites` sites (0: the default): the launcher's own planner, pure host code."""
    if dtype not in (torch.float32, torch.float64) or not 1 <= len(lat) <= 4:
        return False
    return bool(load().nf_cluster_spectrum_tiled_supported(_lat4(lat), _dtype_code_of(dtype), spectrum_kmax(momenta),
                                                           _block_sites(block_sites)))


def cluster_spectrum_tiled_plan(lat, dtype, momenta='all', block_sites=0, per_pass=0):
    """What nf_cluster_spectrum_tiled will do on the lattice `lat` in `dtype`: dict(blocks (per chain), block_sites (in
    force), kmax (K_mu of the four padded axes), columns, quantities, per_pass (in force; 0 asks for min(Q, 16)), passes,
    table_entries (H), launches (kernels: 2 + 2 passes), lds_bytes (of the scatter kernel)).  Pure host code."""
    if not 1 <= len(lat) <= 4:
        raise NormflowHipError(f"cluster_spectrum_tiled_plan: lattices of 1 to 4 axes, got {tuple(lat)}")
    out = SpectrumTiledPlan()
    _check(load().nf_cluster_spectrum_tiled_plan(_lat4(lat), _dtype_code_of(dtype), spectrum_kmax(momenta),
                                                 _block_sites(block_sites), int(per_pass or 0), C.byref(out)),
           "nf_cluster_spectrum_tiled_plan")
    d = {name: getattr(out, name) for name, _ in SpectrumTiledPlan._fields_}
    d['kmax'] = tuple(out.kmax)
    return d


def cluster_spectrum_tiled_workspace(Cn, lat, momenta='all', block_sites=0, per_pass=0):
    """nf_cluster_spectrum_tiled_workspace: the bytes of the workspace of a call on Cn chains on `lat`; pure host code."""
    return int(load().nf_cluster_spectrum_tiled_workspace(int(Cn), _lat4(tuple(lat)), spectrum_kmax(momenta),
                                                          _block_sites(block_sites), int(per_pass or 0)))


def cluster_spectrum_tiled_per_pass(Cn, lat, momenta='all', block_sites=0):
    """The `per_pass` that `cluster_spectrum_tiled(per_pass=None)` takes: the largest value <= min(Q, 16) whose workspace
    stays under `moments_max_workspace()`, and at least 1.  The workspace is linear in per_pass, so two planner calls
    give it."""
    lat = tuple(lat)
    K = spectrum_momenta(lat, momenta)
    cap = min(SPECTRUM_TILED_MAX_PASS, 1 + sum(2 * k - (1 if k and 2 * k == n else 0) for k, n in zip(K, lat)))
    one = cluster_spectrum_tiled_workspace(Cn, lat, momenta, block_sites, 1)
    if one == 0 or cap < 2:
        return 1
    step = cluster_spectrum_tiled_workspace(Cn, lat, momenta, block_sites, 2) - one
    if step <= 0:
        return 1
    return int(max(1, min(cap, 1 + (moments_max_workspace() - one) // step)))


def cluster_spectrum_tiled(phi, labels, momenta='all', block_sites=0, per_pass=None, workspace=None):
    """nf_cluster_spectrum_tiled: `cluster_spectrum` for chains that live in HBM, any lattice of 1 to 4 axes with fewer
    than 2^31 sites; the same dict(out, status, momenta).  status is `cluster_spectrum`'s bit for bit, out differs in the
    order of the sums of squares alone (blocks of `block_sites` slots, 0: the default; include/normflow_hip.h): columns 0
    and 1 and the k = 1 columns are `cluster_moments_tiled`'s bits at the same `block_sites`.  The Q quantities go in passes
    of `per_pass` <= 16 (None: `cluster_spectrum_tiled_per_pass`; it changes the footprint and the launches, never a bit).
    2 + 2 passes launches and 1 + passes memsets on the current stream.  The workspace comes from torch's caching
    allocator per call (stream-aware and graph-pool safe), or is `workspace`: a uint8 tensor of at least
    nf_cluster_spectrum_tiled_workspace bytes.  Graph capture: as `cluster_moments`, call `twiddle_table(lat, device)` first."""
    _require_device(phi, labels)
    lat = tuple(phi.shape[1:])
    if not phi.is_contiguous() or not 1 <= len(lat) <= 4:
        raise NormflowHipError("cluster_spectrum_tiled needs contiguous phi (C, *L) with 1 to 4 lattice axes, got "
                               f"{tuple(phi.shape)}")
    if labels.shape != phi.shape or labels.dtype != torch.int32 or not labels.is_contiguous() or labels.device != phi.device:
        raise NormflowHipError(f"cluster_spectrum_tiled: labels must be a contiguous int32 tensor {tuple(phi.shape)} on "
                               f"{phi.device}, got {tuple(labels.shape)} {labels.dtype} on {labels.device}")
    kmax = spectrum_kmax(momenta)
    K = spectrum_momenta(lat, momenta)
    Cn, dev, bs = phi.shape[0], phi.device, _block_sites(block_sites)
    pp = cluster_spectrum_tiled_per_pass(Cn, lat, momenta, bs) if per_pass is None else int(per_pass)
    if workspace is None:
        need = load().nf_cluster_spectrum_tiled_workspace(Cn, _lat4(lat), kmax, bs, pp)
        workspace = torch.empty(max(int(need), 256), dtype=torch.uint8, device=dev)
    out = torch.empty((Cn, 2 + sum(K)), dtype=torch.float64, device=dev)
    status = torch.empty((Cn,), dtype=torch.int32, device=dev)
    tw = twiddle_table(lat, dev)
    _check(load().nf_cluster_spectrum_tiled(_ptr(phi), _ptr(labels), _ptr(out), _ptr(status), Cn, _lat4(lat), kmax, _ptr(tw),
                                            _dtype_code(phi), bs, pp, _ptr(workspace), workspace.numel(), _stream()),
           "nf_cluster_spectrum_tiled")
    return dict(out=out, status=status, momenta=K)


# ========================================================================= the modes, slots in HBM (nf_cluster_modes_tiled.hip)
MODES_TILED_MAX_PASS = 16               # quantities per pass: nf_cluster_modes' cap


class ModesTiledPlan(C.Structure):
    """nf_modes_tiled_plan (include/normflow_hip.h)."""
    _fields_ = [("blocks", C.c_int64), ("block_sites", C.c_int32), ("N", C.c_int32), ("columns", C.c_int32),
                ("quantities", C.c_int32), ("per_pass", C.c_int32), ("passes", C.c_int32), ("table_entries", C.c_int32),
                ("launches", C.c_int32), ("lds_bytes", C.c_int64)]


def modes_quantities(lat, modes):
    """Q of the rule: 1 + sum over the list of (2 - [the momentum is self-conjugate])."""
    lat = tuple(int(n) for n in lat)
    return 1 + sum(1 if all((2 * n) % L == 0 for n, L in zip(m, lat)) else 2 for m in modes_reduced(lat, modes))


def cluster_modes_tiled_supported(lat, dtype, modes, block_sites=0):
    """True if nf_cluster_modes_tiled takes chains on the lattice `lat` (1 to 4 extents) in `dtype` at the momenta `modes`
    with blocks of `block_sites` sites (0: the default): the launcher's own planner, pure host code (the reason for a
    False is `last_error()`)."""
    if dtype not in (torch.float32, torch.float64) or not 1 <= len(lat) <= 4:
        return False
    arr, P = _modes_array(lat, modes)
    return bool(load().nf_cluster_modes_tiled_supported(_lat4(lat), _dtype_code_of(dtype), arr, P, _block_sites(block_sites)))


def cluster_modes_tiled_plan(lat, dtype, modes, block_sites=0, per_pass=0):
    """What nf_cluster_modes_tiled will do on the lattice `lat` in `dtype` at `modes`: dict(blocks (per chain), block_sites
    (in force), N (the lcm of the extents), columns (2 + P), quantities, per_pass (in force; 0 asks for min(Q, 16)), passes,
    table_entries (H), launches (kernels: 2 + 2 passes), lds_bytes (of the scatter kernel)).  Pure host code."""
    if not 1 <= len(lat) <= 4:
        raise NormflowHipError(f"cluster_modes_tiled_plan: lattices of 1 to 4 axes, got {tuple(lat)}")
    arr, P = _modes_array(lat, modes)
    out = ModesTiledPlan()
    _check(load().nf_cluster_modes_tiled_plan(_lat4(lat), _dtype_code_of(dtype), arr, P, _block_sites(block_sites),
                                              int(per_pass or 0), C.byref(out)), "nf_cluster_modes_tiled_plan")
    return {name: getattr(out, name) for name, _ in ModesTiledPlan._fields_}


def cluster_modes_tiled_workspace(Cn, lat, modes, block_sites=0, per_pass=0):
    """nf_cluster_modes_tiled_workspace: the bytes of the workspace of a call on Cn chains on `lat` at the momenta `modes`
    (or, for an int, at that many quantities Q); pure host code."""
    Q = int(modes) if isinstance(modes, int) else modes_quantities(lat, modes)
    return int(load().nf_cluster_modes_tiled_workspace(int(Cn), _lat4(tuple(lat)), Q, _block_sites(block_sites),
                                                       int(per_pass or 0)))


def cluster_modes_tiled_per_pass(Cn, lat, modes, block_sites=0):
    """The `per_pass` that `cluster_modes_tiled(per_pass=None)` takes: the largest value <= min(Q, 16) whose workspace
    stays under `moments_max_workspace()`, and at least 1.  The workspace is linear in per_pass, so two planner calls
    give it."""
    lat = tuple(lat)
    Q = int(modes) if isinstance(modes, int) else modes_quantities(lat, modes)
    cap = min(MODES_TILED_MAX_PASS, Q)
    one = cluster_modes_tiled_workspace(Cn, lat, Q, block_sites, 1)
    if one == 0 or cap < 2:
        return 1
    step = cluster_modes_tiled_workspace(Cn, lat, Q, block_sites, 2) - one
    if step <= 0:
        return 1
    return int(max(1, min(cap, 1 + (moments_max_workspace() - one) // step)))


def cluster_modes_tiled(phi, labels, modes, block_sites=0, per_pass=None, workspace=None):
    """nf_cluster_modes_tiled: `cluster_modes` for chains that live in HBM, any lattice of 1 to 4 axes with fewer than 2^31
    sites whose lcm of extents is at most 65536; the same dict(out, status, modes).  status is `cluster_modes`' bit for bit,
    out differs in the order of the sums of squares alone (blocks of `block_sites` slots, 0: the default;
    include/normflow_hip.h): columns 0 and 1 are `cluster_moments_tiled`'s bits at the same `block_sites`.  The Q quantities
    go in passes of `per_pass` <= 16 (None: `cluster_modes_tiled_per_pass`; it changes the footprint and the launches, never
    a bit).  2 + 2 passes launches and 1 + passes memsets on the current stream.  The workspace comes from torch's caching
    allocator per call (stream-aware and graph-pool safe), or is `workspace`: a uint8 tensor of at least
    nf_cluster_modes_tiled_workspace bytes.  Graph capture: as `cluster_modes`, call this function once (or
    `mode_twiddle_table(lat, device)` and `mode_descriptor(lat, modes, device)`) before capturing."""
    _require_device(phi, labels)
    lat = tuple(phi.shape[1:])
    if not phi.is_contiguous() or not 1 <= len(lat) <= 4:
        raise NormflowHipError("cluster_modes_tiled needs contiguous phi (C, *L) with 1 to 4 lattice axes, got "
                               f"{tuple(phi.shape)}")
    if labels.shape != phi.shape or labels.dtype != torch.int32 or not labels.is_contiguous() or labels.device != phi.device:
        raise NormflowHipError(f"cluster_modes_tiled: labels must be a contiguous int32 tensor {tuple(phi.shape)} on "
                               f"{phi.device}, got {tuple(labels.shape)} {labels.dtype} on {labels.device}")
    Cn, dev, bs = phi.shape[0], phi.device, _block_sites(block_sites)
    # the per-list cache of `cluster_modes`: a list seen before costs one dictionary look-up
    try:
        key = (lat, modes if isinstance(modes, tuple) else tuple(modes), dev)
        hit = _MODE_CALLS.get(key)
    except TypeError:                                         # momenta given as lists: not hashable, the slow way
        key = hit = None
    if hit is None:
        hit = (modes_reduced(lat, modes),) + mode_descriptor(lat, modes, dev) + (mode_twiddle_table(lat, dev),)
        if key is not None:
            _MODE_CALLS[key] = hit
    reduced, desc, N, tw = hit
    Q = desc.shape[0]
    pp = cluster_modes_tiled_per_pass(Cn, lat, Q, bs) if per_pass is None else int(per_pass)
    if workspace is None:
        need = load().nf_cluster_modes_tiled_workspace(Cn, _lat4(lat), Q, bs, pp)
        workspace = torch.empty(max(int(need), 256), dtype=torch.uint8, device=dev)
    elif workspace.dtype != torch.uint8 or workspace.device != dev or not workspace.is_contiguous():
        raise NormflowHipError(f"cluster_modes_tiled: workspace must be a contiguous uint8 tensor on {dev}, got "
                               f"{workspace.dtype} on {workspace.device}")
    out = torch.empty((Cn, 2 + len(reduced)), dtype=torch.float64, device=dev)
    status = torch.empty((Cn,), dtype=torch.int32, device=dev)
    _check(load().nf_cluster_modes_tiled(_ptr(phi), _ptr(labels), _ptr(out), _ptr(status), Cn, _lat4(lat), _ptr(desc), Q,
                                         _ptr(tw), N, _dtype_code(phi), bs, pp, _ptr(workspace), workspace.numel(),
                                         _stream()), "nf_cluster_modes_tiled")
    return dict(out=out, status=status, modes=reduced)


# ========================================================================= observables of sampler rows (nf_measure.hip)
MEASURE_REGIMES = ('resident', 'packed', 'segmented')       # NF_MEASURE_RESIDENT, _PACKED, _SEGMENTED


class MeasurePlan(C.Structure):
    """nf_measure_plan (include/normflow_hip.h)."""
    _fields_ = [("regime", C.c_int32), ("rows_per_group", C.c_int32), ("segments", C.c_int32), ("seg_len", C.c_int32),
                ("stage_planes", C.c_int32), ("lanes", C.c_int32), ("vec", C.c_int32), ("n_out", C.c_int32),
                ("lds_bytes", C.c_int64), ("lds_budget", C.c_int64)]


def measure_supported(lat, dtype):
    """True if nf_lattice_measure takes rows on the lattice `lat` (1 to 4 extents) in `dtype`: the launcher's own planner,
    pure host code."""
    return _planner_supported("nf_lattice_measure_supported", lat, dtype)


def measure_plan(lat, dtype):
    """What nf_lattice_measure will do on the lattice `lat` in `dtype`: dict(regime ('resident', 'packed' or 'segmented'),
    rows_per_group, segments, seg_len, stage_planes, lanes, vec, n_out (of the lattice padded to four axes), march_axis
    (the axis of `lat` that segments cut: its slowest of extent > 1), lds_bytes, lds_budget).  Pure host code."""
    out = _planner_plan("measure_plan", "nf_lattice_measure_plan", lat, dtype, MeasurePlan())
    march = next((mu for mu, n in enumerate(lat) if n > 1), len(lat) - 1)
    return dict(regime=MEASURE_REGIMES[out.regime], rows_per_group=out.rows_per_group, segments=out.segments,
                seg_len=out.seg_len, stage_planes=out.stage_planes, lanes=out.lanes, vec=out.vec, n_out=out.n_out,
                march_axis=march, lds_bytes=out.lds_bytes, lds_budget=out.lds_budget)


def measure_n_out(lat):
    """The width of a measure row of the lattice `lat` (1 to 4 axes), which the kernels pad to four axes with extents of 1:
    7 scalars (sum phi, phi^2, phi^4, the links of the four axes) and one slice sum per plane of every axis."""
    return 7 + sum(lat) + 4 - len(lat)


def _measure_out(what, out, cfgs, n_out):
    """`out` of a measure wrapper: a new (N, n_out) float64 tensor, or the caller's contiguous one of that shape."""
    if out is None:
        return torch.empty((cfgs.shape[0], n_out), dtype=torch.float64, device=cfgs.device)
    _require_device(out)
    if out.shape != (cfgs.shape[0], n_out) or out.dtype != torch.float64 or not out.is_contiguous():
        raise NormflowHipError(f"{what}: out must be a contiguous float64 tensor ({cfgs.shape[0]}, {n_out}), got "
                               f"{tuple(out.shape)} {out.dtype}")
    return out


def lattice_measure(cfgs, workspace=None, out=None):
    """nf_lattice_measure: the (N, 7 + sum of the four padded extents) float64 statistics of the contiguous rows cfgs
    (N, *L), 1 to 4 axes, fp32 or fp64, in one pass (two launches on the segmented regime).  The workspace comes from
    torch's caching allocator per call (stream-aware and graph-pool safe, like `_workspace`), or is `workspace`: a uint8
    tensor of at least nf_lattice_measure_workspace bytes.  `out`: write the rows there instead of into a new tensor."""
    _require_device(cfgs)
    lat = tuple(cfgs.shape[1:])
    if not cfgs.is_contiguous() or not 1 <= len(lat) <= 4:
        raise NormflowHipError(f"lattice_measure needs contiguous cfgs (N, *L) with 1 to 4 lattice axes, got {tuple(cfgs.shape)}")
    N, lat4, code = cfgs.shape[0], _lat4(lat), _dtype_code(cfgs)
    out = _measure_out("lattice_measure", out, cfgs, measure_n_out(lat))
    if workspace is None:
        need = load().nf_lattice_measure_workspace(N, lat4, code)
        workspace = torch.empty(int(need), dtype=torch.uint8, device=cfgs.device) if need else None
    _check(load().nf_lattice_measure(_ptr(cfgs), _ptr(out), N, lat4, _ptr(workspace),
                                     0 if workspace is None else workspace.numel(), code, _stream()), "nf_lattice_measure")
    return out


# ========================================================================= the same by bricks (nf_measure_tiled.hip)
class MeasureTiledPlan(C.Structure):
    """nf_measure_tiled_plan (include/normflow_hip.h)."""
    _fields_ = [("axis0", C.c_int32), ("axis1", C.c_int32), ("e0", C.c_int32), ("e1", C.c_int32), ("n0", C.c_int32),
                ("n1", C.c_int32), ("bricks", C.c_int32), ("lanes", C.c_int32), ("vec", C.c_int32), ("n_out", C.c_int32),
                ("n_part", C.c_int32), ("reserved", C.c_int32), ("lds_bytes", C.c_int64), ("lds_budget", C.c_int64)]


def _brick_bytes(brick_bytes):
    """None / 0: the library's default cap."""
    b = 0 if brick_bytes is None else int(brick_bytes)
    if b < 0:
        raise NormflowHipError(f"brick_bytes must be None or >= 0, got {brick_bytes}")
    return b


def measure_tiled_supported(lat, dtype, brick_bytes=None):
    """True if nf_lattice_measure_tiled takes rows on the lattice `lat` (1 to 4 extents) in `dtype` with bricks of at most
    `brick_bytes` (None: the default cap): the launcher's own planner, pure host code."""
    if dtype not in (torch.float32, torch.float64) or not 1 <= len(lat) <= 4:
        return False
    return bool(load().nf_lattice_measure_tiled_supported(_lat4(lat), _brick_bytes(brick_bytes),
                                                          NF_F32 if dtype == torch.float32 else NF_F64))


def measure_tiled_plan(lat, dtype, brick_bytes=None):
    """What nf_lattice_measure_tiled will do on the lattice `lat` in `dtype` with bricks of at most `brick_bytes`:
    dict(axis0, axis1 (the cut axes of `lat`; axis1 None when `lat` has one axis of extent > 1), e0, e1 (planes of axis0
    and sub-planes of axis1 per brick), n0, n1 (bricks along them), bricks (per row), lanes, vec, n_out (of the lattice
    padded to four axes), n_part, lds_bytes, lds_budget).  Pure host code."""
    if not 1 <= len(lat) <= 4:
        raise NormflowHipError(f"measure_tiled_plan: lattices of 1 to 4 axes, got {tuple(lat)}")
    code = NF_F32 if dtype == torch.float32 else NF_F64 if dtype == torch.float64 else NF_F16
    out = MeasureTiledPlan()
    _check(load().nf_lattice_measure_tiled_plan(_lat4(lat), _brick_bytes(brick_bytes), code, C.byref(out)),
           "nf_lattice_measure_tiled_plan")
    pad = 4 - len(lat)
    return dict(axis0=max(out.axis0 - pad, 0), axis1=None if out.axis1 < 0 else out.axis1 - pad, e0=out.e0, e1=out.e1,
                n0=out.n0, n1=out.n1, bricks=out.bricks, lanes=out.lanes, vec=out.vec, n_out=out.n_out, n_part=out.n_part,
                lds_bytes=out.lds_bytes, lds_budget=out.lds_budget)


def lattice_measure_tiled(cfgs, brick_bytes=None, workspace=None, out=None):
    """nf_lattice_measure_tiled: `lattice_measure`'s (N, 7 + sum of the four padded extents) float64 statistics of the
    contiguous rows cfgs (N, *L) by bricks of at most `brick_bytes` (None: the default cap), for rows of any size: two
    launches.  The workspace comes from torch's caching allocator per call (stream-aware and graph-pool safe, like
    `_workspace`), or is `workspace`: a uint8 tensor of at least nf_lattice_measure_tiled_workspace bytes.  One call per
    batch: there is no slab loop (N x bricks workgroups must fit one launch, 2^24 - 1).  `out` as for `lattice_measure`."""
    _require_device(cfgs)
    lat = tuple(cfgs.shape[1:])
    if not cfgs.is_contiguous() or not 1 <= len(lat) <= 4:
        raise NormflowHipError(f"lattice_measure_tiled needs contiguous cfgs (N, *L) with 1 to 4 lattice axes, got "
                               f"{tuple(cfgs.shape)}")
    N, lat4, code, cap = cfgs.shape[0], _lat4(lat), _dtype_code(cfgs), _brick_bytes(brick_bytes)
    out = _measure_out("lattice_measure_tiled", out, cfgs, measure_n_out(lat))
    if workspace is None:
        need = load().nf_lattice_measure_tiled_workspace(N, lat4, cap, code)
        workspace = torch.empty(max(int(need), 256), dtype=torch.uint8, device=cfgs.device)
    _check(load().nf_lattice_measure_tiled(_ptr(cfgs), _ptr(out), N, lat4, cap, _ptr(workspace), workspace.numel(), code,
                                           _stream()), "nf_lattice_measure_tiled")
    return out

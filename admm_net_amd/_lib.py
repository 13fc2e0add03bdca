"""ctypes binding of libadmmnet_hip.so (the C ABI of include/admmnet.h).

This is the stub a maintainer of the reference would add next to admm_net.py
(see INTEGRATION.md).  There is NO fallback: if the shared library is missing
or a call fails, an exception is raised.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int32, c_int64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libadmmnet_hip.so")


class Cfg(ctypes.Structure):
    """struct admmnet_cfg (include/admmnet.h).  ``reserved[0]`` is the C struct's ``sub_batch`` (0 = one batch) and
    ``reserved[1]`` its ``reserved[0]``, the option handle (0 = the process defaults; ``options.Options``): the field list
    keeps the two-int ``reserved`` of ABI version 1."""
    _fields_ = [("M", c_int32), ("N", c_int32), ("L", c_int32), ("K", c_int32),
                ("has_head", c_int32), ("chunk", c_int32), ("reserved", c_int32 * 2)]


class AdamWHyper(ctypes.Structure):
    """struct admmnet_adamw_hyper (include/admmnet.h): one set of the update's constants, computed in Python double."""
    _fields_ = [("decay", c_double), ("one_minus_beta1", c_double), ("beta2", c_double), ("one_minus_beta2", c_double),
                ("step_size", c_double), ("bias_correction2_sqrt", c_double), ("eps", c_double)]


class AdmmNetError(RuntimeError):
    pass


_lib = None

# name -> (restype, argtypes); every symbol include/admmnet.h declares
SYMBOLS = {
    "admmnet_abi_version": (c_int32, []),
    "admmnet_last_error": (c_char_p, []),
    "admmnet_options_intern": (c_int32, [POINTER(c_char_p), POINTER(c_char_p), c_int32]),
    "admmnet_options_describe": (c_int64, [c_int32, c_char_p, c_int64]),
    "admmnet_raw_weight_count": (c_int64, [POINTER(Cfg)]),
    "admmnet_packed_weight_count": (c_int64, [POINTER(Cfg)]),
    "admmnet_pack_weights": (c_int32, [POINTER(Cfg), c_void_p, c_void_p]),
    "admmnet_workspace_bytes": (c_int64, [POINTER(Cfg), c_int64]),
    "admmnet_state_layout": (c_int32, [POINTER(Cfg), c_int64, POINTER(c_int64), POINTER(c_int32)]),
    "admmnet_forward_f32": (c_int32, [POINTER(Cfg), c_void_p, c_void_p, c_void_p, c_void_p, c_int64,
                                      c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "admmnet_begin": (c_int32, [POINTER(Cfg), c_int64, c_void_p, c_int64, c_void_p, c_void_p]),
    "admmnet_layer_front": (c_int32, [POINTER(Cfg), c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_int64,
                                      c_void_p, c_void_p, c_void_p, c_void_p]),
    "admmnet_layer_back": (c_int32, [POINTER(Cfg), c_void_p, c_int32, c_int64, c_void_p, c_void_p, c_void_p]),
    "admmnet_finish": (c_int32, [POINTER(Cfg), c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "admmnet_layer_weight_offset": (c_int64, [POINTER(Cfg), c_int32]),
    "admmnet_glayer_workspace_bytes": (c_int64, [POINTER(Cfg), c_int64]),
    "admmnet_glayer_f32": (c_int32, [POINTER(Cfg), c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p,
                                     c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "admmnet_glayer_spectral_f32": (c_int32, [POINTER(Cfg), c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p,
                                              c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
                                              c_void_p, c_int32, c_void_p]),
    "admmnet_eigh_workspace_bytes": (c_int64, [c_int32, c_int64]),
    "admmnet_eigh_c64": (c_int32, [c_int32, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int64,
                                   c_void_p, c_void_p]),
    "admmnet_eigh_workspace_bytes_o": (c_int64, [c_int32, c_int64, c_int32]),
    "admmnet_eigh_c64_o": (c_int32, [c_int32, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int64,
                                     c_void_p, c_void_p, c_int32]),
    "admmnet_vdvh_c64": (c_int32, [c_int32, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "admmnet_vhsv_f32": (c_int32, [c_int32, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "admmnet_train_partials": (c_int64, [c_int32, c_int64]),
    "admmnet_train_matrix_f32": (c_int32, [c_int32, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p]),
    "admmnet_train_matrix_bwd_f32": (c_int32, [c_int32, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                               c_void_p, c_void_p, c_void_p]),
    "admmnet_train_resnorm_f32": (c_int32, [c_int32, c_int64, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p]),
    "admmnet_train_resnorm_bwd_f32": (c_int32, [c_int32, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float,
                                                c_void_p, c_void_p, c_void_p, c_void_p]),
    "admmnet_train_zupdate_c64": (c_int32, [c_int32, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float,
                                            c_void_p, c_void_p]),
    "admmnet_train_zupdate_bwd_c64": (c_int32, [c_int32, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float,
                                                c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "admmnet_train_gather_c64": (c_int32, [c_int32, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "admmnet_train_scatter_c64": (c_int32, [c_int32, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "admmnet_train_herm_c64": (c_int32, [c_int32, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "admmnet_train_small_partials": (c_int64, [c_int32, c_int64, c_int64]),
    "admmnet_train_phi_c64": (c_int32, [c_int32, c_int64] + [c_void_p] * 7),
    "admmnet_train_phi_bwd_c64": (c_int32, [c_int32, c_int64] + [c_void_p] * 11),
    "admmnet_train_hinput_f32": (c_int32, [c_int32, c_int64] + [c_void_p] * 5),
    "admmnet_train_hinput_bwd_f32": (c_int32, [c_int32, c_int64] + [c_void_p] * 8),
    "admmnet_train_hproject_f32": (c_int32, [c_int32, c_int64] + [c_void_p] * 6),
    "admmnet_train_hproject_bwd_f32": (c_int32, [c_int32, c_int64] + [c_void_p] * 10),
    "admmnet_train_eigmap_f32": (c_int32, [c_int32, c_int64] + [c_void_p] * 8),
    "admmnet_train_eigmap_bwd_f32": (c_int32, [c_int32, c_int64] + [c_void_p] * 11),
    "admmnet_train_stepsize_f32": (c_int32, [c_int64, c_int64, c_float] + [c_void_p] * 8),
    "admmnet_train_stepsize_bwd_f32": (c_int32, [c_int64, c_int64, c_float] + [c_void_p] * 11),
    "admmnet_train_stepsize_pair_partials": (c_int64, [c_int64]),
    "admmnet_train_rnsum_f64": (c_int32, [c_int64] + [c_void_p] * 3),
    "admmnet_train_stepsize_pair_f32": (c_int32, [c_int64, c_float] + [c_void_p] * 9),
    "admmnet_train_stepsize_bwd_pair_front_f32": (c_int32, [c_int64, c_float] + [c_void_p] * 13),
    "admmnet_train_stepsize_bwd_pair_back_f32": (c_int32, [c_int64] + [c_void_p] * 5),
    "admmnet_train_hlayer_workspace": (c_int64, [c_int32, c_int64]),
    "admmnet_train_hlayer_f32": (c_int32, [c_int32, c_int64] + [c_void_p] * 14),
    "admmnet_train_hlayer_bwd_f32": (c_int32, [c_int32, c_int64] + [c_void_p] * 17),
    "admmnet_train_head_workspace": (c_int64, [c_int32, c_int32, c_int64, c_int32]),
    "admmnet_train_head_f32": (c_int32, [c_int32, c_int32, c_int64] + [c_void_p] * 3 + [c_float] + [c_void_p] * 5),
    "admmnet_train_head_bwd_f32": (c_int32, [c_int32, c_int32, c_int64] + [c_void_p] * 6 + [c_float] + [c_void_p] * 8),
    "admmnet_loss_partials": (c_int64, [c_int32, c_int64]),
    "admmnet_loss_anm_f32": (c_int32, [c_int32, c_int32, c_int64] + [c_void_p] * 7 + [c_float] + [c_void_p] * 5),
    "admmnet_loss_anm_bwd_f32": (c_int32, [c_int32, c_int32, c_int64] + [c_void_p] * 9 + [c_float] + [c_void_p] * 5),
    "admmnet_loss_phi_c64": (c_int32, [c_int32, c_int64, c_void_p, c_void_p, c_float, c_float, c_void_p, c_void_p, c_void_p]),
    "admmnet_loss_phi_bwd_c64": (c_int32, [c_int32, c_int64, c_void_p, c_void_p, c_void_p, c_float, c_float, c_void_p, c_void_p]),
    "admmnet_loss_spectrum_workspace_bytes": (c_int64, [c_int32, c_int32, c_int32, c_int64]),
    "admmnet_loss_spectrum_f64": (c_int32, [c_int32, c_int32, c_int32, c_int32, c_int64] + [c_void_p] * 5 + [c_float] * 3 +
                                           [c_void_p] * 3 + [c_int64, c_void_p]),
    "admmnet_loss_spectrum_bwd_f64": (c_int32, [c_int32, c_int32, c_int32, c_int32, c_int64] + [c_void_p] * 5 + [c_float] * 3 +
                                               [c_int32, c_void_p, c_int64, c_void_p, c_void_p]),
    "admmnet_loss_set_partials": (c_int64, [c_int64]),
    "admmnet_loss_set_f32": (c_int32, [c_int32, c_int32, c_int32, c_int64] + [c_void_p] * 7 + [POINTER(c_double)] + [c_void_p] * 6),
    "admmnet_loss_set_bwd_f32": (c_int32, [c_int32, c_int32, c_int32, c_int64] + [c_void_p] * 10 + [POINTER(c_double)] +
                                          [c_void_p] * 5),
    "admmnet_score_partials": (c_int64, [c_int64]),
    "admmnet_score_match_f64": (c_int32, [c_int32, c_int32, c_int64] + [c_void_p] * 5 + [POINTER(c_double)] + [c_void_p] * 6),
    "admmnet_score_ordered_f32": (c_int32, [c_int32, c_int64] + [c_void_p] * 10),
    "admmnet_crb_partials": (c_int64, [c_int64]),
    "admmnet_crb_f64": (c_int32, [c_int32, c_int32, c_int32, c_int64] + [c_void_p] * 6 + [c_int32] + [c_void_p] * 5),
    "admmnet_refine_lds_bytes": (c_int64, [c_int32, c_int32, c_int32]),
    "admmnet_refine_f64": (c_int32, [c_int32, c_int32, c_int32, c_int64] + [c_void_p] * 4 + [c_int32, c_int32, c_double, c_int32,
                                     c_double] + [c_void_p] * 6),
    "admmnet_order_lds_bytes": (c_int64, [c_int32, c_int32, c_int32]),
    "admmnet_order_f64": (c_int32, [c_int32, c_int32, c_int32, c_int64] + [c_void_p] * 6 + [c_int32, c_double, c_double, c_int32] +
                                    [c_void_p] * 9),
    "admmnet_cfar_lds_bytes": (c_int64, [c_int32, c_int32, c_int32]),
    "admmnet_cfar_f64": (c_int32, [c_int32, c_int32, c_int32, c_int32, c_int64] + [c_void_p] * 3 + [c_int32, c_double] + [c_int32] * 4 +
                                   [c_double] + [c_void_p] * 7),
    "admmnet_cfar_relax_lds_bytes": (c_int64, [c_int32, c_int32, c_int32]),
    "admmnet_cfar_relax_f64": (c_int32, [c_int32, c_int32, c_int32, c_int32, c_int64] + [c_void_p] * 3 + [c_int32, c_double] +
                                         [c_int32] * 4 + [c_double, c_void_p, c_int32, c_int32] + [c_void_p] * 7),
    "admmnet_optim_partials": (c_int64, [c_int32, POINTER(c_int64)]),
    "admmnet_optim_gradnorm_f32": (c_int32, [c_int32, POINTER(c_void_p), POINTER(c_int64), c_float] + [c_void_p] * 5),
    "admmnet_optim_scale_f32": (c_int32, [c_int32, POINTER(c_void_p), POINTER(c_int64), c_void_p, c_void_p]),
    "admmnet_optim_adamw_f32": (c_int32, [c_int32] + [POINTER(c_void_p)] * 4 + [POINTER(c_int64), POINTER(c_int32), c_int32,
                                          POINTER(AdamWHyper), c_void_p, c_void_p]),
    "admmnet_optim_pack_f32": (c_int32, [c_int32, POINTER(c_void_p), POINTER(c_int64), c_void_p, c_void_p]),
    "admmnet_optim_unpack_f32": (c_int32, [c_int32, POINTER(c_void_p), POINTER(c_int64), c_void_p, c_void_p]),
    "admmnet_spectrum_workspace_bytes": (c_int64, [c_int32, c_int32, c_int32, c_int32]),
    "admmnet_spectrum_f64": (c_int32, [c_void_p, c_int64, c_int32, c_int32, c_void_p, c_int32, c_void_p,
                                       c_int32, c_void_p, c_void_p, c_int64, c_void_p]),
    "admmnet_peak_search_workspace_bytes": (c_int64, [c_int32, c_int32, c_int32, c_int32, c_int64]),
    "admmnet_peak_search_f64": (c_int32, [c_void_p, c_int64, c_int32, c_int32, c_void_p, c_int32, c_void_p, c_int32,
                                          c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_int64,
                                          c_void_p]),
    "admmnet_peak_top_workspace_bytes": (c_int64, [c_int32, c_int32, c_int32, c_int32]),
    "admmnet_peak_top_f64": (c_int32, [c_void_p, c_int64, c_int32, c_int32, c_void_p, c_int32, c_void_p, c_int32,
                                       c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_int64,
                                       c_void_p]),
    "admmnet_regional_maxima_f64": (c_int32, [c_void_p, c_int64, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    "admmnet_synth_batch": (c_int32, [c_int64, c_int32, c_int32, c_int32, ctypes.c_uint64, c_double, c_double, c_double,
                                      c_double, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_void_p, c_void_p]),
    "admmnet_synth_scenes": (c_int32, [c_int64, c_int32, c_int32, c_int32, c_int32, c_double, ctypes.c_uint64, c_double,
                                       c_double, c_double, c_double, c_int32] + [c_void_p] * 13),
    "admmnet_layer_back_pair": (c_int32, [POINTER(Cfg), c_void_p, c_int32, c_int64, c_void_p, c_void_p, c_void_p]),
    "admmnet_profile_enable": (c_int32, [c_int32]),
    "admmnet_profile_read": (c_int32, [c_void_p, c_void_p, c_int32]),
    "admmnet_profile_dropped": (c_int64, []),
}


def load():
    """Load the HIP extension; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise AdmmNetError(
            f"{LIB_PATH} is missing: build it with `python -m admm_net_amd.build` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)   # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if lib.admmnet_abi_version() != 1:
        raise AdmmNetError("ABI version mismatch")
    _lib = lib
    return lib


def check(rc: int, what: str):
    if rc != 0:
        msg = load().admmnet_last_error()
        raise AdmmNetError(f"{what} failed (code {rc}): {msg.decode() if msg else ''}")

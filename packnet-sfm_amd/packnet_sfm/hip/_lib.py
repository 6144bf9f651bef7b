"""ctypes binding of libpnsfm_hip.so -- the C ABI declared in include/pnsfm.h.

The library is the product: there is NO fallback.  If the gfx950 build is missing (or is not a gfx950
build) importing any HIP-backed module fails loudly here.
"""
import ctypes
import os

import torch  # noqa: F401  -- MUST come first: it loads PyTorch-ROCm's own libamdhip64.so.7, which this library then
#                              shares; loading ours first would pull a second HIP runtime (/opt/rocm) into the process

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.abspath(os.path.join(_HERE, "..", "..", "csrc"))
LIB_PATH = os.path.join(_CSRC, "libpnsfm_hip.so")

_p = ctypes.c_void_p
_i = ctypes.c_int
_f = ctypes.c_float
_sz = ctypes.c_size_t
_ll = ctypes.c_longlong
_d = ctypes.c_double

# name -> (restype, argtypes); mirrors include/pnsfm.h one to one
SIGNATURES = {
    "pnsfm_version": (_i, []),
    "pnsfm_last_error": (ctypes.c_char_p, []),
    "pnsfm_build_target": (ctypes.c_char_p, []),
    "pnsfm_conv2d_packed_elems_fwd": (_sz, [_i, _i, _i]),
    "pnsfm_conv2d_packed_elems_bwd": (_sz, [_i, _i, _i]),
    "pnsfm_conv2d_pack_weights": (_i, [_p, _p, _p, _i, _i, _i, _p]),
    "pnsfm_conv2d_pack_item_bytes": (_sz, []),
    "pnsfm_conv2d_pack_item_fill": (_i, [_p, _p, _p, _p, _i, _i, _i, _i]),
    "pnsfm_conv2d_pack_table": (_i, [_p, _i, _i, _p]),
    "pnsfm_conv2d_forward": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _p]),
    "pnsfm_conv2d_backward_data": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _i, _p]),
    "pnsfm_conv2d_backward_data_add": (_i, [_p, _p, _p, _p, ctypes.c_longlong, _i, _i, _i, _i, _i, _i, _p]),
    "pnsfm_conv2d_backward_weight": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _p]),
    "pnsfm_conv2d_forward_cat": (_i, [_p, _i, _p, _i, _p, _i, _p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "pnsfm_conv2d_backward_weight_cat": (_i, [_p, _i, _p, _i, _p, _i, _p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "pnsfm_conv2d_cat_wgrad_supported": (_i, [_i, _i, _i, _i, _i, _i, _i, _i]),
    "pnsfm_conv2d_forward_strided": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _p]),
    "pnsfm_conv2d_backward_weight_strided": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _p]),
    "pnsfm_conv2d_forward_rows": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p]),
    "pnsfm_conv2d_backward_data_rows": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p]),
    "pnsfm_conv2d_backward_weight_rows": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p]),
    "pnsfm_groupnorm_ws_doubles": (_sz, [_i, _i, _i]),
    "pnsfm_groupnorm_act_forward": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _f, _i, _p]),
    "pnsfm_groupnorm_act_backward": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "pnsfm_set_gn_fused": (_i, [_i]),
    "pnsfm_space_to_depth": (_i, [_p, _p, _i, _i, _i, _i, _sz, _p]),
    "pnsfm_depth_to_space": (_i, [_p, _p, _i, _i, _i, _i, _p]),
    "pnsfm_conv3d_forward": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "pnsfm_conv3d_backward_data": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "pnsfm_conv3d_backward_weight": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "pnsfm_set_pack3d_fold": (_i, [_i]),
    "pnsfm_conv3d_d2s_folded": (_i, [_p, _p, _i, _i]),
    "pnsfm_conv3d_forward_d2s": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "pnsfm_conv3d_rows_folded": (_i, [_p, _p, _i]),
    "pnsfm_conv3d_forward_rows": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _p]),
    "pnsfm_conv3d_backward_data_rows": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _i, _p]),
    "pnsfm_conv3d_backward_weight_rows": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _p]),
    "pnsfm_conv3d_backward_data_ring": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "pnsfm_conv3d_backward_weight_ring": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _p]),
    "pnsfm_conv3d_forward_t": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _p]),
    "pnsfm_conv3d_backward_data_t": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _i, _p]),
    "pnsfm_conv3d_backward_weight_epi": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _p]),
    "pnsfm_conv3d_forward_rows_t": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _p]),
    "pnsfm_conv3d_backward_data_rows_t": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _p]),
    "pnsfm_conv3d_backward_weight_rows_epi": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _p]),
    "pnsfm_conv2d_pack_tapt_supported": (_i, [_i, _i, _i]),
    "pnsfm_conv2d_pack_weights_t": (_i, [_p, _p, _p, _i, _i, _i, _i, _p]),
    "pnsfm_conv2d_pack_item_fill_t": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i]),
    "pnsfm_conv2d_backward_weight_epi": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p]),
    "pnsfm_pack_bias_eff_backward_add": (_i, [_p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _p]),
    "pnsfm_invdepth_act_forward": (_i, [_p, _p, _sz, _f, _p]),
    "pnsfm_invdepth_act_backward": (_i, [_p, _p, _p, _sz, _f, _p]),
    "pnsfm_pose_vec2mat_forward": (_i, [_p, _p, _i, _p]),
    "pnsfm_upsample_nearest_forward": (_i, [_p, _p, _i, _i, _i, _i, _p]),
    "pnsfm_upsample_nearest_backward": (_i, [_p, _p, _i, _i, _i, _i, _p]),
    "pnsfm_loss_combine_forward": (_i, [_p, _i, _p, _i, _f, _p, _p]),
    "pnsfm_loss_combine_backward": (_i, [_p, _i, _i, _f, _p, _p]),
    "pnsfm_pack_bias_eff_forward": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _p]),
    "pnsfm_pack_bias_eff_backward": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _p]),
    "pnsfm_pose_vec2mat_backward": (_i, [_p, _p, _p, _i, _p]),
    "pnsfm_supervised_loss_forward": (_i, [_p, _p, _p, _p, _sz, _i, _i, _p]),
    "pnsfm_supervised_loss_backward": (_i, [_p, _p, _p, _p, _p, _sz, _i, _i, _p]),
    "pnsfm_invdepth_conv_forward": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _f, _p]),
    "pnsfm_invdepth_conv_backward": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _p]),
    "pnsfm_view_synthesis_forward": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "pnsfm_view_synthesis_backward": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "pnsfm_photometric_forward": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _f, _f, _f, _i, _i, _f, _p]),
    "pnsfm_photometric_backward": (_i, [_p, _p, _p, _p, _f, _p, _i, _i, _i, _i, _f, _f, _f, _i, _i, _i, _p]),
    "pnsfm_smoothness_norm_forward": (_i, [_p, _p, _p, _p, _i, _i, _i, _p]),
    "pnsfm_smoothness_norm_backward": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _p]),
    # all scales of the multi-view loss in one launch (tables: host arrays of device pointers / ints)
    "pnsfm_view_synthesis_forward_ms": (_i, [_p, _i, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "pnsfm_view_synthesis_backward_ms": (_i, [_p, _p, _i, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "pnsfm_photometric_identity_forward": (_i, [_p, _p, _p, _i, _i, _i, _i, _f, _f, _f, _p]),
    "pnsfm_photometric_forward_ms": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _f, _f, _f, _i, _i, _p]),
    "pnsfm_photometric_backward_ms": (_i, [_p, _p, _p, _p, _f, _p, _i, _i, _i, _i, _i, _f, _f, _f, _i, _i, _p]),
    "pnsfm_smoothness_norm_forward_ms": (_i, [_p, _p, _p, _p, _i, _p, _p, _i, _p]),
    "pnsfm_smoothness_norm_backward_ms": (_i, [_p, _p, _p, _p, _i, _p, _p, _p, _i, _i, _p]),
    "pnsfm_region_ops": (_i, [_p, _i, _p]),
    # fp16 forward (evaluation / inference)
    "pnsfm_conv2d_packed_elems_h16": (_sz, [_i, _i, _i]),
    "pnsfm_set_h16_max_split": (_i, [_i]),
    "pnsfm_conv2d_pack_weights_h16": (_i, [_p, _i, _p, _i, _i, _i, _p]),
    "pnsfm_conv2d_forward_h16": (_i, [_p, _i, _p, _i, _p, _i, _p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "pnsfm_groupnorm_act_forward_h16": (_i, [_p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _f, _i, _p]),
    "pnsfm_conv3d_forward_h16": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "pnsfm_space_to_depth_h16": (_i, [_p, _p, _i, _i, _i, _i, _p]),
    "pnsfm_depth_to_space_h16": (_i, [_p, _p, _i, _i, _i, _i, _p]),
    "pnsfm_upsample_nearest_forward_h16": (_i, [_p, _p, _i, _i, _i, _i, _p]),
    "pnsfm_invdepth_conv_forward_h16": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _f, _p]),
    "pnsfm_region_ops_h16": (_i, [_p, _i, _p]),
    "pnsfm_conv2d_forward_h16g": (_i, [_p, _p]),
    "pnsfm_set_h16g_deinterleave": (_i, [_i]),
    "pnsfm_bn_fold_h16": (_i, [_p, _p, _p, _p, ctypes.c_double, _p, _i, _p]),
    "pnsfm_maxpool3x3s2_forward_h16": (_i, [_p, _p, _i, _i, _i, _p]),
    # depth evaluation (post-processing and metrics; fp32 or fp16 storage by a flag per tensor)
    "pnsfm_post_process_inv_depth": (_i, [_p, _i, _p, _i, _p, _i, _i, _i, _i, _i, _p]),
    "pnsfm_depth_metrics_ws_bytes": (_sz, [_i]),
    "pnsfm_depth_metrics": (_i, [_p, _i, _p, _i, _p, _p, _p, _p, _i, _i, _i, _i, _i, _f, _f, _i, _i, _i, _i, _i, _i, _i, _p]),
    # depth output (csrc/depth_output.h)
    "pnsfm_viz_inv_depth_ws_bytes": (_sz, [_i]),
    "pnsfm_viz_inv_depth": (_i, [_p, _i, _p, _i, _p, _i, _p, _p, _p, _i, _i, _i, _f, _i, _i, _d, _i, _p]),
    "pnsfm_depth_png16": (_i, [_p, _i, _p, _sz, _p]),
    # velocity supervision (csrc/velocity.h)
    "pnsfm_velocity_loss_forward": (_i, [_p, _p, _i, _i, _f, _p, _p, _p]),
    "pnsfm_velocity_loss_backward": (_i, [_p, _p, _i, _i, _f, _p, _p, _p]),
    # ResNet networks (csrc/resnet.h)
    "pnsfm_batchnorm_act_forward": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _f, _f, _i, _i, _p]),
    "pnsfm_batchnorm_act_backward": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _f, _i, _i, _p]),
    "pnsfm_batchnorm_last_path": (_i, []),
    "pnsfm_maxpool3x3s2_forward": (_i, [_p, _p, _p, _i, _i, _i, _p]),
    "pnsfm_maxpool3x3s2_backward": (_i, [_p, _p, _p, _i, _i, _i, _p]),
    "pnsfm_reflect_pad1_forward": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _p]),
    "pnsfm_reflect_pad1_backward": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _p]),
    "pnsfm_act_crop_forward": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _f, _f, _p]),
    "pnsfm_act_crop_backward": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _i, _f, _f, _p]),
    "pnsfm_affine": (_i, [_p, _p, _sz, _f, _f, _p]),
    "pnsfm_photometric_l1_forward": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _f, _p]),
    "pnsfm_photometric_l1_backward": (_i, [_p, _p, _p, _p, _f, _p, _i, _i, _i, _i, _i, _i, _p]),
    "pnsfm_smoothness_forward": (_i, [_p, _p, _p, _i, _i, _i, _p]),
    "pnsfm_smoothness_backward": (_i, [_p, _p, _p, _f, _f, _i, _i, _i, _p]),
    "pnsfm_adam_step": (_i, [_p, _p, _p, _p, _sz, _f, _f, _f, _f, _f, _f, _i, _p]),
    "pnsfm_adam_flat_step": (_i, [_p, _p, _p, _p, _sz, _p, _p]),
    "pnsfm_adam_flat_update": (_i, [_p, _p, _p, _p, _sz, _p, _i, _p]),
    "pnsfm_stream_wait_stream": (_i, [_p, _p]),
    "pnsfm_adam_pack_item_bytes": (_sz, []),
    "pnsfm_adam_pack_item_fill": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i]),
    "pnsfm_adam_pack_table": (_i, [_p, _i, _i, _p]),
    "pnsfm_adam_seg_bytes": (_sz, []),
    "pnsfm_adam_seg_fill": (_i, [_p, _p, _p, _p, _p, _p, _sz, _i]),
    "pnsfm_adam_segments": (_i, [_p, _i, _i, _p]),
    "pnsfm_resample8": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _p]),
    "pnsfm_jitter_totensor": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _p]),
    # depth maps and the evaluation transforms (csrc/depth_input.h)
    "pnsfm_depth_resize_preserve": (_i, [_p, _ll, _ll, _i, _i, _i, _i, _i, _p, _i, _i, _d, _d, _p]),
    "pnsfm_depth_resize_nearest": (_i, [_p, _ll, _ll, _i, _i, _i, _i, _i, _p, _i, _i, _d, _d, _p]),
    "pnsfm_totensor8": (_i, [_p, _p, _i, _i, _i, _i, _p]),
    "pnsfm_nrs_project_forward": (_i, [_p, _p, _p, _p, _i, _i, _f, _p]),
    "pnsfm_nrs_project_backward": (_i, [_p, _p, _p, _p, _p, _p, _p, _i, _i, _f, _p]),
    "pnsfm_sparse_compact_ws_ints": (_sz, [_i]),
    "pnsfm_sparse_compact": (_i, [_p, _i, _p, _p, _i, _p, _p, _p]),
    "pnsfm_sparse_pool_cells": (_i, [_p, _i, _i, _i, _p, _p]),
    "pnsfm_sparse_neighbors": (_i, [_p, _p, _p, _i, _i, _i, _i, _p, _p]),
    "pnsfm_sparse_conv": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "pnsfm_sparse_conv_backward_weight": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _p]),
    "pnsfm_sparse_maxpool_forward": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _p]),
    "pnsfm_sparse_maxpool_backward": (_i, [_p, _p, _p, _i, _i, _i, _p]),
    "pnsfm_sparse_densify": (_i, [_p, _p, _p, _i, _i, _i, _p]),
    "pnsfm_sparse_gather": (_i, [_p, _p, _p, _p, _i, _i, _i, _p]),
    "pnsfm_set_autotune": (_i, [_i]),
    "pnsfm_set_conv_variant": (_i, [_i]),
    "pnsfm_tune_shipped_entries": (_i, []),
    "pnsfm_set_conv_math": (_i, [_i]),
    "pnsfm_get_conv_math": (_i, []),
    "pnsfm_set_wgrad_variant": (_i, [_i]),
    "pnsfm_tune_set": (_i, [ctypes.POINTER(ctypes.c_int), _i, _i]),
    "pnsfm_tune_key": (_i, [_i] * 9 + [ctypes.POINTER(ctypes.c_int)]),
    "pnsfm_tune_key_rows": (_i, [_i] * 8 + [ctypes.POINTER(ctypes.c_int)]),
    "pnsfm_conv2d_last_config": (_i, [ctypes.POINTER(ctypes.c_int)]),
    "pnsfm_calib_mfma": (_i, [_p, _i, _i, _p]),
    "pnsfm_calib_copy": (_i, [_p, _p, _sz, _p]),
    "pnsfm_prof_enable": (_i, [_i]),
    "pnsfm_prof_reset": (_i, []),
    "pnsfm_prof_collect": (_i, [_i, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                ctypes.POINTER(ctypes.c_longlong)]),
    "pnsfm_prof_dump": (_i, [ctypes.c_char_p]),
}


def bind(lib):
    """Attach restype/argtypes for every symbol of include/pnsfm.h; raises if one is missing."""
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    return lib


# The product path requires device tensors.  (tests/emu flips this to run the same wrappers on the
# host-emulated build; nothing under packnet-sfm_amd/ ever does.)
REQUIRE_CUDA = True
_LIB = None


def get():
    """The loaded gfx950 library; raises ImportError if it has not been built."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "libpnsfm_hip.so not found at %s -- build it with `python __graft_entry__.py` "
                "(hipcc --offload-arch=gfx950). There is no CPU/PyTorch fallback for the HIP ops." % LIB_PATH)
        lib = bind(ctypes.CDLL(LIB_PATH))
        target = lib.pnsfm_build_target().decode()
        if target != "gfx950":
            raise ImportError("libpnsfm_hip.so was built for %r, expected 'gfx950'" % target)
        _LIB = lib
    return _LIB


class HipError(RuntimeError):
    pass


def check(rc, what):
    if rc != 0:
        raise HipError("%s failed (rc=%d): %s" % (what, rc, get().pnsfm_last_error().decode()))

"""ctypes binding of the C ABI in include/kpnerf.h — the stub a maintainer of the (pure-Python)
reference would add to call the gfx950 library.

The product library is ``keypointnerf_amd/_lib/libkpnerf_hip.so`` (built by ``build.py`` /
``__graft_entry__.build()``, hipcc --offload-arch=gfx950).  There is NO fallback: if it is missing
or cannot be loaded, ``get_library()`` raises.  ``KpnLibrary(path)`` can bind any library exporting
the same ABI; the CPU test-suite uses that to drive the host SIMT-emulator build of the very same
kernel sources (tests/simt) with numpy buffers — never through this module's default path.
"""
import ctypes
import os

# torch first: PyTorch-ROCm ships its own libamdhip64.so.7.  The library must bind to THE SAME HIP
# runtime instance as torch (device pointers and streams are shared), which the dynamic loader
# guarantees by SONAME once torch's copy is already in the process.  Loading libkpnerf_hip.so first
# would pull /opt/rocm's runtime in as a second instance ("no ROCm-capable device is detected").
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(_HERE, "_lib", "libkpnerf_hip.so")

c_f = ctypes.c_float
c_i32 = ctypes.c_int32
c_i64 = ctypes.c_int64
c_p = ctypes.c_void_p
c_sz = ctypes.c_size_t


class SceneDesc(ctypes.Structure):
    """struct kpn_scene_desc"""
    _fields_ = [(n, c_i32) for n in ("n_views", "src_h", "src_w", "geo0_h", "geo0_w", "geo1_h", "geo1_w", "tex_h",
                                     "tex_w", "disable_fg_mask")] + \
               [(n, c_f) for n in ("znear", "zfar", "nml_scale", "sigma")] + \
               [(n, c_p) for n in ("KRT", "extrin", "kpt3d", "img", "fg_mask", "geo0", "geo1", "tex")]


class RenderStages(ctypes.Structure):
    """struct kpn_render_stages"""
    _fields_ = [(n, c_p) for n in ("z_coarse", "rgba_coarse", "z_fine", "rgba_fine", "dirs", "cam_pos")]


class RenderArgs(ctypes.Structure):
    """struct kpn_render_args"""
    _fields_ = [(n, c_p) for n in ("K", "RT", "bounds")] + [("znear", c_f), ("zfar", c_f)] + \
               [(n, c_i32) for n in ("x0", "y0", "step", "nx", "ny", "n_coarse", "n_fine", "fine", "chunk_rays")] + \
               [(n, c_p) for n in ("tex_fg", "depth", "alpha", "tex_fg_fine", "depth_fine", "alpha_fine", "sdf")] + \
               [("step_y", c_i32), ("rows_kernel", c_i32), ("fuse_kernel", c_i32), ("stages", ctypes.POINTER(RenderStages))]


class TrainArgs(ctypes.Structure):
    """struct kpn_train_args"""
    _fields_ = [(n, c_p) for n in ("pix", "u_coarse", "noise_coarse", "noise_fine", "u_fine")] + \
               [("keep_coarse", ctypes.c_uint32), ("keep_fine", ctypes.c_uint32), ("rand_noise_std", c_f)]


class TrainLossArgs(ctypes.Structure):
    """struct kpn_train_loss_args"""
    _fields_ = [(n, c_p) for n in ("tex", "tex_fine", "tar", "alpha", "alpha_fine", "tar_alpha")] + [("n", c_i64)] + \
               [(n, c_f) for n in ("l1_c", "l1", "l2", "lp", "mloss")] + [("reset_ticket", c_i32)] + \
               [(n, c_p) for n in ("terms", "d_tex", "d_tex_fine", "d_alpha", "d_alpha_fine")]


class RenderGrads(ctypes.Structure):
    """struct kpn_render_grads"""
    _fields_ = [(n, c_p) for n in ("d_tex_fg", "d_depth", "d_alpha", "d_tex_fg_fine", "d_depth_fine", "d_alpha_fine", "d_sdf")]


class ParamTable(ctypes.Structure):
    """struct kpn_param_table"""
    _fields_ = [("g", c_p * 19), ("v_or_w", c_p * 19), ("b", c_p * 19), ("ani_al", c_p)]


class FieldShape(ctypes.Structure):
    """struct kpn_field_shape"""
    _fields_ = [("n_kpt", c_i32), ("sp_level", c_i32)]


N_KPT_CAPACITY, SP_LEVEL_CAPACITY = 24, 3     # KPN_N_KPT, KPN_SP_LEVEL


class AdamSegment(ctypes.Structure):
    """struct kpn_adam_segment"""
    _fields_ = [(n, c_p) for n in ("param", "grad", "exp_avg", "exp_avg_sq")] + [("count", c_i64)]


class AdamArgs(ctypes.Structure):
    """struct kpn_adam_args"""
    _fields_ = [("segments_host", ctypes.POINTER(AdamSegment)), ("n_segments", c_i32), ("step", c_i64)] + \
               [(n, ctypes.c_double) for n in ("lr", "beta1", "beta2", "eps", "weight_decay")]


# the arithmetic of the stride-1 convolution's GEMMs (kpn_conv2d_ex_*, kpn_conv_block_ex_*)
CONV_F32, CONV_BF16X3 = 0, 1


class Conv2dDesc(ctypes.Structure):
    """struct kpn_conv2d_desc"""
    _fields_ = [(n, c_i32) for n in ("N", "H", "W", "cin", "cout", "k", "pad", "has_bias")]


class Conv2dS2Desc(ctypes.Structure):
    """struct kpn_conv2d_s2_desc"""
    _fields_ = [(n, c_i32) for n in ("N", "H", "W", "cin", "cout", "kind", "has_bias")]


S2_CONV3, S2_STEM7, S2_DECONV3 = 0, 1, 2      # KPN_S2_*


class Conv2dRpDesc(ctypes.Structure):
    """struct kpn_conv2d_rp_desc"""
    _fields_ = [(n, c_i32) for n in ("N", "H", "W", "cin", "cout", "kind", "has_bias")]


RP_CONV3, RP_CONV7, RP_STEM7 = 0, 1, 2        # KPN_RP_*


class GroupNormDesc(ctypes.Structure):
    """struct kpn_group_norm_desc"""
    _fields_ = [(n, c_i32) for n in ("N", "H", "W", "C", "G", "affine", "relu")] + [("eps", c_f)]


class ConvBlockDesc(ctypes.Structure):
    """struct kpn_conv_block_desc"""
    _fields_ = [(n, c_i32) for n in ("N", "H", "W", "cin", "cout")] + [("eps", c_f)]


class ConvBlockParams(ctypes.Structure):
    """struct kpn_conv_block_params"""
    _fields_ = [("gamma", c_p * 4), ("beta", c_p * 4), ("packed", c_p * 4)]


class ConvBlockGrads(ctypes.Structure):
    """struct kpn_conv_block_grads"""
    _fields_ = [("dgamma", c_p * 4), ("dbeta", c_p * 4), ("dw", c_p * 4)]


class ResEncoderDesc(ctypes.Structure):
    """struct kpn_res_encoder_desc"""
    _fields_ = [(n, c_i32) for n in ("N", "H", "W", "in_ch", "ngf", "n_down", "n_blocks", "n_up", "out_ch")] + [("eps", c_f)]


class HgFilterDesc(ctypes.Structure):
    """struct kpn_hg_filter_desc"""
    _fields_ = [(n, c_i32) for n in ("N", "H", "W", "in_ch", "c_stem", "c2", "c3", "c4", "depth", "c_hd", "out_ch_hd", "out_ch")] + [("eps", c_f)]


class HgFilterParams(ctypes.Structure):
    """struct kpn_hg_filter_params"""
    _fields_ = [("tensors", ctypes.POINTER(c_p)), ("packed", c_p)]


class HgFilterGrads(ctypes.Structure):
    """struct kpn_hg_filter_grads"""
    _fields_ = [("tensors", ctypes.POINTER(c_p))]


class ResampleDesc(ctypes.Structure):
    """struct kpn_resample2_desc"""
    _fields_ = [(n, c_i32) for n in ("N", "h", "w", "C")]


# name -> (restype, argtypes); mirrors include/kpnerf.h one to one
_SIGNATURES = {
    "kpn_abi_version": (ctypes.c_int, []),
    "kpn_last_error": (ctypes.c_char_p, []),
    "kpn_is_device_build": (ctypes.c_int, []),
    "kpn_plain_weight_floats": (c_sz, []),
    "kpn_packed_weight_floats": (c_sz, []),
    "kpn_pack_weights": (ctypes.c_int, [c_p, c_p]),
    "kpn_pack_weights_device": (ctypes.c_int, [c_p, c_p, c_p]),
    "kpn_scene_workspace_bytes": (c_sz, [ctypes.POINTER(SceneDesc)]),
    "kpn_scene_prepare": (ctypes.c_int, [ctypes.POINTER(SceneDesc), c_p, c_p]),
    "kpn_scene_layout": (ctypes.c_int, [ctypes.POINTER(SceneDesc), ctypes.POINTER(c_sz)]),
    "kpn_ray_bbox_intersection": (ctypes.c_int, [c_p, c_p, c_p, c_i64, c_p, c_p, c_p, c_p]),
    "kpn_make_rays": (ctypes.c_int, [c_p, c_p, c_f, c_f, c_p, c_i32, c_i32, c_i32, c_i32, c_i32, c_p, c_p, c_p, c_p, c_p]),
    "kpn_importance_sample": (ctypes.c_int, [c_p, c_p, c_p, c_i64, c_i32, c_i32, c_p, c_p]),
    "kpn_rgba2out": (ctypes.c_int, [c_p, c_p, c_i64, c_i32, c_p, c_p, c_p, c_p, c_p, c_p]),
    "kpn_rgba2out_backward": (ctypes.c_int, [c_p, c_p, c_i64, c_i32, c_p, c_p, c_p, c_p, c_p, c_p]),
    "kpn_geo_rows_backward_workspace_bytes": (c_sz, [c_i64, c_i32]),
    "kpn_geo_rows_backward": (ctypes.c_int, [ctypes.POINTER(SceneDesc), c_p, c_p, c_i64, c_p, ctypes.c_uint32, c_p, c_p, c_p,
                                             c_p, c_p, c_sz, c_p]),
    "kpn_query_backward_geometry_workspace_bytes": (c_sz, [c_i64, c_i32]),
    "kpn_query_backward_geometry": (ctypes.c_int, [ctypes.POINTER(SceneDesc), c_p, c_p, c_i64, c_p, c_i32, ctypes.c_uint32, c_p,
                                                   ctypes.c_float, c_p, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "kpn_query_backward_workspace_bytes": (c_sz, [c_i64, c_i32]),
    "kpn_query_backward": (ctypes.c_int, [ctypes.POINTER(SceneDesc), c_p, c_p, c_i64, c_p, c_p, c_i32, ctypes.c_uint32, c_p,
                                          ctypes.c_float, c_p, c_p, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "kpn_render_rays_train_backward_workspace_bytes": (c_sz, [ctypes.POINTER(SceneDesc), ctypes.POINTER(RenderArgs)]),
    "kpn_render_rays_train_backward": (ctypes.c_int, [ctypes.POINTER(SceneDesc), c_p, c_p, ctypes.POINTER(RenderArgs),
                                                      ctypes.POINTER(TrainArgs), ctypes.POINTER(RenderGrads), c_p, c_p, c_p, c_p,
                                                      c_p, c_sz, c_p]),
    # the same calls with d_kpt3d (n_kpt, 3) and n_kpt after the last map gradient (include/kpnerf.h)
    "kpn_geo_rows_backward_workspace_bytes_kpt": (c_sz, [c_i64, c_i32]),
    "kpn_geo_rows_backward_kpt": (ctypes.c_int, [ctypes.POINTER(SceneDesc), c_p, c_p, c_i64, c_p, ctypes.c_uint32, c_p, c_p, c_p,
                                                 c_p, c_p, c_i32, c_p, c_sz, c_p]),
    "kpn_query_backward_workspace_bytes_kpt": (c_sz, [c_i64, c_i32]),
    "kpn_query_backward_kpt": (ctypes.c_int, [ctypes.POINTER(SceneDesc), c_p, c_p, c_i64, c_p, c_p, c_i32, ctypes.c_uint32, c_p,
                                              ctypes.c_float, c_p, c_p, c_p, c_p, c_p, c_p, c_i32, c_p, c_sz, c_p]),
    "kpn_render_rays_train_backward_workspace_bytes_kpt": (c_sz, [ctypes.POINTER(SceneDesc), ctypes.POINTER(RenderArgs)]),
    "kpn_render_rays_train_backward_kpt": (ctypes.c_int, [ctypes.POINTER(SceneDesc), c_p, c_p, ctypes.POINTER(RenderArgs),
                                                          ctypes.POINTER(TrainArgs), ctypes.POINTER(RenderGrads), c_p, c_p, c_p, c_p,
                                                          c_p, c_i32, c_p, c_sz, c_p]),
    "kpn_render_rays_train_backward_kept_kpt": (ctypes.c_int, [ctypes.POINTER(SceneDesc), c_p, c_p, ctypes.POINTER(RenderArgs),
                                                               ctypes.POINTER(TrainArgs), ctypes.POINTER(RenderGrads), c_p, c_p, c_p,
                                                               c_p, c_p, c_i32, c_p, c_sz, c_p, c_sz, c_p]),
    "kpn_set_geo_rows_mode": (ctypes.c_int, [c_i32]),
    "kpn_get_geo_rows_mode": (ctypes.c_int, []),
    "kpn_packed_f16_range_check": (ctypes.c_int, [c_p, c_p, c_p]),
    "kpn_set_fuse_mode": (ctypes.c_int, [c_i32]),
    "kpn_get_fuse_mode": (ctypes.c_int, []),
    "kpn_set_density_first": (ctypes.c_int, [c_i32]),
    "kpn_get_density_first": (ctypes.c_int, []),
    "kpn_density_stats": (ctypes.c_int, [c_p, c_p, c_p, c_i32]),
    "kpn_density_first_passes": (ctypes.c_int, [c_p, c_p, c_i32]),
    "kpn_bwd_profile_enable": (ctypes.c_int, [c_i32]),
    "kpn_bwd_profile_collect": (ctypes.c_int, [c_p, c_p, c_p, c_p, c_p]),
    "kpn_set_range_guard": (ctypes.c_int, [c_i32]),
    "kpn_get_range_guard": (ctypes.c_int, []),
    "kpn_range_guard_count": (ctypes.c_int, [c_p, c_p]),
    "kpn_ssim_scratch_bytes": (c_sz, [c_i32, c_i32]),
    "kpn_ssim": (ctypes.c_int, [c_p, c_p, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_p, c_p, c_p]),
    "kpn_query_workspace_bytes": (c_sz, [c_i64, c_i32]),
    "kpn_query": (ctypes.c_int, [ctypes.POINTER(SceneDesc), c_p, c_p, c_i64, c_p, c_p, c_i32, c_p, c_p, c_p, c_sz, c_p]),
    "kpn_render_workspace_bytes": (c_sz, [ctypes.POINTER(SceneDesc), ctypes.POINTER(RenderArgs)]),
    "kpn_render_rays": (ctypes.c_int, [ctypes.POINTER(SceneDesc), c_p, c_p, ctypes.POINTER(RenderArgs), c_p, c_sz, c_p]),
    "kpn_render_rays_train": (ctypes.c_int, [ctypes.POINTER(SceneDesc), c_p, c_p, ctypes.POINTER(RenderArgs),
                                             ctypes.POINTER(TrainArgs), c_p, c_sz, c_p]),
    "kpn_frame_to_rgb8": (ctypes.c_int, [c_p, c_i32, c_i32, c_i32, c_p, c_p]),
    "kpn_mse_psnr": (ctypes.c_int, [c_p, c_p, c_i64, c_p, c_p, c_p]),
    "kpn_flops_per_point": (ctypes.c_double, [c_i32]),
    "kpn_flops_per_row": (ctypes.c_double, []),
    "kpn_profile_enable": (ctypes.c_int, [c_i32]),
    "kpn_render_rays_train_state_bytes": (c_sz, [ctypes.POINTER(SceneDesc), ctypes.POINTER(RenderArgs)]),
    "kpn_render_rays_train_keep": (ctypes.c_int, [ctypes.POINTER(SceneDesc), c_p, c_p, ctypes.POINTER(RenderArgs),
                                                  ctypes.POINTER(TrainArgs), c_p, c_sz, c_p]),
    "kpn_render_rays_train_backward_kept": (ctypes.c_int, [ctypes.POINTER(SceneDesc), c_p, c_p, ctypes.POINTER(RenderArgs),
                                                           ctypes.POINTER(TrainArgs), ctypes.POINTER(RenderGrads), c_p, c_p, c_p, c_p,
                                                           c_p, c_sz, c_p, c_sz, c_p]),
    "kpn_pix_l1_loss": (ctypes.c_int, [c_p, c_p, ctypes.c_int64, ctypes.c_float, c_p, c_p, c_p, c_p]),
    "kpn_train_loss_workspace_bytes": (c_sz, [c_i64]),
    "kpn_train_loss": (ctypes.c_int, [ctypes.POINTER(TrainLossArgs), c_p, c_p]),
    "kpn_profile_collect": (ctypes.c_int, [c_p, c_p, c_p]),
    "kpn_profile_collect2": (ctypes.c_int, [c_p, c_p, c_p, c_p]),
    "kpn_profile_collect3": (ctypes.c_int, [c_p, c_p, c_p, c_p, c_p]),
    "kpn_row_scratch_cap_bytes": (ctypes.c_size_t, []),
    "kpn_set_row_scratch_cap_bytes": (ctypes.c_int, [ctypes.c_size_t]),
    "kpn_selftest_mfma": (ctypes.c_int, [c_p, c_p, c_p]),
    "kpn_vgg_plain_floats": (c_sz, []),
    "kpn_vgg_packed_floats": (c_sz, []),
    "kpn_vgg_pack_device": (ctypes.c_int, [c_p, c_p, c_p]),
    "kpn_vgg_workspace_bytes": (c_sz, [c_i32, c_i32, c_i32]),
    "kpn_vgg_stage_floats": (c_sz, [c_i32, c_i32, c_i32]),
    "kpn_vgg_loss": (ctypes.c_int, [c_p, c_p, c_i32, c_i32, c_i32, c_p, c_p, c_p, c_p, c_f, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "kpn_geo_encoder_plain_floats": (c_sz, [c_i32, c_i32]),
    "kpn_geo_encoder_packed_floats": (c_sz, [c_i32, c_i32]),
    "kpn_geo_encoder_pack_device": (ctypes.c_int, [c_p, c_p, c_i32, c_i32, c_p]),
    "kpn_geo_encoder_workspace_bytes": (c_sz, [c_i32] * 6),
    "kpn_geo_encoder_stage_floats": (c_sz, [c_i32] * 6),
    "kpn_geo_encoder_stage_info": (ctypes.c_int, [c_i32] * 7 + [ctypes.c_char_p, c_i32, ctypes.POINTER(c_i64), ctypes.POINTER(c_i32)]),
    "kpn_geo_encode": (ctypes.c_int, [c_p] + [c_i32] * 6 + [c_p, c_f, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "kpn_tex_encoder_plain_floats": (c_sz, [c_i32] * 5),
    "kpn_tex_encoder_packed_floats": (c_sz, [c_i32] * 5),
    "kpn_tex_encoder_pack_device": (ctypes.c_int, [c_p, c_p] + [c_i32] * 5 + [c_p]),
    "kpn_tex_encoder_workspace_bytes": (c_sz, [c_i32] * 9),
    "kpn_tex_encoder_stage_floats": (c_sz, [c_i32] * 9),
    "kpn_tex_encoder_stage_info": (ctypes.c_int, [c_i32] * 10 + [ctypes.c_char_p, c_i32, ctypes.POINTER(c_i64), ctypes.POINTER(c_i32)]),
    "kpn_tex_encode": (ctypes.c_int, [c_p] + [c_i32] * 9 + [c_p, c_f, c_p, c_p, c_p, c_sz, c_p]),
    "kpn_fold_norm_floats": (c_sz, []),
    "kpn_fold_params": (ctypes.c_int, [ctypes.POINTER(ParamTable), c_p, c_p, c_p]),
    "kpn_fold_params_backward": (ctypes.c_int, [ctypes.POINTER(ParamTable), c_p, c_p, ctypes.POINTER(ParamTable), c_i32, c_p]),
    "kpn_adam_step": (ctypes.c_int, [ctypes.POINTER(AdamArgs), c_p]),
    "kpn_plain_weight_floats_shape": (c_sz, [ctypes.POINTER(FieldShape)]),
    "kpn_widen_plain": (ctypes.c_int, [ctypes.POINTER(FieldShape), c_p, c_p, c_p]),
    "kpn_narrow_plain_grad": (ctypes.c_int, [ctypes.POINTER(FieldShape), c_p, c_p, c_i32, c_p]),
    "kpn_scene_prepare_kpt": (ctypes.c_int, [ctypes.POINTER(SceneDesc), c_i32, c_p, c_p]),
    "kpn_fold_params_shape": (ctypes.c_int, [ctypes.POINTER(FieldShape), ctypes.POINTER(ParamTable), c_p, c_p, c_p]),
    "kpn_fold_params_backward_shape": (ctypes.c_int, [ctypes.POINTER(FieldShape), ctypes.POINTER(ParamTable), c_p, c_p,
                                                      ctypes.POINTER(ParamTable), c_i32, c_p]),
    "kpn_conv2d_packed_floats": (c_sz, [ctypes.POINTER(Conv2dDesc)]),
    "kpn_conv2d_pack_device": (ctypes.c_int, [ctypes.POINTER(Conv2dDesc), c_p, c_p, c_p]),
    "kpn_conv2d_workspace_bytes": (c_sz, [ctypes.POINTER(Conv2dDesc)]),
    "kpn_conv2d_wgrad_ranges": (c_i32, [ctypes.POINTER(Conv2dDesc)]),
    "kpn_conv2d_forward": (ctypes.c_int, [ctypes.POINTER(Conv2dDesc), c_p, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "kpn_conv2d_backward": (ctypes.c_int, [ctypes.POINTER(Conv2dDesc), c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_sz, c_p]),
    # the same six with the arithmetic (CONV_F32 / CONV_BF16X3) behind the descriptor
    "kpn_conv2d_ex_packed_floats": (c_sz, [ctypes.POINTER(Conv2dDesc), c_i32]),
    "kpn_conv2d_ex_pack_device": (ctypes.c_int, [ctypes.POINTER(Conv2dDesc), c_i32, c_p, c_p, c_p]),
    "kpn_conv2d_ex_workspace_bytes": (c_sz, [ctypes.POINTER(Conv2dDesc), c_i32]),
    "kpn_conv2d_ex_wgrad_ranges": (c_i32, [ctypes.POINTER(Conv2dDesc), c_i32]),
    "kpn_conv2d_ex_forward": (ctypes.c_int, [ctypes.POINTER(Conv2dDesc), c_i32, c_p, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "kpn_conv2d_ex_backward": (ctypes.c_int, [ctypes.POINTER(Conv2dDesc), c_i32, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "kpn_conv2d_s2_packed_floats": (c_sz, [ctypes.POINTER(Conv2dS2Desc)]),
    "kpn_conv2d_s2_pack_device": (ctypes.c_int, [ctypes.POINTER(Conv2dS2Desc), c_p, c_p, c_p]),
    "kpn_conv2d_s2_workspace_bytes": (c_sz, [ctypes.POINTER(Conv2dS2Desc)]),
    "kpn_conv2d_s2_wgrad_ranges": (c_i32, [ctypes.POINTER(Conv2dS2Desc)]),
    "kpn_conv2d_s2_forward": (ctypes.c_int, [ctypes.POINTER(Conv2dS2Desc), c_p, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "kpn_conv2d_s2_backward": (ctypes.c_int, [ctypes.POINTER(Conv2dS2Desc), c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "kpn_conv2d_rp_packed_floats": (c_sz, [ctypes.POINTER(Conv2dRpDesc)]),
    "kpn_conv2d_rp_pack_device": (ctypes.c_int, [ctypes.POINTER(Conv2dRpDesc), c_p, c_p, c_p]),
    "kpn_conv2d_rp_workspace_bytes": (c_sz, [ctypes.POINTER(Conv2dRpDesc)]),
    "kpn_conv2d_rp_wgrad_ranges": (c_i32, [ctypes.POINTER(Conv2dRpDesc)]),
    "kpn_conv2d_rp_forward": (ctypes.c_int, [ctypes.POINTER(Conv2dRpDesc), c_p, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "kpn_conv2d_rp_backward": (ctypes.c_int, [ctypes.POINTER(Conv2dRpDesc), c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "kpn_group_norm_stats_floats": (c_sz, [ctypes.POINTER(GroupNormDesc)]),
    "kpn_group_norm_workspace_bytes": (c_sz, [ctypes.POINTER(GroupNormDesc)]),
    "kpn_group_norm_forward": (ctypes.c_int, [ctypes.POINTER(GroupNormDesc), c_p, c_p, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "kpn_group_norm_backward": (ctypes.c_int, [ctypes.POINTER(GroupNormDesc), c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "kpn_conv_block_workspace_bytes": (c_sz, [ctypes.POINTER(ConvBlockDesc)]),
    "kpn_conv_block_state_floats": (c_sz, [ctypes.POINTER(ConvBlockDesc)]),
    "kpn_conv_block_forward": (ctypes.c_int, [ctypes.POINTER(ConvBlockDesc), c_p, ctypes.POINTER(ConvBlockParams), c_p, c_p, c_p, c_sz, c_p]),
    "kpn_conv_block_backward": (ctypes.c_int, [ctypes.POINTER(ConvBlockDesc), c_p, c_p, ctypes.POINTER(ConvBlockParams), c_p, c_p,
                                               ctypes.POINTER(ConvBlockGrads), c_p, c_sz, c_p]),
    "kpn_conv_block_ex_workspace_bytes": (c_sz, [ctypes.POINTER(ConvBlockDesc), c_i32]),
    "kpn_conv_block_ex_state_floats": (c_sz, [ctypes.POINTER(ConvBlockDesc), c_i32]),
    "kpn_conv_block_ex_forward": (ctypes.c_int, [ctypes.POINTER(ConvBlockDesc), c_i32, c_p, ctypes.POINTER(ConvBlockParams), c_p, c_p, c_p, c_sz,
                                                 c_p]),
    "kpn_conv_block_ex_backward": (ctypes.c_int, [ctypes.POINTER(ConvBlockDesc), c_i32, c_p, c_p, ctypes.POINTER(ConvBlockParams), c_p, c_p,
                                                  ctypes.POINTER(ConvBlockGrads), c_p, c_sz, c_p]),
    "kpn_res_encoder_layers": (c_i32, [ctypes.POINTER(ResEncoderDesc)]),
    "kpn_res_encoder_workspace_bytes": (c_sz, [ctypes.POINTER(ResEncoderDesc)]),
    "kpn_res_encoder_state_floats": (c_sz, [ctypes.POINTER(ResEncoderDesc)]),
    "kpn_res_encoder_packed_floats": (c_sz, [ctypes.POINTER(ResEncoderDesc)]),
    "kpn_res_encoder_pack_device": (ctypes.c_int, [ctypes.POINTER(ResEncoderDesc), ctypes.POINTER(c_p), c_p, c_p]),
    "kpn_res_encoder_forward": (ctypes.c_int, [ctypes.POINTER(ResEncoderDesc), c_p, c_p, ctypes.POINTER(c_p), c_p, c_p, c_p, c_sz, c_p]),
    "kpn_res_encoder_backward": (ctypes.c_int, [ctypes.POINTER(ResEncoderDesc), c_p, c_p, c_p, c_p, ctypes.POINTER(c_p), ctypes.POINTER(c_p),
                                                c_p, c_sz, c_p]),
    "kpn_hg_filter_tensors": (c_i32, [ctypes.POINTER(HgFilterDesc)]),
    "kpn_hg_filter_workspace_bytes": (c_sz, [ctypes.POINTER(HgFilterDesc)]),
    "kpn_hg_filter_state_floats": (c_sz, [ctypes.POINTER(HgFilterDesc)]),
    "kpn_hg_filter_packed_floats": (c_sz, [ctypes.POINTER(HgFilterDesc)]),
    "kpn_hg_filter_pack_device": (ctypes.c_int, [ctypes.POINTER(HgFilterDesc), ctypes.POINTER(c_p), c_p, c_p]),
    "kpn_hg_filter_forward": (ctypes.c_int, [ctypes.POINTER(HgFilterDesc), c_p, ctypes.POINTER(HgFilterParams), c_p, c_p, c_p, c_p, c_sz, c_p]),
    "kpn_hg_filter_backward": (ctypes.c_int, [ctypes.POINTER(HgFilterDesc), c_p, c_p, c_p, ctypes.POINTER(HgFilterParams), c_p,
                                              ctypes.POINTER(HgFilterGrads), c_p, c_sz, c_p]),
    "kpn_avg_pool2_forward": (ctypes.c_int, [ctypes.POINTER(ResampleDesc), c_p, c_p, c_p]),
    "kpn_avg_pool2_backward": (ctypes.c_int, [ctypes.POINTER(ResampleDesc), c_p, c_p, c_p]),
    "kpn_upsample2x_add_forward": (ctypes.c_int, [ctypes.POINTER(ResampleDesc), c_p, c_p, c_p, c_p]),
    "kpn_upsample2x_add_backward": (ctypes.c_int, [ctypes.POINTER(ResampleDesc), c_p, c_p, c_p]),
}
ABI_VERSION = 10


class KpnError(RuntimeError):
    pass


class KpnLibrary:
    def __init__(self, path):
        if not os.path.isfile(path):
            raise KpnError(
                f"{path} not found: the HIP library has not been built. Run `python build.py` "
                f"(hipcc --offload-arch=gfx950). There is no CPU fallback for this path.")
        self.path = path
        self.cdll = ctypes.CDLL(path)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(self.cdll, name)  # AttributeError if the symbol is missing
            fn.restype = res
            fn.argtypes = args
            setattr(self, name, fn)
        v = self.kpn_abi_version()
        if v != ABI_VERSION:
            raise KpnError(f"{path}: ABI version {v}, binding expects {ABI_VERSION}")

    def check(self, code):
        if code != 0:
            raise KpnError(f"kpnerf error {code}: {self.kpn_last_error().decode()}")

    def exported_symbols(self):
        return sorted(_SIGNATURES)


_default = None


def get_library():
    """The gfx950 product library; raises KpnError if it is not built (no fallback)."""
    global _default
    if _default is None:
        lib = KpnLibrary(DEFAULT_LIB)
        if not lib.kpn_is_device_build():
            raise KpnError(f"{DEFAULT_LIB} is not a device build")
        _default = lib
    return _default

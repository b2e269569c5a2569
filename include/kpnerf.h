/*
 * kpnerf.h — C ABI of libkpnerf_hip.so, the MI355X (gfx950) ray-march library behind
 * KeypointNeRF's render path.
 *
 * The reference (facebookresearch/KeypointNeRF, pure Python) has no FFI/plugin interface; the seam
 * for this path is attribute lookup on its `net` object.  Each entry point below
 * replaces one of those Python callables and cites it (file:line under the reference repo).
 * The binding a maintainer would add on the reference side is a ctypes stub — see INTEGRATION.md
 * and keypointnerf_amd/lib.py, which is exactly that stub.
 *
 * Conventions
 *   - every pointer is DEVICE memory unless its name ends in `_host`;
 *   - all arithmetic is fp32 (the reference sets torch default dtype float32, train.py:16);
 *     index/compaction lists are int32; masks are uint8 (0/1);
 *   - `stream` is a hipStream_t passed as void*; calls are asynchronous on it, never synchronise,
 *     never allocate;
 *   - inputs are never written; outputs and `workspace` are caller-allocated;
 *   - every function returns 0 on success, a negative KPN_E* code otherwise; kpn_last_error()
 *     gives the message (thread-local).  Nothing returns NaN silently for valid inputs.
 */
#ifndef KPNERF_H
#define KPNERF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 3 (round 6): kpn_render_args gained `stages` at its end (callers built against 2 must be rebuilt: the struct grew);
 * new entry points: kpn_set_density_first / kpn_get_density_first / kpn_density_stats / kpn_density_first_passes, kpn_bwd_profile_* */
/* 4: additive - the perceptual term of the training loss: kpn_vgg_plain_floats / kpn_vgg_packed_floats / kpn_vgg_pack_device,
 * kpn_vgg_workspace_bytes / kpn_vgg_stage_floats, kpn_vgg_loss (nothing of ABI 3 changed) */
/* 5: additive - forward of the two image encoders: kpn_geo_encoder_* / kpn_geo_encode (HGFilterV2), kpn_tex_encoder_* /
 * kpn_tex_encode (ResBlkEncoder) (nothing of ABI 4 changed) */
/* 6: additive - every pixel and mask term of the training loss in one launch: kpn_train_loss_args, kpn_train_loss_workspace_bytes,
 * kpn_train_loss (nothing of ABI 5 changed; kpn_pix_l1_loss stays) */
/* 7: additive - the parameter leg of a training step: kpn_param_table, kpn_fold_params, kpn_fold_params_backward, kpn_fold_norm_floats,
 * kpn_adam_segment, kpn_adam_args, kpn_adam_step (nothing of ABI 6 changed) */
/* 8: additive - one stride-1 convolution with its three gradients: kpn_conv2d_desc, kpn_conv2d_packed_floats, kpn_conv2d_pack_device,
 * kpn_conv2d_workspace_bytes, kpn_conv2d_wgrad_ranges, kpn_conv2d_forward, kpn_conv2d_backward (nothing of ABI 7 changed) */
/* 9: additive - GroupNorm / InstanceNorm2d [+ ReLU] with its gradients: kpn_group_norm_desc, kpn_group_norm_stats_floats,
 * kpn_group_norm_workspace_bytes, kpn_group_norm_forward, kpn_group_norm_backward (nothing of ABI 8 changed) */
/* 10: additive - the two resampling steps of an HourGlass with their gradients: kpn_resample2_desc, kpn_avg_pool2_forward,
 * kpn_avg_pool2_backward, kpn_upsample2x_add_forward, kpn_upsample2x_add_backward (nothing of ABI 9 changed) */
/* still 10: kpn_scene_layout (where kpn_scene_prepare puts each prepared map in the scene workspace) is one more export and changes
 * nothing that a caller built against 10 uses, so the number stays; a binding that wants it looks the symbol up */
/* still 10: the stride-2, stem and transposed convolutions with their gradients (kpn_conv2d_s2_desc, kpn_conv2d_s2_packed_floats,
 * kpn_conv2d_s2_pack_device, kpn_conv2d_s2_workspace_bytes, kpn_conv2d_s2_wgrad_ranges, kpn_conv2d_s2_forward, kpn_conv2d_s2_backward)
 * are additive within 10: nothing that a caller built against 10 uses changed, kpn_conv2d_* and its refusals included */
/* still 10: the replication-padded stride-1 convolutions with their gradients (kpn_conv2d_rp_desc, kpn_conv2d_rp_packed_floats,
 * kpn_conv2d_rp_pack_device, kpn_conv2d_rp_workspace_bytes, kpn_conv2d_rp_wgrad_ranges, kpn_conv2d_rp_forward, kpn_conv2d_rp_backward)
 * are additive within 10 in the same way */
/* still 10: a whole ConvBlock as one differentiable operator (kpn_conv_block_desc, kpn_conv_block_params, kpn_conv_block_grads,
 * kpn_conv_block_workspace_bytes, kpn_conv_block_state_floats, kpn_conv_block_forward, kpn_conv_block_backward) is additive within 10
 * in the same way */
/* still 10: a whole ResBlkEncoder as one differentiable operator (kpn_res_encoder_desc, kpn_res_encoder_layers,
 * kpn_res_encoder_workspace_bytes, kpn_res_encoder_state_floats, kpn_res_encoder_packed_floats, kpn_res_encoder_pack_device,
 * kpn_res_encoder_forward, kpn_res_encoder_backward) is additive within 10 in the same way */
/* still 10: the arithmetic selector of the stride-1 convolution and the ConvBlock (KPN_CONV_F32 / KPN_CONV_BF16X3, kpn_conv2d_ex_*,
 * kpn_conv_block_ex_*) is additive within 10 in the same way: kpn_conv2d_* and kpn_conv_block_* are its arith = KPN_CONV_F32 case */
/* still 10: a whole HGFilterV2 as one differentiable operator (kpn_hg_filter_desc, kpn_hg_filter_params, kpn_hg_filter_grads,
 * kpn_hg_filter_tensors, kpn_hg_filter_workspace_bytes, kpn_hg_filter_state_floats, kpn_hg_filter_packed_floats,
 * kpn_hg_filter_pack_device, kpn_hg_filter_forward, kpn_hg_filter_backward) is additive within 10 in the same way */
/* still 10: keypoint sets - models with 1..24 keypoints and 0..3 encoding octaves served as the 24 / 3 model (kpn_field_shape,
 * kpn_plain_weight_floats_shape, kpn_widen_plain, kpn_narrow_plain_grad, kpn_scene_prepare_kpt, kpn_fold_params_shape,
 * kpn_fold_params_backward_shape) are additive within 10 in the same way */
#define KPN_ABI_VERSION 10
#define KPN_N_KPT 24      /* configs/zju.json:44 sp_args.n_kpt: the CAPACITY of the field kernels (models with fewer keypoints: "Keypoint sets" below) */
#define KPN_MAX_VIEWS 16

enum { KPN_OK = 0, KPN_EINVAL = -1, KPN_ELAUNCH = -2, KPN_EWORKSPACE = -3 };

int kpn_abi_version(void);
const char* kpn_last_error(void);
/* 1 if the library was built for the device (gfx950), 0 for the host SIMT emulator build (tests only) */
int kpn_is_device_build(void);

/* ---------------------------------------------------------------------------------------------
 * Parameters.  `plain_host`: the weight-norm-folded hot-path parameters as one flat fp32 vector in
 * the order of keypointnerf_amd/synthetic.py:HOTPATH_LAYERS (W row-major (out,in) then bias per
 * layer, raw ani_al last) — i.e. the reference modules mlp_geo (src/utils.py:476-517),
 * ibr_compress_gfeat (src/model.py:577-580) and mlp_tex (src/model.py:1239-1258).
 * kpn_pack_weights re-orders them into the MFMA A-operand streams the kernels read. */
size_t kpn_plain_weight_floats(void);
size_t kpn_packed_weight_floats(void);
int kpn_pack_weights(const float* plain_host, float* packed_host);
/* The same re-ordering on the device (plain_dev -> packed_dev, both device pointers, asynchronous on `stream`): a
 * training loop re-packs after every optimizer step without a host round trip.  The index map is taken once per
 * process from kpn_pack_weights. */
int kpn_pack_weights_device(const float* plain_dev, float* packed_dev, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Scene = what KeypointNeRF.query() receives besides the points: source cameras, keypoints, source
 * images, fg masks and the encoder feature maps in NCHW, as the reference hands them over
 * (src/model.py:690-701, 336-355, 653-680). */
typedef struct kpn_scene_desc {
    int32_t n_views;                 /* V  (<= KPN_MAX_VIEWS) */
    int32_t src_h, src_w;            /* source image size H, W (cam["height"], cam["width"]) */
    int32_t geo0_h, geo0_w;          /* feat_geo[0]: (V,64,geo0_h,geo0_w) */
    int32_t geo1_h, geo1_w;          /* feat_geo[1]: (V, 8,geo1_h,geo1_w) */
    int32_t tex_h, tex_w;            /* feat_tex   : (V, 8,tex_h,tex_w)   */
    int32_t disable_fg_mask;         /* KeypointNeRF.disable_fg_mask, src/model.py:566,734 */
    float znear, zfar;               /* cam["znear"], cam["zfar"] (2.0/5.0, src/model.py:43,345) */
    float nml_scale;                 /* cam["nml_scale"] (100.0) */
    float sigma;                     /* sp_args.sigma (0.1) */
    const float* KRT;                /* (V,4,4) */
    const float* extrin;             /* (V,4,4) */
    const float* kpt3d;              /* (24,3); (n_kpt,3) for kpn_scene_prepare_kpt */
    const float* img;                /* (V,3,H,W) */
    const uint8_t* fg_mask;          /* (V,H,W) bool bytes; ignored if disable_fg_mask */
    const float* geo0;
    const float* geo1;
    const float* tex;
} kpn_scene_desc;

/* bytes of device workspace that kpn_scene_prepare fills (channels-last maps + per-view tables) */
size_t kpn_scene_workspace_bytes(const kpn_scene_desc* desc);
/* Builds the kernel-side scene: NCHW -> channels-last (one 256-B line per 64-channel tap), RGB+mask
 * interleaved, keypoints moved to every camera frame (src/spatial.py:85), source camera centres
 * (inverse(KRT)[:3,3], src/model.py:823-824). */
int kpn_scene_prepare(const kpn_scene_desc* desc, void* scene_ws, void* stream);
/* Where kpn_scene_prepare puts its results: the offsets, in floats from the start of the workspace, of the per-view tables
 * (V x 112), rgbm (V,H,W,4), geo0 (V,h,w,64), geo1 (V,h,w,8), tex (V,h,w,8) and the flags ([0] = max |value| of the
 * images and maps, as a float; a NaN input makes it NaN), in this order.  For tests and tools that read the prepared maps. */
int kpn_scene_layout(const kpn_scene_desc* desc, size_t offsets[6]);

/* ---------------------------------------------------------------------------------------------
 * Stage ops = the reference's per-stage callables. */

/* KeypointNeRF.ray_bbox_intersection, src/model.py:1178-1237.
 * bounds (2,3), orig (3), direct (R,3) -> near (R), far (R), hit (R). */
int kpn_ray_bbox_intersection(const float* bounds, const float* orig, const float* direct, int64_t n_rays,
                              float* near_out, float* far_out, uint8_t* hit_out, void* stream);

/* Ray set-up of batch_render_pifu_nerf, src/model.py:1019-1043, for the pixel grid
 * px = x0 + ix*step, py = y0 + iy*step (ix<nx, iy<ny; ray index = iy*nx + ix; eval branch :1019-1022
 * has step = 2^(level-1), (x0,y0) = stride offset (j,i)).  K,RT: target camera (4,4).
 * -> dirs (R,3), cam_pos (3), near (R), far (R) after the AABB clip. */
int kpn_make_rays(const float* K, const float* RT, float znear, float zfar, const float* bounds, int32_t x0,
                  int32_t y0, int32_t step, int32_t nx, int32_t ny, float* dirs, float* cam_pos, float* near_out,
                  float* far_out, void* stream);

/* KeypointNeRF.importance_sample, src/model.py:1110-1148.  contrib (R,D-2), z (R,D-1),
 * u (R,n) or NULL (uniform=True -> linspace(0,1,n)) -> samples (R,n). */
int kpn_importance_sample(const float* contrib, const float* z, const float* u, int64_t n_rays, int32_t d_minus_2,
                          int32_t n_samples, float* samples_out, void* stream);

/* KeypointNeRF.rgba2out, src/model.py:1150-1176.  rgba (R,S,5) [sigma,sdf,r,g,b], z (R,S) ->
 * color (R,3), depth (R), alpha (R), contrib (R,S) (may be NULL), sdf (R). */
int kpn_rgba2out(const float* rgba, const float* z, int64_t n_rays, int32_t n_samples, float* color, float* depth,
                 float* alpha, float* contrib, float* sdf, void* stream);

/* Backward of rgba2out (what torch autograd derives from src/model.py:1162-1174): given the forward inputs and the
 * upstream gradients of color (R,3), depth (R), alpha (R), sdf (R) (any may be NULL = zero), writes d_rgba (R,S,5).
 * z carries no gradient in the reference (sample positions are drawn under no_grad, :1038,1118).  The compositor piece of
 * the training backward; kpn_render_rays_train_backward chains it with the field reverse. */
int kpn_rgba2out_backward(const float* rgba, const float* z, int64_t n_rays, int32_t n_samples, const float* d_color,
                          const float* d_depth, const float* d_alpha, const float* d_sdf, float* d_rgba, void* stream);

/* Backward of the per-(point, source view) geometry rows: MLPUNet.layers1 232->128->128->(+8)120->64
 * (src/utils.py:691-716) and the bilinear gathers of feat_geo[0] / feat_geo[1] that feed it (src/model.py:763-765,
 * src/utils.py:74-89) — what autograd does for ~70 % of the field's arithmetic in `training_step`
 * (src/model.py:128-155).  The forward activations are recomputed (nothing is kept from the forward pass).
 *   pts (N,3); keep_mask = the train-time view dropout bits (bit v = 0: view v off, as in kpn_train_args);
 *   d_x (N, V, 64): d loss / d (layers1 output of point n in view v); rows of points that are masked
 *        (query's validity, src/model.py:725-739) are ignored;
 *   d_plain: += gradient w.r.t. the weight-norm-folded parameters, same flat layout as kpn_pack_weights' input
 *        (kpn_plain_weight_floats() floats; only the four layers1 blocks are touched);
 *   d_geo0 (V, geo0_h, geo0_w, 64), d_geo1 (V, geo1_h, geo1_w, 8): += gradient w.r.t. the feature maps,
 *        CHANNELS-LAST (permute to NCHW to hand it to the encoder's backward).
 * Accumulating: the caller zeroes the three outputs.  Float atomics: the summation order is not deterministic.
 * The layers1 piece of the training backward; pooling / layers2 / colour head: kpn_query_backward. */
size_t kpn_geo_rows_backward_workspace_bytes(int64_t n_points, int32_t n_views);
int kpn_geo_rows_backward(const kpn_scene_desc* desc, const void* scene_ws, const float* packed_weights, int64_t n_points,
                          const float* pts, uint32_t keep_mask, const float* d_x, float* d_plain, float* d_geo0,
                          float* d_geo1, void* workspace, size_t workspace_bytes, void* stream);

/* Backward of the field evaluation w.r.t. its two GEOMETRY outputs: query()'s [sdf_raw, rad] (mode 0) or eval_func's
 * [sigma = mask*relu(rad + noise), sdf] (mode 1, src/model.py:981-996) — i.e. loss.backward() of training_step
 * (src/model.py:128-155) through view pooling, MLPUNetFusion.layers2 (src/utils.py:500-518, 612-647, 722-748), and
 * then layers1 + the feat_geo gathers as kpn_geo_rows_backward.  d_out (N,5): columns 0,1 are used; the colour
 * columns 2..4 are ignored by THIS entry point (kpn_query_backward propagates all five).
 * Masked points contribute nothing in mode 1 (mask = 0); in mode 0 their constant layers2(0) output is not
 * differentiated either (training uses mode 1).  noise (N) / noise_std: the density noise added before the relu.
 * Outputs accumulate like kpn_geo_rows_backward's (d_plain: layers1 and layers2 blocks). */
size_t kpn_query_backward_geometry_workspace_bytes(int64_t n_points, int32_t n_views);
int kpn_query_backward_geometry(const kpn_scene_desc* desc, const void* scene_ws, const float* packed_weights,
                                int64_t n_points, const float* pts, int32_t mode, uint32_t keep_mask, const float* noise,
                                float noise_std, const float* d_out, float* d_plain, float* d_geo0, float* d_geo1,
                                void* workspace, size_t workspace_bytes, void* stream);

/* Backward of the WHOLE field evaluation, colour head included: everything above plus
 * ibr_compress_gfeat, IBRRenderingHead (src/model.py:784-843, 1267-1302: ray_encoder, the ani_al blend weights,
 * weighted mean/var over views, base / vis / out layers, softmax blend of the source colours) and the feat_tex gather.
 * view (N,3): the query rays' directions.  d_out (N,5): all five columns are propagated.
 * d_plain: += all hot-path parameters incl. the raw ani_al (last entry); d_tex (V, tex_h, tex_w, 8) channels-last, +=. */
size_t kpn_query_backward_workspace_bytes(int64_t n_points, int32_t n_views);
int kpn_query_backward(const kpn_scene_desc* desc, const void* scene_ws, const float* packed_weights, int64_t n_points,
                       const float* pts, const float* view, int32_t mode, uint32_t keep_mask, const float* noise,
                       float noise_std, const float* d_out, float* d_plain, float* d_geo0, float* d_geo1, float* d_tex,
                       void* workspace, size_t workspace_bytes, void* stream);

/* The same backward calls with one more output, the gradient with respect to the 3D KEYPOINTS (sp_data["kpt3d"]): what autograd
 * does for SpatialEncoder.forward's rel_z_decay branch (src/spatial.py:76-118), where the keypoints enter the encoding through
 * kptxyz = kpt3d R^T + t, dz and the decay weight w.  Everything else (arguments, outputs, accumulation) is the call without the
 * suffix.
 *   d_kpt3d (n_kpt, 3): += d loss / d kpt3d, summed over the kept (point, view) rows; only the first n_kpt rows are written
 *        (n_kpt = the keypoints the scene was prepared with, 1..KPN_N_KPT: kpn_scene_prepare_kpt; 24 after kpn_scene_prepare).
 *        Accumulating like the other outputs: the caller zeroes it.  fp64 sums in a fixed order, no float atomics: reproducible
 *        for a given order of the valid list.
 *   workspace: the matching *_workspace_bytes_kpt (the plain size plus the transposed encoding operand of layers1.0 and the
 *        fp64 partial sums).
 * Rows of views dropped by keep_mask and rows of masked points contribute exactly nothing and are never read.  No gradient reaches
 * the query points, the cameras or sigma through these entries. */
size_t kpn_geo_rows_backward_workspace_bytes_kpt(int64_t n_points, int32_t n_views);
int kpn_geo_rows_backward_kpt(const kpn_scene_desc* desc, const void* scene_ws, const float* packed_weights, int64_t n_points,
                              const float* pts, uint32_t keep_mask, const float* d_x, float* d_plain, float* d_geo0,
                              float* d_geo1, float* d_kpt3d, int32_t n_kpt, void* workspace, size_t workspace_bytes, void* stream);
size_t kpn_query_backward_workspace_bytes_kpt(int64_t n_points, int32_t n_views);
int kpn_query_backward_kpt(const kpn_scene_desc* desc, const void* scene_ws, const float* packed_weights, int64_t n_points,
                           const float* pts, const float* view, int32_t mode, uint32_t keep_mask, const float* noise,
                           float noise_std, const float* d_out, float* d_plain, float* d_geo0, float* d_geo1, float* d_tex,
                           float* d_kpt3d, int32_t n_kpt, void* workspace, size_t workspace_bytes, void* stream);

/* Rows kernel of the dominant stage (MLPUNet.layers1 per (point, view) row, reference src/utils.py:691-720), all with
 * fp32 accumulation and the same parity bar against the reference goldens:
 *   3 = v_mfma_f32_32x32x16_f16 with every fp32 operand carried as two fp16 pieces (x - fp16(x) is formed exactly by one
 *       v_fma_mix_f32) and three products per term set (hh hl lh: every term above 2^-24 relative); two 32-point tiles per
 *       wavefront, one wavefront per SIMD
 *       (k_geo_rows_f2).  The default.  Operands must stay within fp16's range (a pre-activation beyond 454 in natural units,
 *       a packed weight or a feature-map value beyond 65504 is not representable): the RANGE GUARD below sees to that.
 *   2 = v_mfma_f32_32x32x16_bf16, three bf16 pieces, six products (k_geo_rows_h2): the same structure in fp32's exponent range.
 *   0 = v_mfma_f32_32x32x2_f32 (fp32 operands, k_geo_rows).
 *   (1, an earlier one-tile-per-wavefront kernel, is refused: not part of the shipped library.)
 * Process-wide, default 3; one call may select another kernel through kpn_render_args.rows_kernel (no environment variable:
 * removed in round 5 — one selection mechanism). */
int kpn_set_geo_rows_mode(int32_t mode);
int kpn_get_geo_rows_mode(void);
/* The per-point kernel (MLPUNet.layers2 + ibr_compress_gfeat + IBRRenderingHead, reference src/utils.py:577-587,
 * src/model.py:819,1267-1302): 1 = weights as two fp16 pieces per value, three products (hh lh hl) on v_mfma_f32_32x32x16_f16
 * (k_fuse_color_h, the default: fp32-class results at less than a fifth of the matrix time); 0 = fp32 weights on
 * v_mfma_f32_32x32x2_f32 (k_fuse_color).  Process-wide, default 1; per call: kpn_render_args.fuse_kernel.  With V = 3 and no view
 * dropped mode 1 launches k_fuse_color_h3 (the same arithmetic, the loops over the views unrolled). */
int kpn_set_fuse_mode(int32_t mode);
int kpn_get_fuse_mode(void);
/* DENSITY FIRST (round 6) — reference src/model.py:981-996 (eval_func: sigma = relu(rad)) and :1150-1176 (rgba2out: a sample's
 * weight is T * (1 - exp(-sigma * delta))): a sample with relu(rad) == 0 contributes EXACTLY 0 to every output, whatever its colour.
 * The render passes (kpn_render_rays; fuse mode 1 on the pooled scratch layout, i.e. the defaults) can therefore evaluate the
 * per-point part in two passes per batch: k_density_h (pooled vector -> layers2 -> density, the compress layer, and a compact list
 * of the points with !(rad <= 0)), then k_row_records_live + k_colour_h / k_colour_h3 (gather records and the V-view colour head
 * for the listed points only).  Per point the arithmetic is the fused kernel's: frames are bit-identical either way.
 *   mode 0: never (the fused per-point kernel, whose short path needs a whole 32-point tile dead);
 *   mode 1: always;
 *   mode 2: auto, the default: per render pass, from the dead fraction the earlier passes measured on the device (>= 20 %: density
 *           first; the pair is 0.16 ms per launch slower than the fused kernel when every point is live and 3 % of a frame faster
 *           when 82 % are dead; no host synchronisation: DESIGN.md).
 * kpn_query, the train branch and the fp32-range kernels behind the range guard always use the fused kernel.  Process-wide;
 * KPN_DENSITY_FIRST=0/1/2 sets the initial value. */
int kpn_set_density_first(int32_t mode);
int kpn_get_density_first(void);
/* How many render passes (coarse / fine pass of a kpn_render_rays call) ran density first and how many on the fused kernel since
 * the library was loaded or the counts were reset (host-side counts; which form mode 2 chose). */
int kpn_density_first_passes(int64_t* density_first, int64_t* fused, int32_t reset);
/* Measurement hook: *listed = the points whose density the per-point kernels of the render passes decided on since the last reset
 * (every point inside the visual hull that was sent to the MLPs), *live = those with !(rad <= 0), i.e. the points whose colour can
 * reach the image; 1 - live / listed is the zero-density fraction bench.py reports.  Counted on the device (one addition per
 * wavefront), read here: synchronises `stream`.  reset != 0 clears the counters. */
int kpn_density_stats(void* stream, int64_t* listed, int64_t* live, int32_t reset);
/* *beyond = number of packed weights that fp16 cannot hold (0 = rows mode 3 / fuse mode 1 run on these weights; otherwise the
 * range guard routes every pass to the fp32-range kernels).  Reads four floats back from the device and synchronises `stream`. */
int kpn_packed_f16_range_check(const float* packed_weights_dev, void* stream, int32_t* beyond);
/* RANGE GUARD of the two-fp16-piece kernels (rows mode 3, fuse mode 1) — on by default, no host synchronisation involved:
 *   - what is known before a pass is tested ON THE DEVICE by the kernels themselves: the packers' count of weights beyond fp16's
 *     range (above) and max |value| of the source images / feature maps, which kpn_scene_prepare records in the scene workspace;
 *     when either is out of range the fp16 kernels return at once and the fp32-range kernels (rows mode 2, fuse mode 0),
 *     launched behind them for every batch of rows, do the work;
 *   - activations cannot be known before: an operand beyond fp16's range turns every accumulator it touches into a NaN, no
 *     activation of these kernels turns a NaN back into a number, and the per-point kernel flags a batch in which a point's
 *     [sdf, rad, rgb] is not finite; the fp32-range kernels then evaluate that batch again.
 * Results are never NaN where the reference's are finite.  The cost when nothing is out of range: two launches per batch that
 * return at once.  kpn_set_range_guard(0) (or the environment variable KPN_NO_RANGE_GUARD=1) switches it off for timing
 * comparisons.  kpn_range_guard_count: number of batches the fp32-range kernels evaluated again on the current device since
 * the library was loaded (0 = everything ran on the fp16 kernels); synchronises `stream`. */
int kpn_set_range_guard(int32_t on);
int kpn_get_range_guard(void);
int kpn_range_guard_count(void* stream, int64_t* batches_host);

/* KeypointNeRF.query (+ query_color + IBRRenderingHead), src/model.py:690-843,1239-1302, eval mode.
 * pts (N,3), view (N,3) -> out (N,5), valid (N).
 * mode 0: out = [sdf_raw, rad, r,g,b] exactly as query() returns;
 * mode 1: out = eval_func(query()) = [mask*relu(rad), mask*sdf+(1-mask)*0.1/nml_scale, r,g,b]
 *         (src/model.py:978-997, rand_noise_std = 0).
 * workspace: kpn_query_workspace_bytes(N, V) bytes. */
size_t kpn_query_workspace_bytes(int64_t n_points, int32_t n_views);
int kpn_query(const kpn_scene_desc* desc, const void* scene_ws, const float* packed_weights, int64_t n_points,
              const float* pts, const float* view, int32_t mode, float* out, uint8_t* valid, void* workspace,
              size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Whole path: KeypointNeRF.batch_render_pifu_nerf, eval branch (src/model.py:942-1108), and — with
 * step=1 over the full image — render_pifu_nerf's tile loop + pixel_shuffle (src/model.py:897-940),
 * which visits exactly the same rays.  Outputs are planar like the reference's out dict (B=1):
 * tex_fg (3,ny,nx), depth (ny,nx), alpha (ny,nx), and if fine: tex_fg_fine, depth_fine, alpha_fine,
 * sdf.  Any output pointer may be NULL. */
/* Optional per-sample outputs of a render call, in ray order (ray = iy * nx + ix) — what the reference holds in z_vals / raw
 * between its stages (src/model.py:1058-1085): the depths and eval_func'ed field values [sigma, sdf, r, g, b] of the coarse pass
 * and of the merged, sorted fine pass.  For the CONDITIONAL parity check of tests/parity_gate.py (each stage of the oracle run on
 * the kernel's own inputs); any pointer may be NULL.  rgb of a sample with sigma == 0 is unspecified (never composited). */
typedef struct kpn_render_stages {
    float* z_coarse;       /* (R, n_coarse) */
    float* rgba_coarse;    /* (R, n_coarse, 5) */
    float* z_fine;         /* (R, n_coarse + n_fine) */
    float* rgba_fine;      /* (R, n_coarse + n_fine, 5) */
    float* dirs;           /* (R, 3) the rays' unit directions and */
    float* cam_pos;        /* (3) their common origin, as the call's ray set-up formed them (src/model.py:1019-1043) */
} kpn_render_stages;
typedef struct kpn_render_args {
    const float* K;          /* cam_tar["K"]  (4,4) */
    const float* RT;         /* cam_tar["RT"] (4,4) */
    const float* bounds;     /* (2,3) */
    float znear, zfar;       /* cam_tar znear/zfar */
    int32_t x0, y0, step, nx, ny;
    int32_t n_coarse, n_fine;   /* sample_per_ray_c / _f */
    int32_t fine;               /* dr_kwargs.fine */
    int32_t chunk_rays;         /* rays per internal pass (0 = default) */
    float* tex_fg; float* depth; float* alpha;
    float* tex_fg_fine; float* depth_fine; float* alpha_fine; float* sdf;
    int32_t step_y;             /* 0: rows advance by `step` like the columns (the reference's grids); > 0: py = y0 + iy*step_y —
                                 * one frame's rows dealt round-robin to the ranks of a render job (rank r of W: y0 = r,
                                 * step_y = W), SURVEY 8(e) */
    int32_t rows_kernel;        /* KPN_ROWS_*: the rows kernel of THIS call; 0 = the process-wide selection (kpn_set_geo_rows_mode) */
    int32_t fuse_kernel;        /* KPN_FUSE_*: the per-point kernel of THIS call; 0 = the process-wide selection (kpn_set_fuse_mode).
                                 * kpn_render_rays only: the kpn_render_rays_train* entry points (forward, kept state, backward
                                 * recompute must run the same kernels) refuse a non-zero selection with KPN_EINVAL */
    const kpn_render_stages* stages;   /* NULL (the default): nothing but the images leaves the call (ABI 3) */
} kpn_render_args;
/* per-call kernel selection (kpn_render_args): the same kernels as kpn_set_geo_rows_mode(0 / 2 / 3) and kpn_set_fuse_mode(0 / 1) */
enum { KPN_ROWS_DEFAULT = 0, KPN_ROWS_F32 = 1, KPN_ROWS_BF16X3 = 2, KPN_ROWS_F16X2 = 3 };
enum { KPN_FUSE_DEFAULT = 0, KPN_FUSE_F32 = 1, KPN_FUSE_F16X2 = 2 };

/* Note on the fine pass: z_fine = sort(cat(z_coarse, z_new)) (src/model.py:1076) repeats the coarse samples; their field
 * values are taken from the coarse pass and the field is evaluated at the new samples only — identical points, identical
 * deterministic values, outputs bit-identical to evaluating all of them again (environment variable
 * KPN_NO_COARSE_REUSE=1 does that, for comparison).  kpn_render_rays_train evaluates everything (fresh dropout / noise). */
size_t kpn_render_workspace_bytes(const kpn_scene_desc* desc, const kpn_render_args* args);
int kpn_render_rays(const kpn_scene_desc* desc, const void* scene_ws, const float* packed_weights,
                    const kpn_render_args* args, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * SURVEY.md §8(f) "next" rows on the output side of the path (callers of the renderer).
 *
 * kpn_frame_to_rgb8: KeypointNeRFLightningModule._arrange_nerf_images (src/model.py:427-430: clamp to [0,1],
 * CHW -> HWC) + the uint8 quantisation `(img*255.).astype(np.uint8)` of render_novel_views / save_test_image
 * (src/model.py:496,504,281) + the channel flip handed to cv2.imwrite (`[:, :, ::-1]`, src/model.py:222,283).
 * chw (3,H,W) fp32 -> hwc_out (H,W,3) uint8; bgr != 0 writes B,G,R.  Integer result is bit-exact.
 *
 * kpn_mse_psnr: ZJUEvaluator.compute_score's mse / _compute_psnr (src/zju_evaluator.py:16-19,63-64):
 * mse = mean((pred-gt)^2) over all n elements, psnr = -10 ln(mse)/ln(10).  out2 (device, 2 doubles) = [mse, psnr];
 * partial sums are accumulated in fp64.  scratch: 2048 doubles + 1 int (device, 16,392 bytes).
 *
 * kpn_pix_l1_loss: the L1 terms of the training loss - pix_loss(src, tar, {"l1": lambda}) (src/utils.py:164-168) as
 * compute_error_nerf applies it to tex_cal = tex_fg (lambda_l1_c) and tex_cal_fine = tex_fg_fine (lambda_l1), src/utils.py:
 * 128-145, configs/zju.json:109-112 - together with its gradient: loss[0] (device) = lambda * mean|src - tar| over n
 * elements; d_src (n floats, may be NULL) = lambda * sign(src - tar) / n, i.e. what loss.backward() hands to the renderer
 * (the d_tex_fg / d_tex_fg_fine of kpn_render_grads).  scratch: 16,392 bytes as kpn_mse_psnr.  Deterministic. */
int kpn_pix_l1_loss(const float* src, const float* tar, int64_t n, float lambda, float* loss, float* d_src, void* scratch,
                    void* stream);
/* kpn_train_loss: every pixel and mask term of compute_error_nerf (src/utils.py:108-171) for the outputs the renderer produces
 * (no auxiliary heads), values and seed gradients, in ONE launch:
 *   terms[0] e_pix_c     = l1_c  * mean|tex - tar|                                   (src/utils.py:130-132, 179)
 *   terms[1] e_pix_l1    = l1    * mean|tex_fine - tar|                              (src/utils.py:141, 179)
 *   terms[2] e_pix_l2    = l2    * mean (tex_fine - tar)^2                           (src/utils.py:181)
 *   terms[3] e_pix_lp    = lp    * mean (|tex_fine - tar| + 1e-4)^0.4                (src/utils.py:183)
 *   terms[4] mask_loss_c = mloss * mean (clip(alpha, 1e-3, 1) - tar_alpha)^2         (src/utils.py:150-153)
 *   terms[5] mask_loss_f = mloss * mean (clip(alpha_fine, 1e-3, 1) - tar_alpha)^2    (src/utils.py:155-158)
 * tex, tex_fine, tar: 3n floats; alpha, alpha_fine, tar_alpha: n floats (batch 1).  A term whose weight is <= 0 or one of whose
 * inputs is NULL is skipped: its slot is 0 and its gradient buffer is not touched.  Gradients are what torch autograd derives for
 * an upstream gradient of 1 per term (any gradient pointer may be NULL: not written):
 *   d_tex (3n) of terms[0];  d_tex_fine (3 x 3n): row k of terms[1 + k] (l1, l2, lp kept apart, so that a caller can scale each
 *   by its own upstream gradient);  d_alpha (n) of terms[4];  d_alpha_fine (n) of terms[5].
 * l1: lambda sign(d) / 3n (sign(0) = 0);  l2: 2 lambda d / 3n;  lp: 0.4 lambda (|d| + 1e-4)^-0.6 sign(d) / 3n;  mask: 2 lambda
 * (c - t) / n where 1e-3 <= a <= 1 (both ends inclusive, torch's clamp backward) and 0 elsewhere; a NaN alpha makes its term NaN
 * and has gradient 0, as in torch.  terms[0], terms[1], d_tex and row 0 of d_tex_fine are bit-identical to two kpn_pix_l1_loss
 * calls.  Deterministic (per-block fp64 partial sums added in block order, no float atomics).
 * workspace: kpn_train_loss_workspace_bytes(n) bytes (256-byte aligned); its first word is a ticket that has to be 0 on entry and that the kernel
 * leaves at 0.  reset_ticket != 0 zeroes it first (one memset node) - pass it for the first call on a workspace of undefined
 * contents; later calls on the same workspace (for the same or a smaller n) pass 0 and are a single launch.  Calls that share a
 * workspace must be ordered (one stream). */
typedef struct kpn_train_loss_args {
    const float* tex;                 /* tex_cal (3n) or NULL */
    const float* tex_fine;            /* tex_cal_fine (3n) or NULL */
    const float* tar;                 /* tar_img (3n); may be NULL only if tex and tex_fine are */
    const float* alpha;               /* (n) or NULL */
    const float* alpha_fine;          /* (n) or NULL */
    const float* tar_alpha;           /* (n) or NULL */
    int64_t n;                        /* pixels */
    float l1_c, l1, l2, lp, mloss;    /* lambda_l1_c, lambda_l1, lambda_l2, lambda_lp, lambda_mloss */
    int32_t reset_ticket;
    float* terms;                     /* 6 floats */
    float* d_tex;                     /* 3n or NULL */
    float* d_tex_fine;                /* 3 x 3n or NULL */
    float* d_alpha;                   /* n or NULL */
    float* d_alpha_fine;              /* n or NULL */
} kpn_train_loss_args;
size_t kpn_train_loss_workspace_bytes(int64_t n);
int kpn_train_loss(const kpn_train_loss_args* args, void* workspace, void* stream);
int kpn_frame_to_rgb8(const float* chw, int32_t height, int32_t width, int32_t bgr, uint8_t* hwc_out, void* stream);
int kpn_mse_psnr(const float* pred, const float* gt, int64_t n, double* out2, void* scratch, void* stream);
/* kpn_ssim: ZJUEvaluator._compute_ssim (src/zju_evaluator.py:21-45) = skimage 0.19 (environment.yml:135)
 * structural_similarity(pred, gt, multichannel=True) on the crop [y0, y0+h) x [x0, x0+w) (cv2.boundingRect of
 * mask_at_box, computed by the caller) of two (3,H,W) fp32 images: 7x7 uniform window, sample covariance, data_range 2
 * (skimage's default for float images), mean over the interior and the channels.  out (device, 1 double).
 * skimage is not installed here: the oracle restates its published algorithm with scipy.ndimage.uniform_filter (the
 * filter skimage itself calls); parity against skimage proper is unpinned. */
size_t kpn_ssim_scratch_bytes(int32_t crop_w, int32_t crop_h);
int kpn_ssim(const float* pred_chw, const float* gt_chw, int32_t height, int32_t width, int32_t x0, int32_t y0, int32_t crop_w,
             int32_t crop_h, double* out, void* scratch, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Measurement hooks (bench.py).  When enabled, every launch of the dominant kernel (k_geo_rows) is
 * bracketed by HIP events recorded on the caller's stream and the number of (point,view) rows it
 * processed is copied back asynchronously.  kpn_profile_collect synchronises the recorded events
 * and returns the totals since kpn_profile_enable(1).  Diagnostic only; off by default. */
int kpn_profile_enable(int32_t on);
int kpn_profile_collect(double* geo_rows_ms_host, int64_t* launches_host, int64_t* rows_host);
/* The row scratch between the two field kernels is capped (kpn_row_scratch_cap_bytes(): 3 GiB by default, environment
 * variable KPN_ROW_SCRATCH_MIB); a pass with more valid (point, view) rows than fit is evaluated in batches that reuse it.
 * The launcher cannot know the number of batches without a sync, so it launches the worst-case number and the surplus
 * launches return at once: kpn_profile_collect2 reports them separately (ms / launches / rows cover the launches that
 * processed rows). */
int kpn_profile_collect2(double* geo_rows_ms_host, int64_t* launches_host, int64_t* rows_host, int64_t* surplus_launches_host);
/* The same plus *clock_ghz_host = the shader clock the chip sustained under the recorded pair-tile rows-kernel launches: shader
 * cycles (s_memtime) between the first workgroup's entry and its last work item, divided by the launches' HIP-event time (a lower
 * bound: the workgroup finishes a little before its launch).  The MI355X clocks to its power budget (≈ 1.9 GHz under this load,
 * 2.4 GHz peak): a roofline fraction against the 2.4 GHz peak understates what the kernel does per cycle.  0 if not measured. */
int kpn_profile_collect3(double* geo_rows_ms_host, int64_t* launches_host, int64_t* rows_host, int64_t* surplus_launches_host,
                         double* clock_ghz_host);
/* The same for the BACKWARD (kpn_query_backward, kpn_render_rays_train_backward[_kept]): HIP events around each kernel group of
 * every pass while enabled.  kpn_bwd_profile_collect: ms5 / launches5 = time and launch groups of [0] k_geo_rows (the forward's rows,
 * only when the pass recomputes them), [1] k_color_bwd, [2] k_fuse_bwd, [3] k_geo_rows_bwd, [4] k_weight_grad<*> + reduce;
 * *rows = valid points x V of the recorded passes (the rows k_geo_rows_bwd and k_weight_grad process), *kept_rows = valid points x
 * views kept by the pass's dropout mask (the rows k_color_bwd processes), *points = valid points.  Synchronises the device. */
int kpn_bwd_profile_enable(int32_t on);
int kpn_bwd_profile_collect(double* ms5, int64_t* launches5, int64_t* rows, int64_t* kept_rows, int64_t* points);
size_t kpn_row_scratch_cap_bytes(void);
/* Process-wide; workspace sizes queried before a change are stale (query kpn_*_workspace_bytes again). */
int kpn_set_row_scratch_cap_bytes(size_t bytes);

/* TRAIN branch of batch_render_pifu_nerf (forward only), every random draw supplied by the caller so that it can
 * be the reference's own: src/model.py:1008-1017 (patch pixels), :1049-1053 (stratified jitter), :993-994 (density
 * noise, coarse and fine eval), :742-748 (per-view dropout of the coarse and of the fine query), :1129 (random
 * importance samples).  `args` as for kpn_render_rays with nx*ny = n rays (x0,y0,step unused); outputs are (C,ny,nx)
 * planar in patch order.  Backward: kpn_render_rays_train_backward. */
typedef struct kpn_train_args {
    const int32_t* pix;          /* (R,2) target pixels (x,y) */
    const float* u_coarse;       /* (R,Sc)        th.rand_like(z) */
    const float* noise_coarse;   /* (R*Sc)        th.randn_like(rad) of the coarse eval_func; NULL iff std == 0 */
    const float* noise_fine;     /* (R*(Sc+Sf))   ... of the fine eval_func */
    const float* u_fine;         /* (R,Sf)        th.rand of importance_sample */
    uint32_t keep_coarse;        /* bit v = source view v kept by the coarse query's dropout */
    uint32_t keep_fine;          /* ... by the fine query's dropout */
    float rand_noise_std;        /* dr_kwargs.rand_noise_std (0.01) */
} kpn_train_args;
int kpn_render_rays_train(const kpn_scene_desc* desc, const void* scene_ws, const float* packed_weights,
                          const kpn_render_args* args, const kpn_train_args* train, void* workspace,
                          size_t workspace_bytes, void* stream);

/* loss.backward() through the train branch (the field part of training_step, src/model.py:128-155): given the
 * gradients of kpn_render_rays_train's seven outputs — planar (C, ny*nx) like the outputs, NULL = zero — accumulate the
 * gradients of every hot-path parameter (d_plain, flat layout of kpn_pack_weights' input, raw ani_al last) and of the
 * three feature maps (channels-last, like kpn_query_backward).  Same `args` / `train` as the forward call (outputs in
 * `args` are ignored).  Nothing is kept from the forward pass: z, rgba and the field activations are recomputed per
 * pass; the sample positions carry no gradient (drawn under no_grad, src/model.py:1038,1118). */
typedef struct kpn_render_grads {
    const float* d_tex_fg; const float* d_depth; const float* d_alpha;
    const float* d_tex_fg_fine; const float* d_depth_fine; const float* d_alpha_fine; const float* d_sdf;
} kpn_render_grads;
size_t kpn_render_rays_train_backward_workspace_bytes(const kpn_scene_desc* desc, const kpn_render_args* args);
int kpn_render_rays_train_backward(const kpn_scene_desc* desc, const void* scene_ws, const float* packed_weights,
                                   const kpn_render_args* args, const kpn_train_args* train, const kpn_render_grads* grads,
                                   float* d_plain, float* d_geo0, float* d_geo1, float* d_tex, void* workspace,
                                   size_t workspace_bytes, void* stream);

/* The same pair with the forward's work KEPT for the backward: kpn_render_rays_train_keep is kpn_render_rays_train (same
 * outputs, bit for bit) that also fills `state` (kpn_render_rays_train_state_bytes: rays, depths, field values and the
 * valid lists + (point, view) rows of both field passes, per chunk of rays — about 1 KB per field evaluation);
 * kpn_render_rays_train_backward_kept is kpn_render_rays_train_backward (same gradients up to summation order: the
 * order of the valid list varies from call to call) that reads them from `state` instead of repeating the forward — the field part of a
 * training iteration then runs the forward once (reference: autograd keeps every activation; here only the pass state is
 * kept, the MLP activations are still recomputed tile by tile inside the backward kernels).  `workspace` is the one of
 * kpn_render_rays_train_backward_workspace_bytes.  The state is valid until the weights, the scene or the draws change. */
size_t kpn_render_rays_train_state_bytes(const kpn_scene_desc* desc, const kpn_render_args* args);
int kpn_render_rays_train_keep(const kpn_scene_desc* desc, const void* scene_ws, const float* packed_weights,
                               const kpn_render_args* args, const kpn_train_args* train, void* state, size_t state_bytes,
                               void* stream);
int kpn_render_rays_train_backward_kept(const kpn_scene_desc* desc, const void* scene_ws, const float* packed_weights,
                                        const kpn_render_args* args, const kpn_train_args* train, const kpn_render_grads* grads,
                                        float* d_plain, float* d_geo0, float* d_geo1, float* d_tex, void* state,
                                        size_t state_bytes, void* workspace, size_t workspace_bytes, void* stream);

/* Both train-branch backward calls with the keypoint gradient (kpn_query_backward_kpt above; src/spatial.py:76-118): d_kpt3d
 * (n_kpt, 3) receives the sum of the coarse and the fine pass of every chunk of rays, +=.  `workspace` is the one of
 * kpn_render_rays_train_backward_workspace_bytes_kpt for both; the state is the plain call's. */
size_t kpn_render_rays_train_backward_workspace_bytes_kpt(const kpn_scene_desc* desc, const kpn_render_args* args);
int kpn_render_rays_train_backward_kpt(const kpn_scene_desc* desc, const void* scene_ws, const float* packed_weights,
                                       const kpn_render_args* args, const kpn_train_args* train, const kpn_render_grads* grads,
                                       float* d_plain, float* d_geo0, float* d_geo1, float* d_tex, float* d_kpt3d, int32_t n_kpt,
                                       void* workspace, size_t workspace_bytes, void* stream);
int kpn_render_rays_train_backward_kept_kpt(const kpn_scene_desc* desc, const void* scene_ws, const float* packed_weights,
                                            const kpn_render_args* args, const kpn_train_args* train, const kpn_render_grads* grads,
                                            float* d_plain, float* d_geo0, float* d_geo1, float* d_tex, float* d_kpt3d,
                                            int32_t n_kpt, void* state, size_t state_bytes, void* workspace,
                                            size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The perceptual term of the training loss, VGGLoss (src/utils.py:750-805), called by compute_error on every training and
 * validation step (src/utils.py:164-170, lambda_vgg in configs/zju.json):
 *   loss = lambda * sum_i tap_w[i] * mean|phi_i(norm(x)) - phi_i(norm(y))|,   norm(v) = (v - mean) / std per channel,
 * phi_i = vgg19.features[0:2], [2:7], [7:12], [12:21] (relu1_1 .. relu4_1): nine 3x3 / stride 1 / pad 1 convolutions with
 * bias and ReLU, 2x2 / stride 2 floor-mode max-pools in front of the 3rd, 5th and 9th; widths 64 64 | 128 128 | 256 x4 | 512.
 * x, y: (B, 3, H, W) fp32, B >= 1, H, W >= 8.  d_x (may be NULL = loss only): d loss / d x, with y detached and the VGG
 * parameters frozen (src/utils.py:772-774,804) as autograd produces it: sign(0) = 0, ReLU passes where its output is > 0, a
 * max-pool window's gradient goes to its first maximum in row-major order.  x and y go through bit-identical arithmetic, so
 * x == y gives loss 0 and d_x 0 exactly; results are bit-reproducible (no float atomics).
 *
 * Weights: `plain` (device, kpn_vgg_plain_floats) = the nine convolutions of features[0:21] in order, each its OIHW weight
 * then its bias; kpn_vgg_pack_device writes both packed copies the kernels read (forward, and transposed + flipped for the
 * backward) into `packed` (device, kpn_vgg_packed_floats, 16-byte aligned).  mean_host[3], std_host[3] (VGGLoss.normalize),
 * tap_w_host[4] (VGGLoss.weights) are host arrays.  `stages` (may be NULL; kpn_vgg_stage_floats): the post-ReLU output of
 * every convolution, conv 1 .. 9 one after the other, each (2B, H_l, W_l, C_l) NHWC with the B images of x first, then those
 * of y (H_l = H >> pools before it) - for the parity check.  `workspace` (kpn_vgg_workspace_bytes, 16-byte aligned). */
size_t kpn_vgg_plain_floats(void);
size_t kpn_vgg_packed_floats(void);
int kpn_vgg_pack_device(const float* plain, float* packed, void* stream);
size_t kpn_vgg_workspace_bytes(int32_t B, int32_t H, int32_t W);
size_t kpn_vgg_stage_floats(int32_t B, int32_t H, int32_t W);
int kpn_vgg_loss(const float* x, const float* y, int32_t B, int32_t H, int32_t W, const float* packed, const float* mean_host,
                 const float* std_host, const float* tap_w_host, float lambda, float* loss, float* d_x, float* stages,
                 void* workspace, size_t workspace_bytes, void* stream);

/* FLOP / byte model of one field evaluation, for roofline reporting */
double kpn_flops_per_point(int32_t n_views);
/* algorithmic FLOPs of one k_geo_rows row = 2 * 70,080 MACs (MLPUNet layers1) */
double kpn_flops_per_row(void);

/* Device self-test of the MFMA operand/result lane maps the kernels assume (asymmetric operands).
 * Returns 0 if D == A*B for v_mfma_f32_32x32x2_f32 in the assumed layout. */
int kpn_selftest_mfma(float* scratch_256k, void* stream, float* max_err_host);

/* -------------------------------------------------------------------------------------------------------------------------
 * The image encoders in front of the ray march, forward only (inference): the reference's HGFilterV2 (geometry) and
 * ResBlkEncoder (texture), src/utils.py:199-474, as attach_geo_feat / attach_tex_feat call them (src/model.py:653-680):
 *   feat_geo = geo_encoder(2 * avg_pool2d^ds(im) - 1),   feat_tex = tex_encoder(2 * avg_pool2d^ds(im) - 1).
 * img: (V, 3, H, W) fp32 NCHW in [0, 1] (the source images, before the ds average pools; ds = ds_geo / ds_tex, 0 or 1: one
 * average pool is one rounding, as in the reference; more pools are refused with KPN_EINVAL).
 * Outputs are NHWC.  Kernels: csrc/encoder_kernels.hip (fp32 MFMA implicit GEMM; no float atomics, fixed-order reductions:
 * bit-reproducible, and the maps of an image do not depend on the other images of the call).
 *
 * Geometry: HGFilterV2(n_stack = 1, n_downsample = 4, hd = False, norm = "group", out_ch, out_ch_hd); h = H >> ds and
 * w = W >> ds must be multiples of 64 (KPN_EINVAL otherwise).  feat (V, h/4, w/4, out_ch) = HGFilterV2.forward(x)[0],
 * feat_hd (V, h, w, out_ch_hd) = [1].  Texture: ResBlkEncoder(3, out_ch, ngf, n_down, n_blocks, n_up, norm = "instance"), ngf a
 * power of two >= 8, 1 <= n_up <= n_down <= 5; any h, w >= 1; feat (V, ht, wt, out_ch) with ht = h after n_down steps of
 * (h - 1) / 2 + 1 and n_up doublings.  eps: the eps of the GroupNorm / InstanceNorm2d modules.
 *
 * Weights: `plain` (device, *_plain_floats) holds the parameters in the order the forward meets them - per convolution its
 * OIHW (ConvTranspose2d: IOHW) weight then its bias, per GroupNorm gamma then beta, a ConvBlock as bn1, conv1, bn2, conv2, bn3,
 * conv3 [, bn4, downsample convolution]; geometry: conv1, bn1, conv2, unpack1.conv, unpack1.norm, conv_out, conv3, conv4, the
 * hourglass in call order (b1_4, b2_4, b1_3, b2_3, b1_2, b2_2, b1_1, b2_1, b2_plus_1, b3_1 .. b3_4), top_m_0, conv_last0,
 * bn_end0, l0; texture: the convolutions of `layers` in order (keypointnerf_amd/encoders.py builds both from a module).
 * *_pack_device writes `packed` (device, *_packed_floats, 16-byte aligned).  `stages` (may be NULL; *_stage_floats): named
 * intermediate tensors, NHWC, for locating a disagreement; *_stage_info(index) gives name, offset (floats) and dims (V, H, W, C)
 * of entry `index`, KPN_EINVAL behind the last.  `workspace` (*_workspace_bytes, 16-byte aligned; 0 = unsupported size). */
size_t kpn_geo_encoder_plain_floats(int32_t out_ch, int32_t out_ch_hd);
size_t kpn_geo_encoder_packed_floats(int32_t out_ch, int32_t out_ch_hd);
int kpn_geo_encoder_pack_device(const float* plain, float* packed, int32_t out_ch, int32_t out_ch_hd, void* stream);
size_t kpn_geo_encoder_workspace_bytes(int32_t V, int32_t H, int32_t W, int32_t ds, int32_t out_ch, int32_t out_ch_hd);
size_t kpn_geo_encoder_stage_floats(int32_t V, int32_t H, int32_t W, int32_t ds, int32_t out_ch, int32_t out_ch_hd);
int kpn_geo_encoder_stage_info(int32_t V, int32_t H, int32_t W, int32_t ds, int32_t out_ch, int32_t out_ch_hd, int32_t index,
                               char* name, int32_t name_cap, int64_t* offset, int32_t* dims);
int kpn_geo_encode(const float* img, int32_t V, int32_t H, int32_t W, int32_t ds, int32_t out_ch, int32_t out_ch_hd,
                   const float* packed, float eps, float* feat, float* feat_hd, float* stages, void* workspace,
                   size_t workspace_bytes, void* stream);
size_t kpn_tex_encoder_plain_floats(int32_t ngf, int32_t n_down, int32_t n_blocks, int32_t n_up, int32_t out_ch);
size_t kpn_tex_encoder_packed_floats(int32_t ngf, int32_t n_down, int32_t n_blocks, int32_t n_up, int32_t out_ch);
int kpn_tex_encoder_pack_device(const float* plain, float* packed, int32_t ngf, int32_t n_down, int32_t n_blocks, int32_t n_up,
                                int32_t out_ch, void* stream);
size_t kpn_tex_encoder_workspace_bytes(int32_t V, int32_t H, int32_t W, int32_t ds, int32_t ngf, int32_t n_down, int32_t n_blocks,
                                       int32_t n_up, int32_t out_ch);
size_t kpn_tex_encoder_stage_floats(int32_t V, int32_t H, int32_t W, int32_t ds, int32_t ngf, int32_t n_down, int32_t n_blocks,
                                    int32_t n_up, int32_t out_ch);
int kpn_tex_encoder_stage_info(int32_t V, int32_t H, int32_t W, int32_t ds, int32_t ngf, int32_t n_down, int32_t n_blocks, int32_t n_up,
                               int32_t out_ch, int32_t index, char* name, int32_t name_cap, int64_t* offset, int32_t* dims);
int kpn_tex_encode(const float* img, int32_t V, int32_t H, int32_t W, int32_t ds, int32_t ngf, int32_t n_down, int32_t n_blocks,
                   int32_t n_up, int32_t out_ch, const float* packed, float eps, float* feat, float* stages, void* workspace,
                   size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The parameter leg of a training step: the live parameter tensors <-> the flat vector `plain` of kpn_pack_weights, and the
 * optimizer step, one launch each.  Deterministic (fixed-order fp64 row sums, no atomics).
 *
 * kpn_param_table: the tensors of the KPN_PARAM_LAYERS layers in the order of `plain` (synthetic.py:HOTPATH_LAYERS).  For a layer
 * the reference wraps in torch.nn.utils.weight_norm (src/utils.py:542-543: mlp_geo.layers1.layers.0-2, layers2.layers.0-1)
 * g = weight_g (out) and v_or_w = weight_v (out,in); for every other layer g = NULL and v_or_w = weight (out,in).  b = bias (out),
 * ani_al = mlp_tex.ani_al (1).  The same struct names the destinations of the gradients. */
#define KPN_PARAM_LAYERS 19
typedef struct kpn_param_table {
    float* g[KPN_PARAM_LAYERS];
    float* v_or_w[KPN_PARAM_LAYERS];
    float* b[KPN_PARAM_LAYERS];
    float* ani_al;
} kpn_param_table;
/* floats of the side buffer kpn_fold_params leaves for its backward: per weight-normed row (504) the row norm in fp64 and the
 * fp32 scale g / norm; 8-byte aligned.  (kpn_fold_params_shape leaves the same buffer: the norm of a narrow row is the fp64 sum over
 * the 232 canonical columns in the canonical lane order, i.e. the value kpn_fold_params gives for the widened row.) */
size_t kpn_fold_norm_floats(void);
/* kpn_fold_params: replaces torch._weight_norm(v, g, 0) per layer (what weight_norm's hook evaluates, src/utils.py:542-543), the
 * reshapes and the concatenation of weights.plain_tensor_from_module.  Per weight-normed row n = sqrt(sum v^2) and g / n in
 * fp64, s = (float)(g / n), W = v * s: within 2^-23 relative of the exact fold; weights of the other layers, biases and the raw
 * ani_al are copied.  table is read only.  plain_out: kpn_plain_weight_floats(); norms_out: kpn_fold_norm_floats().
 * A row of zero norm gives inf / NaN as torch does.  Null or inconsistent tables: KPN_EINVAL. */
int kpn_fold_params(const kpn_param_table* table, float* plain_out, float* norms_out, void* stream);
/* kpn_fold_params_backward: replaces what loss.backward() runs behind plain_tensor_from_module (the cat's 39 slices and five
 * weight-norm backwards): d_plain -> the gradients of the tensors of `table`, written to the same slots of grads_table (an entry
 * that is NULL is skipped).  dg = dot / n, dv = s dW - (g dot / n^3) v with dot = sum dW v in fp64; everything else is a copy.
 * norms: what kpn_fold_params left for the same table values.  accumulate = 0 overwrites the destinations, != 0 adds to them
 * (.grad's semantics under accumulate_grad_batches). */
int kpn_fold_params_backward(const kpn_param_table* table, const float* norms, const float* d_plain,
                             const kpn_param_table* grads_table, int32_t accumulate, void* stream);
/* kpn_adam_step: replaces the step of the optimizer configure_optimizers returns (torch.optim.Adam, src/model.py:46-47) for the
 * tensors listed in segments_host (a HOST array, read during the call; at most KPN_ADAM_MAX_SEGMENTS per launch, more are served
 * by further launches).  torch.optim.Adam's semantics with amsgrad = False, maximize = False, for step number `step` (counted
 * from 1, kept by the caller on the host: no device-to-host copy, no synchronisation):
 *   g' = g + weight_decay p;  m <- m + (1 - beta1)(g' - m);  v <- beta2 v + (1 - beta2) g'^2;
 *   p <- p - lr / (1 - beta1^step) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps)
 * evaluated per element in fp64 on the fp32 state, m, v and p rounded once each. */
#define KPN_ADAM_MAX_SEGMENTS 64
typedef struct kpn_adam_segment {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    int64_t count;                    /* elements */
} kpn_adam_segment;
typedef struct kpn_adam_args {
    const kpn_adam_segment* segments_host;
    int32_t n_segments;
    int64_t step;
    double lr, beta1, beta2, eps, weight_decay;
} kpn_adam_args;
int kpn_adam_step(const kpn_adam_args* args, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Keypoint sets: models with n_kpt = 1..KPN_N_KPT keypoints and sp_level = 0..KPN_SP_LEVEL octaves of the rel_z_decay encoding.
 * The reference sizes the first linear of mlp_geo from the encoder, D = SpatialEncoder.get_dim() = (1 + 2 sp_level) n_kpt
 * (src/spatial.py:49-53, src/model.py:569-572): its weight is (128, D + 64), the encoding value of block t (0 = dz w, 1 + 2l =
 * sin, 2 + 2l = cos of octave l) and keypoint k sits in column t n_kpt + k (src/spatial.py:110-118), the 64 geometry channels
 * behind them.  The field kernels are built for the 24 / 3 model, whose column is 24 t + k (168 + j for geometry channel j).  A
 * narrower model is served as that model: NARROW column t n_kpt + k <-> CANONICAL column 24 t + k, D + j <-> 168 + j; the
 * canonical columns without a narrow one (PADDED: t > 2 sp_level or k >= n_kpt) carry weight 0, and the keypoint table repeats
 * keypoint 0 in rows n_kpt..23, so a padded encoding value is finite, one a real keypoint produces too, and its product with the
 * zero weight is an exact 0 in every accumulator.  Padded keypoints cost what real ones cost.
 * The NARROW PLAIN vector is `plain` of kpn_pack_weights with layers1.0's W as (128, D + 64); nothing else differs.
 * KPN_N_KPT is the capacity.  Every entry below returns KPN_EINVAL, with a message and before any launch, for n_kpt outside
 * 1..KPN_N_KPT or sp_level outside 0..KPN_SP_LEVEL. */
#define KPN_SP_LEVEL 3    /* configs/zju.json:41 sp_args.sp_level: the capacity */
typedef struct kpn_field_shape { int32_t n_kpt, sp_level; } kpn_field_shape;
/* floats of the narrow plain vector; 0 if the shape is out of range; kpn_plain_weight_floats() for {24, 3} */
size_t kpn_plain_weight_floats_shape(const kpn_field_shape* shape);
/* narrow plain -> plain (kpn_plain_weight_floats()): one launch that writes every element of plain_dev, +0 in the padded columns
 * of layers1.0's W; everything else is a copy. */
int kpn_widen_plain(const kpn_field_shape* shape, const float* narrow_dev, float* plain_dev, void* stream);
/* Its adjoint, a gather: the gradient w.r.t. plain -> the gradient w.r.t. the narrow plain vector, one launch.  The padded
 * columns of d_plain_dev are not read.  accumulate = 0 overwrites d_narrow_dev, != 0 adds to it (as kpn_fold_params_backward). */
int kpn_narrow_plain_grad(const kpn_field_shape* shape, const float* d_plain_dev, float* d_narrow_dev, int32_t accumulate,
                          void* stream);
/* kpn_scene_prepare for desc->kpt3d of (n_kpt, 3) (the reference asserts kpt3d.shape[1] == n_kpt, src/spatial.py:80): rows
 * n_kpt..23 of each view's keypoint table are the camera-frame coordinates of keypoint 0.  kpn_scene_prepare is its n_kpt = 24
 * case, bit for bit. */
int kpn_scene_prepare_kpt(const kpn_scene_desc* desc, int32_t n_kpt, void* scene_ws, void* stream);
/* kpn_fold_params / kpn_fold_params_backward for a table whose v_or_w[0] (and, in grads_table, its gradient slot) is the narrow
 * (128, D + 64) weight_v of layers1.0; plain_out and d_plain are canonical.  One launch each: the same kernels with a load map -
 * the thread that owns canonical column c reads the narrow column mapped to it, or 0 - so plain_out, norms_out (the fp64 row
 * sums run over the 232 canonical columns, the padded ones adding exact zeros), dg and dv (written through the same map; a
 * padded column has no destination) are bit for bit those of kpn_fold_params / _backward on the widened weight_v, gathered. */
int kpn_fold_params_shape(const kpn_field_shape* shape, const kpn_param_table* table, float* plain_out, float* norms_out,
                          void* stream);
int kpn_fold_params_backward_shape(const kpn_field_shape* shape, const kpn_param_table* table, const float* norms,
                                   const float* d_plain, const kpn_param_table* grads_table, int32_t accumulate, void* stream);

/* ---------------------------------------------------------------------------------------------
 * One convolution of the image encoders, forward and backward: replaces torch.nn.functional.conv2d and its autograd
 * (convolution_backward) as the layers of ConvBlock, HourGlass and HGFilterV2 call them (src/utils.py:416-474, 261-309, 322-414).
 * Scope: groups = 1, dilation = 1, stride 1, a square kernel k in {1, 3, 5}, zero padding 0 <= pad <= k - 1, optional bias, fp32,
 * cin and cout multiples of 4 (at most 1024).  Anything else - stride 2, the 7x7 stems, replication padding, ConvTranspose2d -
 * is refused with KPN_EINVAL; kpn_last_error() names the field.
 * Activations are NHWC (torch channels_last): x (N, H, W, cin), y and dy (N, Ho, Wo, cout), Ho = H + 2 pad - k + 1; the weight
 * is OIHW as nn.Conv2d holds it.  Kernels: csrc/encoder_kernels.hip (fp32 MFMA, exact fp32 products, fp32 accumulation).
 *   y  = conv(x, w) + bias                                 k_enc_conv (the encoders' forward kernel), split K as there
 *   dx = conv(dy, w'[ci][co][k-1-ky][k-1-kx], pad k-1-pad)  k_enc_conv over the second packed copy
 *   dw[co][ci][ky][kx] = sum_pixels x[pixel + tap] dy[pixel][co]   k_enc_wgrad: fp32 chains over ranges of output pixels (from the
 *                        shape alone, kpn_conv2d_wgrad_ranges), the ranges added in order in fp64 and rounded once
 *   db[co] = sum_pixels dy[pixel][co]                      fp64 partial sums over fixed pixel chunks, added in order, rounded once
 * No float atomics: every result is bit-identical from run to run.
 * kpn_conv2d_packed_floats / kpn_conv2d_pack_device read only cin, cout, k of the descriptor: `packed` (device, 16-byte aligned)
 * holds the forward copy, then the input-gradient copy.  `workspace` (kpn_conv2d_workspace_bytes, 16-byte aligned; 0 = unsupported
 * descriptor) serves the forward and the backward alike.  bias: NULL exactly when has_bias = 0.
 * kpn_conv2d_backward: each of dx, dw, db may be NULL - that leg is not launched and nothing is written for it; dw (OIHW) and db
 * are overwritten, not accumulated.  packed is read for dx only, x for dw only. */
typedef struct kpn_conv2d_desc {
    int32_t N, H, W;                  /* input images and their size */
    int32_t cin, cout, k, pad, has_bias;
} kpn_conv2d_desc;
size_t kpn_conv2d_packed_floats(const kpn_conv2d_desc* desc);
int kpn_conv2d_pack_device(const kpn_conv2d_desc* desc, const float* w_oihw, float* packed, void* stream);
size_t kpn_conv2d_workspace_bytes(const kpn_conv2d_desc* desc);
/* pixel ranges of the weight gradient (0 = unsupported descriptor): chunks = ceil(N Ho Wo / 16), tiles = ceil(k k cin / BM) *
 * ceil(cout / BN) with (BM, BN) = (64, 64), or (128, 32) when cout <= 32; chunks per range = max(20, ceil(chunks / clamp(1024 / tiles,
 * 1, 64))); ranges = ceil(chunks / chunks per range) */
int32_t kpn_conv2d_wgrad_ranges(const kpn_conv2d_desc* desc);
int kpn_conv2d_forward(const kpn_conv2d_desc* desc, const float* x, const float* packed, const float* bias, float* y,
                       void* workspace, size_t workspace_bytes, void* stream);
int kpn_conv2d_backward(const kpn_conv2d_desc* desc, const float* x, const float* dy, const float* packed, float* dx, float* dw,
                        float* db, void* workspace, size_t workspace_bytes, void* stream);

/* The arithmetic of the three GEMMs (y, dx, dw) of a stride-1 convolution, chosen per call.  The kpn_conv2d_ex_* entry points are
 * kpn_conv2d_* with `arith` behind the descriptor; with KPN_CONV_F32 they are the same code and give the same bits, packed buffer
 * included.  Another value of arith is refused with KPN_EINVAL ("arith must be ..."; the size queries return 0) and launches nothing.
 *   KPN_CONV_F32     v_mfma_f32_32x32x2_f32 as described above.
 *   KPN_CONV_BF16X3  v_mfma_f32_32x32x16_bf16 (csrc/encoder_split_kernels.hip).  Every fp32 operand value v is carried as three bf16
 *                    pieces, h = bf16(v), m = bf16(v - h), l = bf16(v - h - m) (round to nearest even; the residuals are exact in fp32),
 *                    so |v - (h + m + l)| <= 2^-24 |v| over fp32's whole exponent range: no range guard and no scales, and scaling an
 *                    operand by a power of two scales the result by it exactly (short of overflow and subnormals).  A product a * b
 *                    is six piece products, accumulated in fp32 in this order per 16 K entries and accumulator:
 *                        ah bh, ah bm, am bh, am bm, ah bl, al bh
 *                    (what is left out is below 2^-24 of the product).  Activations are split in the kernel as they are staged, once
 *                    per tile; weights at pack time: `packed` holds 6 bytes per weight (kpn_conv2d_ex_packed_floats counts floats of
 *                    4 bytes), the forward copy then the input-gradient copy, each [chunk of 32 K][piece][8 K][cout_p][8 bf16].
 *                    Tiles: 128 x 64 (pixels x channels), or 256 x 32 when cout <= 32, four wavefronts with two accumulators each,
 *                    K chunk 32.  Split K: as kpn_conv2d_forward, from the per-image geometry with these tiles and chunks - an image's y
 *                    and dx do not depend on its batch.  dw: the pixel index is the MFMA's K; after every 16 pixels the fp32
 *                    accumulators are added to fp64 sums; the range rule is the one of kpn_conv2d_wgrad_ranges with (BM, BN) =
 *                    (128, 64), or (256, 32) when cout <= 32.  db does not depend on arith.  No float atomics.
 *                    Accuracy: that of the fp32 kernels against fp64 (tests/conv_arith_cases.py).
 * `packed`, `workspace` and the range count belong to one arithmetic: query and pack with the arith of the call.  Packed sizes differ
 * between the two (6 against 4 bytes per weight), but the calls do not take the size of `packed`: handing a pack of the other
 * arithmetic is the caller's contract, as a pack of another descriptor is.
 * Not served with KPN_CONV_BF16X3 (there is no _ex form): kpn_conv2d_s2_*, kpn_conv2d_rp_*, kpn_res_encoder_*, kpn_geo_encode,
 * kpn_tex_encode, the VGG loss; there is no two-piece fp16 variant. */
enum { KPN_CONV_F32 = 0, KPN_CONV_BF16X3 = 1 };
size_t kpn_conv2d_ex_packed_floats(const kpn_conv2d_desc* desc, int32_t arith);
int kpn_conv2d_ex_pack_device(const kpn_conv2d_desc* desc, int32_t arith, const float* w_oihw, float* packed, void* stream);
size_t kpn_conv2d_ex_workspace_bytes(const kpn_conv2d_desc* desc, int32_t arith);
int32_t kpn_conv2d_ex_wgrad_ranges(const kpn_conv2d_desc* desc, int32_t arith);
int kpn_conv2d_ex_forward(const kpn_conv2d_desc* desc, int32_t arith, const float* x, const float* packed, const float* bias, float* y,
                          void* workspace, size_t workspace_bytes, void* stream);
int kpn_conv2d_ex_backward(const kpn_conv2d_desc* desc, int32_t arith, const float* x, const float* dy, const float* packed, float* dx,
                           float* dw, float* db, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The resolution-changing layers of the image encoders, forward and backward: the three kinds kpn_conv2d_* refuses.  groups = 1,
 * dilation = 1, zero padding, optional bias, fp32.  Activations are NHWC (torch channels_last) except the stem's input, which is
 * NCHW and read as it is (an already normalised tensor: no 2 x - 1).  Kernels: csrc/encoder_kernels.hip, the encoders' own.
 *   KPN_S2_CONV3    y (N, H/2, W/2, cout) = conv(x (N, H, W, cin), w OIHW, stride 2, pad 1)
 *                   dx = conv_transpose(dy, w, stride 2, pad 1, output_padding 1): the four-gather transposed kernel over a second
 *                   packed copy of the same weight - exact for even H, W, which is why odd ones are refused
 *                   dw: the stride-1 layer's weight gradient with stride-2 im2col rows
 *   KPN_S2_STEM7    y (N, Ho, Wo, cout) = conv(x (N, cin, H, W), w OIHW, stride 2, pad 3), Ho = (H - 1) / 2 + 1; no input gradient;
 *                   dw: the same GEMM over K rows tap * 4 + ci, the padded channel never loaded and never stored
 *   KPN_S2_DECONV3  y (N, 2H, 2W, cout) = conv_transpose(x (N, H, W, cin), w (cin, cout, 3, 3), stride 2, pad 1, output_padding 1)
 *                   dx = conv(dy, w read as OIHW, stride 2, pad 1)
 *                   dw (cin, cout, 3, 3): that convolution's weight gradient with the roles swapped - im2col rows from dy, the
 *                   other operand x, over the N H W source pixels
 *   db[co] = sum over the pixels of dy, as kpn_conv2d_backward.
 * Split K, the ranges of the weight gradient (the rule of kpn_conv2d_wgrad_ranges over the GEMM named above: K rows kh kw cin_p with
 * cin_p = cin rounded up to 4, the GEMM's cout and pixel count), fp64 range sums and the fixed-order combine are those of
 * kpn_conv2d_*: no float atomics, bit-identical from run to run.
 * kpn_conv2d_s2_packed_floats / _pack_device read only kind, cin, cout: `packed` (device, 16-byte aligned) holds the forward copy,
 * then (not for the stem) the input-gradient copy.  `workspace` (kpn_conv2d_s2_workspace_bytes, 16-byte aligned; 0 = unsupported
 * descriptor) serves the forward and the backward alike.  bias: NULL exactly when has_bias = 0.
 * kpn_conv2d_s2_backward: each of dx, dw, db may be NULL - that leg is not launched and nothing is written for it; dw and db are
 * overwritten, not accumulated.  packed is read for dx only, x for dw only.  A refused call (KPN_EINVAL; kpn_last_error() names the
 * field) launches nothing. */
enum { KPN_S2_CONV3 = 0,    /* Conv2d(k=3, stride 2, pad 1); NHWC x; H, W even; cin, cout multiples of 4 in 4..1024 */
       KPN_S2_STEM7 = 1,    /* Conv2d(k=7, stride 2, pad 3); x is NCHW (N, cin, H, W), 1 <= cin <= 4, any H, W >= 1;
                               cout a multiple of 4 in 4..1024; no input gradient (dx must be NULL) */
       KPN_S2_DECONV3 = 2 };/* ConvTranspose2d(k=3, stride 2, pad 1, output_padding 1); NHWC x (N,H,W,cin) -> y (N,2H,2W,cout);
                               weight (cin, cout, 3, 3); cin, cout multiples of 4 in 4..1024 */
typedef struct kpn_conv2d_s2_desc { int32_t N, H, W, cin, cout, kind, has_bias; } kpn_conv2d_s2_desc;
size_t kpn_conv2d_s2_packed_floats(const kpn_conv2d_s2_desc* desc);
int kpn_conv2d_s2_pack_device(const kpn_conv2d_s2_desc* desc, const float* w, float* packed, void* stream);
size_t kpn_conv2d_s2_workspace_bytes(const kpn_conv2d_s2_desc* desc);
int32_t kpn_conv2d_s2_wgrad_ranges(const kpn_conv2d_s2_desc* desc);
int kpn_conv2d_s2_forward(const kpn_conv2d_s2_desc* desc, const float* x, const float* packed, const float* bias, float* y,
                          void* workspace, size_t workspace_bytes, void* stream);
int kpn_conv2d_s2_backward(const kpn_conv2d_s2_desc* desc, const float* x, const float* dy, const float* packed, float* dx, float* dw,
                           float* db, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The replication-padded convolutions of the texture encoder, forward and backward: ReplicationPad2d(k / 2) + Conv2d(k, stride 1) as
 * ResBlkEncoder and ResBlk hold them (src/utils.py:199-259) - the 7x7 stem, the two 3x3 convolutions of every ResBlk, the 7x7 output
 * layer.  groups = 1, dilation = 1, optional bias, fp32; the output grid is the input grid, and any H, W >= 1 is served, sizes below
 * the pad included.  The padded tensor never exists: the loads clamp the source coordinate.  Activations are NHWC (torch channels_last)
 * except the stem's input, which is NCHW and read as it is.  Kernels: csrc/encoder_kernels.hip, the encoders' own.
 *   y[o] = sum_tap sum_ci w[co][ci][tap] x[clamp(o + tap - p)] + bias           k_enc_conv with the clamped load, split K as there
 *   dx[(y, x)][ci] = sum_(ky, kx) sum_co w[co][ci][ky][kx] sum_{oy in Ry(y, ky)} sum_{ox in Rx(x, kx)} dy[(oy, ox)][co]
 *        Ry(y, ky) = { oy in [0, H) : clamp(oy + ky - p, 0, H - 1) = y }: the one position y - ky + p for 0 < y < H - 1,
 *        [0, min(H - 1, p - ky)] for y = 0, [max(0, H - 1 - ky + p), H - 1] for y = H - 1 (their union when H = 1); Rx alike.
 *        The same GEMM as the zero-padded input gradient over the flipped copy of the weight; its A entry is the sum of dy over that
 *        rectangle (at most (p + 1)^2 values, on the outermost ring of pixels only), added oy outer, ox inner: a gather - no scratch
 *        copy of a padded gradient, no scatter, no atomics
 *   dw: the weight gradient of kpn_conv2d_backward with im2col rows through the clamped load (the stem: K rows tap * 4 + ci over
 *        the NCHW tensor, the padded channel never loaded and never stored); the ranges follow the rule of kpn_conv2d_wgrad_ranges over
 *        K rows k k cin_p (cin_p = cin rounded up to 4), cout and the N H W pixels
 *   db[co] = sum over the pixels of dy, as kpn_conv2d_backward.
 * No float atomics: bit-identical from run to run.
 * kpn_conv2d_rp_packed_floats / _pack_device read only kind, cin, cout: `packed` (device, 16-byte aligned) holds the forward copy,
 * then (not for the stem) the input-gradient copy.  `workspace` (kpn_conv2d_rp_workspace_bytes, 16-byte aligned; 0 = unsupported
 * descriptor) serves the forward and the backward alike.  bias: NULL exactly when has_bias = 0.
 * kpn_conv2d_rp_backward: each of dx, dw, db may be NULL - that leg is not launched and nothing is written for it; dw (OIHW) and db
 * are overwritten, not accumulated.  packed is read for dx only, x for dw only.  A refused call (KPN_EINVAL; kpn_last_error() names
 * the field) launches nothing. */
enum { KPN_RP_CONV3 = 0,    /* ReplicationPad2d(1) + Conv2d(k=3); NHWC x; cin, cout multiples of 4 in 4..1024 */
       KPN_RP_CONV7 = 1,    /* ReplicationPad2d(3) + Conv2d(k=7); NHWC x; the same channel rule */
       KPN_RP_STEM7 = 2 };  /* ReplicationPad2d(3) + Conv2d(k=7); x is NCHW (N, cin, H, W), 1 <= cin <= 4; cout a multiple of 4 in
                               4..1024; no input gradient (dx must be NULL) */
typedef struct kpn_conv2d_rp_desc { int32_t N, H, W, cin, cout, kind, has_bias; } kpn_conv2d_rp_desc;
size_t kpn_conv2d_rp_packed_floats(const kpn_conv2d_rp_desc* desc);
int kpn_conv2d_rp_pack_device(const kpn_conv2d_rp_desc* desc, const float* w_oihw, float* packed, void* stream);
size_t kpn_conv2d_rp_workspace_bytes(const kpn_conv2d_rp_desc* desc);
int32_t kpn_conv2d_rp_wgrad_ranges(const kpn_conv2d_rp_desc* desc);
int kpn_conv2d_rp_forward(const kpn_conv2d_rp_desc* desc, const float* x, const float* packed, const float* bias, float* y,
                          void* workspace, size_t workspace_bytes, void* stream);
int kpn_conv2d_rp_backward(const kpn_conv2d_rp_desc* desc, const float* x, const float* dy, const float* packed, float* dx, float* dw,
                           float* db, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * One normalisation of the image encoders with the ReLU behind it, forward and backward: replaces torch.nn.functional.group_norm
 * [+ relu] and their autograd as the legs of ConvBlock call them (GroupNorm -> ReLU -> Conv2d, src/utils.py:416-474), and
 * InstanceNorm2d without affine parameters (G = C, affine = 0; ResBlkEncoder, src/utils.py:199-247).
 * Activations are NHWC (torch channels_last), dense, fp32: x, y, dy, dx (N, H, W, C).  Groups are G blocks of cpg = C / G
 * consecutive channels; statistics are per (image, group) over cpg H W values, biased variance.
 * Scope: C a power of two in 4 .. 1024, G dividing C, N in 1 .. 65535, H, W >= 1, N H W C < 2^31, eps > 0, affine and relu in
 * {0, 1}; gamma and beta non-NULL exactly when affine; every pointer 16-byte aligned.  Anything else is refused with KPN_EINVAL;
 * kpn_last_error() names the field.  Kernels: csrc/encoder_kernels.hip.
 *   forward:  the encoders' own statistics (fp64 sums over nchunks = clamp(H W / 256, 1, 64) pixel ranges per image, added in a
 *             fixed order) folded into scale = gamma rstd, shift = beta - mean scale, each rounded once;
 *             y = [relu](fma(x, scale, shift))
 *   backward: g = relu ? (fma(x, scale, shift) > 0 ? dy : 0) : dy - the forward's own bits, recomputed from `stats`, y is not read;
 *             A_c = sum g, B_c = sum g x per (image, channel) in fp64 over the same pixel ranges; per (image, group)
 *             ds = sum_c gamma_c B_c, db = sum_c gamma_c A_c, cnt = cpg H W, c2 = (db mean - ds) rstd^3 / cnt,
 *             c3 = -c2 mean - db rstd / cnt;  dx = fma(g, gamma_c rstd, fma(x, c2, c3));
 *             dgamma_c = sum_n (B_nc - mean A_nc) rstd, dbeta_c = sum_n A_nc: fp64, images in order, rounded once
 * No float atomics: every result is bit-identical from run to run, and an image's y and dx do not depend on its batch.
 * `stats` (kpn_group_norm_stats_floats; written by the forward, read by the backward): scale [N][C], shift [N][C], then
 * mean [N][G], rstd [N][G] - the fp64 statistics rounded once.  `workspace` (kpn_group_norm_workspace_bytes; 0 = unsupported
 * descriptor) serves the forward and the backward alike.
 * kpn_group_norm_backward: each of dx, dgamma, dbeta may be NULL - nothing is written for it (dx = NULL: the elementwise pass is
 * not launched); dgamma and dbeta are overwritten, not accumulated, and refused when affine = 0. */
typedef struct kpn_group_norm_desc {
    int32_t N, H, W, C, G, affine, relu;
    float eps;
} kpn_group_norm_desc;
size_t kpn_group_norm_stats_floats(const kpn_group_norm_desc* desc);
size_t kpn_group_norm_workspace_bytes(const kpn_group_norm_desc* desc);
int kpn_group_norm_forward(const kpn_group_norm_desc* desc, const float* x, const float* gamma, const float* beta, float* y,
                           float* stats, void* workspace, size_t workspace_bytes, void* stream);
int kpn_group_norm_backward(const kpn_group_norm_desc* desc, const float* x, const float* dy, const float* gamma, const float* stats,
                            float* dx, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The two resampling steps between the ConvBlocks of an HourGlass, forward and backward: replace torch.nn.functional.avg_pool2d(x, 2,
 * stride = 2) and skip + torch.nn.functional.interpolate(low, scale_factor = 2, mode = "bicubic", align_corners = True) with their
 * autograd (HourGlass._forward, src/utils.py:287-306).
 * Activations are NHWC (torch channels_last), dense, fp32: the low tensors (N, h, w, C), the high tensors (N, 2h, 2w, C).
 * Scope: N, h, w >= 1, C a positive multiple of 4 (64-bit element indices), every pointer 16-byte aligned.  Anything else is refused with
 * KPN_EINVAL, kpn_last_error() names the field, and nothing is launched.  No workspace.  Kernels: csrc/encoder_kernels.hip.
 *   kpn_avg_pool2_forward:   y[n][i][j][c] = 0.25 (((x[n][2i][2j][c] + x[n][2i][2j+1][c]) + x[n][2i+1][2j][c]) + x[n][2i+1][2j+1][c])
 *   kpn_avg_pool2_backward:  dx[n][y][x][c] = 0.25 dy[n][y / 2][x / 2][c] (exact)
 *   kpn_upsample2x_add_forward:  y = skip + U low, or y = U low for skip = NULL; y_high may be skip itself (in place).  U is ATen's
 *       bicubic x2 with align_corners: for output row y, fy = sy y with sy = (h - 1) / (2h - 1) (0 for h = 1), iy = floor(fy), the four
 *       cubic convolution weights (A = -0.75) of fy - iy on rows clamp(iy - 1 .. iy + 2, 0, h - 1); the same in x; the columns are
 *       added in an fmaf chain per row, the rows in a second chain, skip last
 *   kpn_upsample2x_add_backward: d_low = U^T dy_high as a gather, one thread per four channels of a LOW pixel (r, c): the high rows
 *       y whose taps land on r, found by evaluating the forward's own fy, iy and weights over a widened range of y, each with the
 *       sum of its weights that clamp onto r; the same in x.  Fixed add order: for y ascending { for x ascending: row = fma(dy[y][x],
 *       ax[x], row) }; acc = fma(row, ay[y], acc).  No atomics, no scratch.  The gradient with respect to skip is dy_high itself.
 * Every result is bit-identical from run to run, and an image's results do not depend on its batch. */
typedef struct kpn_resample2_desc {
    int32_t N, h, w, C;               /* low (N, h, w, C), high (N, 2h, 2w, C) */
} kpn_resample2_desc;
int kpn_avg_pool2_forward(const kpn_resample2_desc* desc, const float* x_high, float* y_low, void* stream);
int kpn_avg_pool2_backward(const kpn_resample2_desc* desc, const float* dy_low, float* dx_high, void* stream);
int kpn_upsample2x_add_forward(const kpn_resample2_desc* desc, const float* low, const float* skip /* NULL or high */,
                               float* y_high /* may alias skip */, void* stream);
int kpn_upsample2x_add_backward(const kpn_resample2_desc* desc, const float* dy_high, float* d_low, void* stream);

/* ---------------------------------------------------------------------------------------------
 * A whole ConvBlock(cin, cout, norm = "group") (src/utils.py:416-474) for training, forward and backward, as one call each: replaces
 * the three or four GroupNorm -> ReLU -> Conv2d legs, torch.cat and the residual add, with their autograd.  With c = cout the legs
 * are bn1 / conv1 (cin -> c/2, 3x3), bn2 / conv2 (c/2 -> c/4), bn3 / conv3 (c/4 -> c/4) and, for cin != cout, bn4 / the 1x1
 * downsample convolution (cin -> c); every norm is GroupNorm(min(32, C), C) with parameters, no convolution has a bias.
 * Activations are NHWC (torch channels_last), dense, fp32: x, dx (N, H, W, cin); y, dy (N, H, W, cout).
 * Scope: cin, cout / 2 and cout / 4 powers of two in 4 .. 1024 (cout <= 1024 when cin != cout), N in 1 .. 65535, H, W >= 1,
 * N H W max(cin, cout) < 2^31, eps > 0; every pointer 16-byte aligned.  Anything else is refused with KPN_EINVAL, kpn_last_error()
 * names the field, and nothing is launched.  Kernels: csrc/encoder_kernels.hip; dataflow: csrc/api_block.hip.
 *   params:  gamma[i] / beta[i] of bn(i+1), packed[i] = what kpn_conv2d_pack_device gives for the weight of conv(i+1) (k = 3) and,
 *            at index 3, of the downsample convolution (k = 1): the forward copy, then the flipped copy.  Index 3 is not read for
 *            cin == cout.  The backward does not read beta.
 *   forward: the dataflow of the inference encoders - GroupNorm statistics only (those of kpn_group_norm_forward), scale / shift and
 *            the ReLU applied inside the loads of the convolution (those of kpn_conv2d_forward), the convolutions writing channel
 *            slices, the residual (x, or the downsample leg) added once: y has the bits of the same block computed leg by leg with
 *            kpn_group_norm_forward(relu = 1), kpn_conv2d_forward, a concatenation and one fp32 add.
 *   state (kpn_conv_block_state_floats; written by the forward, read by the backward):
 *            S (N, H, W, 3c/4): the outputs of conv1 (channels [0, c/2)) and conv2 ([c/2, 3c/4)) before the residual is added - the
 *            sources of bn2 and bn3; conv3's output is added to the residual in its epilogue and is not kept.  Then, per leg in
 *            order: scale [N][C], shift [N][C], mean [N][G], rstd [N][G] as kpn_group_norm_forward keeps them.  No normalised tensor.
 *   backward: dx (or NULL), and per leg grads->dgamma[i], dbeta[i], dw[i] (OIHW), each of which may be NULL: nothing is written for
 *            a NULL result, and a leg that neither it nor anything upstream of it needs is not launched.  Results are overwritten,
 *            not accumulated.  Each leg is the input gradient of kpn_conv2d_backward, the weight gradient with the norm and the ReLU
 *            recomputed in its loads, and the norm gradient of kpn_group_norm_backward with the part of dy that reached the leg's
 *            source through the concatenation added behind its expression.  dx = dy + (norm gradient of bn1) for cin == cout;
 *            dx = (norm gradient of bn1) + (norm gradient of bn4), in this order, for cin != cout.
 * `workspace` (kpn_conv_block_workspace_bytes; 0 = unsupported descriptor) serves the forward and the backward alike.
 * No float atomics: every result is bit-identical from run to run, and an image's y and dx do not depend on its batch. */
typedef struct kpn_conv_block_desc {
    int32_t N, H, W, cin, cout;
    float eps;
} kpn_conv_block_desc;
typedef struct kpn_conv_block_params {
    const float* gamma[4];
    const float* beta[4];
    const float* packed[4];
} kpn_conv_block_params;
typedef struct kpn_conv_block_grads {
    float* dgamma[4];
    float* dbeta[4];
    float* dw[4];
} kpn_conv_block_grads;
size_t kpn_conv_block_workspace_bytes(const kpn_conv_block_desc* desc);
size_t kpn_conv_block_state_floats(const kpn_conv_block_desc* desc);
int kpn_conv_block_forward(const kpn_conv_block_desc* desc, const float* x, const kpn_conv_block_params* params, float* y, float* state,
                           void* workspace, size_t workspace_bytes, void* stream);
int kpn_conv_block_backward(const kpn_conv_block_desc* desc, const float* x, const float* dy, const kpn_conv_block_params* params,
                            const float* state, float* dx, const kpn_conv_block_grads* grads, void* workspace, size_t workspace_bytes,
                            void* stream);
/* The block with the arithmetic of its convolutions chosen per call (KPN_CONV_F32 / KPN_CONV_BF16X3 as kpn_conv2d_ex_*): every leg's
 * y, dx and dw GEMMs run in `arith`; the norms, their gradients and the adds do not change.  params->packed[i] then holds what
 * kpn_conv2d_ex_pack_device gives with the same arith.  The block equals, bit for bit, the layer-by-layer computation over
 * kpn_conv2d_ex_* with that arith.  KPN_CONV_F32 is kpn_conv_block_*; an unknown arith is refused with KPN_EINVAL ("arith must be
 * ...", the size queries return 0) and launches nothing. */
size_t kpn_conv_block_ex_workspace_bytes(const kpn_conv_block_desc* desc, int32_t arith);
size_t kpn_conv_block_ex_state_floats(const kpn_conv_block_desc* desc, int32_t arith);
int kpn_conv_block_ex_forward(const kpn_conv_block_desc* desc, int32_t arith, const float* x, const kpn_conv_block_params* params, float* y,
                              float* state, void* workspace, size_t workspace_bytes, void* stream);
int kpn_conv_block_ex_backward(const kpn_conv_block_desc* desc, int32_t arith, const float* x, const float* dy,
                               const kpn_conv_block_params* params, const float* state, float* dx, const kpn_conv_block_grads* grads,
                               void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * A whole ResBlkEncoder(norm = "instance") (src/utils.py:199-259) for training, forward and backward, as one call each: replaces every
 * ReplicationPad2d + Conv2d pair, stride-2 and transposed convolution, InstanceNorm2d [+ ReLU] and residual add, with their autograd.
 * Layers, in module order (kpn_res_encoder_layers = 2 + n_down + 2 n_blocks + n_up of them): the 7x7 stem in_ch -> ngf, n_down
 * Conv2d(k 3, stride 2, pad 1) doubling the width, two replication-padded 3x3 convolutions per ResBlk, n_up ConvTranspose2d(k 3,
 * stride 2, pad 1, output_padding 1) halving it, the replication-padded 7x7 output layer -> out_ch.  Every convolution has a bias;
 * every layer but the last has an InstanceNorm2d(affine = False) behind it.
 * x is the NCHW image (N, in_ch, H, W), read as it is (KPN_RP_STEM7); y, dy are NHWC (N, H >> (n_down - n_up), W >> (n_down - n_up),
 * out_ch), dense, fp32.
 * Scope: in_ch in 1 .. 4; ngf a power of two >= 4 with ngf << n_down <= 1024; 1 <= n_up <= n_down; n_blocks in 0 .. 64; out_ch a multiple
 * of 4 in 4 .. 1024; N in 1 .. 65535; H and W divisible by 2^n_down; every layer's input and output below 2^31 elements; eps > 0; every
 * pointer but x 16-byte aligned.  Anything else is refused with KPN_EINVAL (the size queries return 0), kpn_last_error() names the field,
 * and nothing is launched.  Kernels: csrc/encoder_kernels.hip; dataflow: csrc/api_tex_train.hip.
 *   packed (kpn_res_encoder_packed_floats / _pack_device; they read only in_ch .. out_ch): per layer, in order, what the layer's own
 *            packer writes (kpn_conv2d_rp_pack_device / kpn_conv2d_s2_pack_device): the forward copy, then (not for the stem) the
 *            input-gradient copy.  weights[i]: the plain weight of layer i as the module holds it (OIHW; IOHW for a transposed layer).
 *   forward: the dataflow of kpn_tex_encode with nothing released - InstanceNorm statistics only, scale / shift and the ReLU applied
 *            inside the loads of the next convolution; a normalised tensor exists only where a residual needs it: a_0 = relu(norm(c)) in
 *            front of the first ResBlk and a_k = norm(c2) + a_{k-1} behind ResBlk k.  bias[i]: the bias of layer i.  y has the bits of the
 *            same encoder computed layer by layer (kpn_conv2d_rp_forward, kpn_conv2d_s2_forward, kpn_group_norm_forward, one fp32 add
 *            per ResBlk).
 *   state (kpn_res_encoder_state_floats = sum numel(c_i) + sum numel(a_k) + 4 N sum C_norm; written by the forward, read by the
 *            backward): the output c_i (NHWC) of every layer but the last, in order; then a_0 .. a_{n_blocks}; then, per layer but the
 *            last, scale [N][C], shift [N][C], mean [N][C], rstd [N][C] of the norm behind it.  No normalised tensor of a non-residual
 *            layer, no padded tensor.
 *   backward: dw[i] (the layout of weights[i]) and db[i] per layer, each of which may be NULL: nothing is written for a NULL result,
 *            and the walk ends at the lowest layer whose dw is wanted.  Results are overwritten, not accumulated.  There is no dx (the
 *            stem has no input gradient).  db[i] of every layer but the last is written as exact zeros and nothing is reduced for it: a
 *            bias in front of an InstanceNorm2d without parameters does not reach the output (IN(c + b) = IN(c)), where torch returns
 *            rounding noise.  db of the output layer is the sum of dy over the pixels.  Every layer's gradients are those of its own
 *            kpn_conv2d_*_backward and kpn_group_norm_backward, the norm and the ReLU recomputed in the loads of the weight gradient.
 * `workspace` (kpn_res_encoder_workspace_bytes; 0 = unsupported descriptor) serves the forward and the backward alike.
 * No float atomics: every result is bit-identical from run to run, and an image's y does not depend on its batch. */
typedef struct kpn_res_encoder_desc {
    int32_t N, H, W, in_ch, ngf, n_down, n_blocks, n_up, out_ch;
    float eps;
} kpn_res_encoder_desc;
int32_t kpn_res_encoder_layers(const kpn_res_encoder_desc* desc);
size_t kpn_res_encoder_workspace_bytes(const kpn_res_encoder_desc* desc);
size_t kpn_res_encoder_state_floats(const kpn_res_encoder_desc* desc);
size_t kpn_res_encoder_packed_floats(const kpn_res_encoder_desc* desc);
int kpn_res_encoder_pack_device(const kpn_res_encoder_desc* desc, const float* const* weights, float* packed, void* stream);
int kpn_res_encoder_forward(const kpn_res_encoder_desc* desc, const float* x, const float* packed, const float* const* bias, float* y,
                            float* state, void* workspace, size_t workspace_bytes, void* stream);
int kpn_res_encoder_backward(const kpn_res_encoder_desc* desc, const float* x, const float* dy, const float* packed, const float* state,
                             float* const* dw, float* const* db, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * A whole HGFilterV2(n_stack = 1, hd = False, norm = "group") (src/utils.py:322-414) for training, forward and backward, as one call
 * each: replaces the stem, every ConvBlock, the HourGlass with its pools and bicubic upsamples, unpack1 / conv_out, conv_last0 / bn_end0 /
 * l0, every fused norm + ReLU, and the sums autograd makes where a tensor has two consumers.
 * Layers: conv1 (7x7, stride 2, pad 3, in_ch -> c_stem, bias) + bn1 + ReLU; ConvBlocks conv2 (c_stem -> c2), [avg-pool 2], conv3
 * (c2 -> c3), conv4 (c3 -> c4); HourGlass(depth, c4); ConvBlock top_m_0 (c4 -> c4); conv_last0 (1x1, c4 -> c4, bias) + bn_end0 + ReLU;
 * l0 (1x1, c4 -> out_ch, bias).  The hd branch off the conv2 output: unpack1 = ConvTranspose2d(k 3, stride 2, pad 1, output_padding 1,
 * c2 -> c_hd, no bias) + GroupNorm + ReLU, conv_out (5x5, pad 2, c_hd -> out_ch_hd, bias).  Every norm is GroupNorm(min(32, C), C) with
 * parameters and the one eps.  The reference's instance is c_stem 64, c2 128, c3 128, c4 256, depth 4, c_hd 32.
 * x is the NCHW image (N, in_ch, H, W), read as it is (KPN_S2_STEM7); out (N, H/4, W/4, out_ch) and x_hd (N, H, W, out_ch_hd) are NHWC,
 * dense, fp32.
 * Scope: in_ch in 1 .. 4; every ConvBlock one that kpn_conv_block_* serves (so c_stem, c2 / 2 .. c4 / 4 powers of two >= 4); c_hd a
 * power of two in 4 .. 1024; out_ch, out_ch_hd multiples of 4 in 4 .. 1024; depth in 1 .. 8; H, W even with H / 2 and W / 2 divisible
 * by 2^(depth + 1); N in 1 .. 65535; every tensor below 2^31 elements; eps > 0; every pointer but x 16-byte aligned.  Anything else
 * is refused with KPN_EINVAL (the size queries return 0), kpn_last_error() names the field, and nothing is launched.  Kernels:
 * csrc/encoder_kernels.hip; dataflow: csrc/api_geo_train.hip.
 *   tensors (kpn_hg_filter_tensors of them), in this order: conv1 weight, bias; bn1 weight, bias; per ConvBlock in dataflow order -
 *            conv2, conv3, conv4, then per HourGlass level from the outermost in b1, b2, then the next level (b2_plus at the innermost),
 *            b3; top_m_0 - and per leg (bn1 / conv1, bn2 / conv2, bn3 / conv3 and, for cin != cout, bn4 / downsample) the norm's weight,
 *            its bias and the convolution's weight, 9 or 12 tensors; unpack1.conv weight; unpack1.norm weight, bias; conv_out weight,
 *            bias; conv_last0 weight, bias; bn_end0 weight, bias; l0 weight, bias.  Weights as the module holds them (OIHW; IOHW for
 *            unpack1.conv).
 *   params:  tensors[i] in that order - the forward and the backward read the norm parameters and the biases from it and never the plain
 *            convolution weights, whose entries may be NULL - and packed (kpn_hg_filter_packed_floats / _pack_device, which read only the
 *            widths, depth and in_ch / out_ch*): per convolution weight, in tensor order, what the layer's own packer writes
 *            (kpn_conv2d_s2_pack_device for conv1 and unpack1.conv, kpn_conv2d_pack_device for the others).
 *   forward: the dataflow of kpn_geo_encode with nothing released.  relu(bn1(conv1)) is materialised (it is a block input); unpack1.norm
 *            + ReLU runs inside the loads of conv_out and bn_end0 + ReLU inside the loads of l0; each HourGlass level's b1 output is
 *            overwritten in place by the skip sum.  out and x_hd have the bits of the same network computed operator by operator
 *            (kpn_conv2d_s2_forward, kpn_group_norm_forward(relu = 1), kpn_conv_block_forward, kpn_avg_pool2_forward,
 *            kpn_upsample2x_add_forward, kpn_conv2d_forward).
 *   state (kpn_hg_filter_state_floats; written by the forward, read by the backward), in this order, with (h1, w1) = (H/2, W/2),
 *            (h2, w2) = (H/4, W/4), S(block) = kpn_conv_block_state_floats of that block and stats(C) = 2 N C + 2 N min(32, C) (scale,
 *            shift, mean, rstd):
 *              conv1 output (N, h1, w1, c_stem); stats(c_stem) of bn1; relu(bn1(.)) (N, h1, w1, c_stem); S(conv2); the conv2 output
 *              (N, h1, w1, c2); the unpack1.conv output (N, H, W, c_hd); stats(c_hd) of unpack1.norm; the pooled conv2 output
 *              (N, h2, w2, c2); S(conv3); the conv3 output (N, h2, w2, c3); S(conv4); the conv4 output (N, h2, w2, c4); per HourGlass
 *              level from the outermost, on the level's grid (h, w): S(b1); the level's output b1(inp) + U(low3) (N, h, w, c4); the
 *              pooled input (N, h/2, w/2, c4); S(b2); the b2 output; the next level (or S(b2_plus) and its output); S(b3); then
 *              S(top_m_0); the top_m_0 output (N, h2, w2, c4); the conv_last0 output (N, h2, w2, c4); stats(c4) of bn_end0.
 *            kpn_hg_filter_state_floats is the sum of these.  out, x_hd, the b3 outputs, the un-summed b1 outputs and every normalised
 *            tensor but relu(bn1(.)) are not kept.
 *   backward: d_out (N, H/4, W/4, out_ch) and d_x_hd (N, H, W, out_ch_hd), NHWC; either may be NULL (that branch contributes nothing), not
 *            both.  grads[i] per tensor in tensor order, each of which may be NULL: nothing is written for a NULL result, only the legs
 *            that a wanted gradient needs are launched, and the walk ends at the lowest layer whose gradient is wanted.  Results are
 *            overwritten, not accumulated.  There is no input gradient (the stem has none).  Every layer's gradients are those of its own
 *            single-layer backward (kpn_conv2d_backward, kpn_conv2d_s2_backward, kpn_group_norm_backward, kpn_conv_block_backward,
 *            kpn_upsample2x_add_backward), the norm and the ReLU recomputed in the loads of the weight gradients of conv_out and l0, the
 *            norm gradients in place.  Where a tensor has two consumers - the input of an HourGlass level (b1 and the pool), the conv2
 *            output (unpack1.conv and the pool) - the other consumer's gradient is written first and complete, then
 *            0.25 g_low[y / 2][x / 2] is added onto it (k_enc_pool2_bwd_acc): one fp32 add of two finished values, the bits of
 *            kpn_avg_pool2_backward followed by a tensor add in either order.
 * `workspace` (kpn_hg_filter_workspace_bytes; 0 = unsupported descriptor) serves the forward and the backward alike.
 * No float atomics: every result is bit-identical from run to run, and an image's results do not depend on its batch. */
typedef struct kpn_hg_filter_desc {
    int32_t N, H, W, in_ch, c_stem, c2, c3, c4, depth, c_hd, out_ch_hd, out_ch;
    float eps;
} kpn_hg_filter_desc;
typedef struct kpn_hg_filter_params {
    const float* const* tensors;      /* kpn_hg_filter_tensors entries, in tensor order */
    const float* packed;              /* kpn_hg_filter_pack_device */
} kpn_hg_filter_params;
typedef struct kpn_hg_filter_grads {
    float* const* tensors;            /* kpn_hg_filter_tensors entries, in tensor order; any may be NULL */
} kpn_hg_filter_grads;
int32_t kpn_hg_filter_tensors(const kpn_hg_filter_desc* desc);
size_t kpn_hg_filter_workspace_bytes(const kpn_hg_filter_desc* desc);
size_t kpn_hg_filter_state_floats(const kpn_hg_filter_desc* desc);
size_t kpn_hg_filter_packed_floats(const kpn_hg_filter_desc* desc);
int kpn_hg_filter_pack_device(const kpn_hg_filter_desc* desc, const float* const* tensors, float* packed, void* stream);
int kpn_hg_filter_forward(const kpn_hg_filter_desc* desc, const float* x, const kpn_hg_filter_params* params, float* out, float* x_hd,
                          float* state, void* workspace, size_t workspace_bytes, void* stream);
int kpn_hg_filter_backward(const kpn_hg_filter_desc* desc, const float* x, const float* d_out, const float* d_x_hd,
                           const kpn_hg_filter_params* params, const float* state, const kpn_hg_filter_grads* grads, void* workspace,
                           size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* KPNERF_H */

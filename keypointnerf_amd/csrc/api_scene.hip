// ---------------------------------------------------------------------------------------------
// scene
namespace {
struct SceneLayout { size_t table, rgbm, geo0, geo1, tex, flags, total; };  // float offsets
SceneLayout scene_layout(const kpn_scene_desc* d) {
    SceneLayout L;
    Carver c;   // in floats, blocks of 64
    L.table = c.take((size_t)d->n_views * KPN_TBL_STRIDE, 64);
    L.rgbm = c.take((size_t)d->n_views * d->src_h * d->src_w * 4, 64);
    L.geo0 = c.take((size_t)d->n_views * d->geo0_h * d->geo0_w * 64, 64);
    L.geo1 = c.take((size_t)d->n_views * d->geo1_h * d->geo1_w * 8, 64);
    L.tex = c.take((size_t)d->n_views * d->tex_h * d->tex_w * 8, 64);
    L.flags = c.take((size_t)KPN_SCENE_FLAG_FLOATS, 64);   // [0] = max |value| of the images and maps (kpn_common.h)
    L.total = c.o;
    return L;
}
int check_desc(const kpn_scene_desc* d) {
    KPN_REQUIRE(d != nullptr, "scene desc is null");
    KPN_REQUIRE(d->n_views >= 1 && d->n_views <= KPN_MAX_VIEWS, "n_views out of range");
    KPN_REQUIRE(d->src_h > 1 && d->src_w > 1 && d->geo0_h > 1 && d->geo0_w > 1 && d->geo1_h > 1 && d->geo1_w > 1 &&
                d->tex_h > 1 && d->tex_w > 1, "map sizes must be > 1");
    KPN_REQUIRE((int64_t)d->src_h * d->src_w <= INT32_MAX && (int64_t)d->geo0_h * d->geo0_w <= INT32_MAX &&
                (int64_t)d->geo1_h * d->geo1_w <= INT32_MAX && (int64_t)d->tex_h * d->tex_w <= INT32_MAX, "map too large");
    KPN_REQUIRE(d->zfar > d->znear && d->nml_scale > 0.0f && d->sigma > 0.0f, "bad scalar parameters");
    KPN_REQUIRE(d->KRT && d->extrin && d->kpt3d && d->img && d->geo0 && d->geo1 && d->tex, "null scene tensor");
    KPN_REQUIRE(d->disable_fg_mask || d->fg_mask, "fg_mask is null");
    return KPN_OK;
}
kpn_scene_dev scene_dev(const kpn_scene_desc* d, const void* ws) {
    const SceneLayout L = scene_layout(d);
    const float* base = static_cast<const float*>(ws);
    kpn_scene_dev s;
    s.V = d->n_views; s.H = d->src_h; s.W = d->src_w;
    s.g0h = d->geo0_h; s.g0w = d->geo0_w; s.g1h = d->geo1_h; s.g1w = d->geo1_w; s.th = d->tex_h; s.tw = d->tex_w;
    s.disable_fg_mask = d->disable_fg_mask;
    s.znear = d->znear; s.zfar = d->zfar; s.nml_scale = d->nml_scale;
    s.two_sigma2 = (float)(2.0 * ((double)d->sigma * (double)d->sigma));  // spatial.py:114
    s.keep = 0xFFFFFFFFu;
    s.table = base + L.table; s.rgbm = base + L.rgbm; s.geo0 = base + L.geo0; s.geo1 = base + L.geo1; s.tex = base + L.tex;
    s.flags = base + L.flags;
    return s;
}
}  // namespace

extern "C" size_t kpn_scene_workspace_bytes(const kpn_scene_desc* d) {
    if (check_desc(d) != KPN_OK) return 0;
    return scene_layout(d).total * sizeof(float);
}

extern "C" int kpn_scene_layout(const kpn_scene_desc* d, size_t offsets[6]) {
    if (int e = check_desc(d)) return e;
    KPN_REQUIRE(offsets != nullptr, "offsets is null");
    const SceneLayout L = scene_layout(d);
    offsets[0] = L.table; offsets[1] = L.rgbm; offsets[2] = L.geo0; offsets[3] = L.geo1; offsets[4] = L.tex; offsets[5] = L.flags;
    return KPN_OK;
}

extern "C" int kpn_scene_prepare(const kpn_scene_desc* d, void* scene_ws, void* stream) {
    return kpn_scene_prepare_kpt(d, KPN_NKPT, scene_ws, stream);
}

extern "C" int kpn_scene_prepare_kpt(const kpn_scene_desc* d, int32_t n_kpt, void* scene_ws, void* stream) {
    if (int e = check_desc(d)) return e;
    KPN_REQUIRE(n_kpt >= 1 && n_kpt <= KPN_NKPT, "n_kpt out of range: the field kernels hold 1..24 keypoints (KPN_N_KPT)");
    KPN_REQUIRE(scene_ws != nullptr, "scene workspace is null");
    const SceneLayout L = scene_layout(d);
    float* base = static_cast<float*>(scene_ws);
    const int V = d->n_views;
    float* flags = base + L.flags;   // zeroed by k_scene_table (first on the stream), raised by the copies behind it
    KPN_LAUNCH(k_scene_table, dim3(V), dim3(128), stream, V, (int)n_kpt, d->KRT, d->extrin, d->kpt3d, base + L.table, flags);
    const int HW = d->src_h * d->src_w;
    const int ptiles = (HW + KPN_PACK_PIX - 1) / KPN_PACK_PIX;
    KPN_LAUNCH(k_pack_rgbm, dim3(V * ptiles), dim3(256), stream, HW, ptiles, d->img,
               d->disable_fg_mask ? (const uint8_t*)nullptr : d->fg_mask, base + L.rgbm, flags);
    // float4 loads of a channel's run: every run starts 16-byte aligned
    auto vec = [](const float* p, int hw) { return (hw % 4 == 0 && reinterpret_cast<uintptr_t>(p) % 16 == 0) ? 1 : 0; };
    const int hw0 = d->geo0_h * d->geo0_w, hw1 = d->geo1_h * d->geo1_w, hwt = d->tex_h * d->tex_w;
    const int t0 = (hw0 + KPN_NHWC_TILE / 64 - 1) / (KPN_NHWC_TILE / 64), t1 = (hw1 + KPN_NHWC_TILE / 8 - 1) / (KPN_NHWC_TILE / 8),
              tt = (hwt + KPN_NHWC_TILE / 8 - 1) / (KPN_NHWC_TILE / 8);
    KPN_LAUNCH(k_nchw_to_nhwc<64>, dim3(V * t0), dim3(256), stream, hw0, t0, vec(d->geo0, hw0), d->geo0, base + L.geo0, flags);
    KPN_LAUNCH(k_nchw_to_nhwc<8>, dim3(V * t1), dim3(256), stream, hw1, t1, vec(d->geo1, hw1), d->geo1, base + L.geo1, flags);
    KPN_LAUNCH(k_nchw_to_nhwc<8>, dim3(V * tt), dim3(256), stream, hwt, tt, vec(d->tex, hwt), d->tex, base + L.tex, flags);
    return check_launch("kpn_scene_prepare");
}

// ---------------------------------------------------------------------------------------------
// stage ops
extern "C" int kpn_ray_bbox_intersection(const float* bounds, const float* orig, const float* direct, int64_t R,
                                         float* near_o, float* far_o, uint8_t* hit_o, void* stream) {
    KPN_REQUIRE(bounds && orig && direct && near_o && far_o && hit_o, "null pointer");
    KPN_REQUIRE(R >= 0, "negative ray count");
    if (R == 0) return KPN_OK;
    KPN_LAUNCH(k_ray_bbox, grid1d(R, 256), dim3(256), stream, R, bounds, orig, direct, near_o, far_o, hit_o);
    return check_launch("kpn_ray_bbox_intersection");
}

extern "C" int kpn_make_rays(const float* K, const float* RT, float znear, float zfar, const float* bounds, int32_t x0,
                             int32_t y0, int32_t step, int32_t nx, int32_t ny, float* dirs, float* cam_pos,
                             float* near_o, float* far_o, void* stream) {
    KPN_REQUIRE(K && RT && bounds && dirs && cam_pos && near_o && far_o, "null pointer");
    KPN_REQUIRE(nx > 0 && ny > 0 && step > 0, "bad pixel grid");
    KPN_LAUNCH(k_make_rays, grid1d((int64_t)nx * ny, 256), dim3(256), stream, K, RT, znear, zfar, bounds, (int)x0, (int)y0,
               (int)step, (int)step, (int)nx, (int)ny, (const int*)nullptr, dirs, cam_pos, near_o, far_o);
    return check_launch("kpn_make_rays");
}

extern "C" int kpn_importance_sample(const float* contrib, const float* z, const float* u, int64_t R, int32_t Dm2,
                                     int32_t n, float* out, void* stream) {
    KPN_REQUIRE(contrib && z && out, "null pointer");
    KPN_REQUIRE(Dm2 >= 1 && Dm2 + 1 <= KPN_IS_MAXD, "bin count out of range (<= 128)");
    KPN_REQUIRE(n >= 1 && R >= 0, "bad sizes");
    if (R == 0) return KPN_OK;
    KPN_LAUNCH(k_importance, grid1d(R, 64), dim3(64), stream, R, (int)Dm2, (int)n, contrib, z, u, out);
    return check_launch("kpn_importance_sample");
}

// compositor launch: the kernel is specialised by samples per lane (ceil(S / 64)) so that the double-buffered ray
// state stays in few registers
static void launch_rgba2out(void* stream, int64_t R, int S, const float* rgba, const float* z, float* color, float* depth,
                            float* alpha, float* contrib, float* sdf, const int16_t* src, const float* rgba_new, int Sc) {
    const int64_t blocks = (R + 3) / 4;  // 4 waves per block, one ray per wave per iteration
    const dim3 grid((unsigned)(blocks < 8192 ? blocks : 8192));
    const int per = (S + 63) / 64;
    if (per <= 1) KPN_LAUNCH(k_rgba2out<1>, grid, dim3(256), stream, R, S, rgba, z, color, depth, alpha, contrib, sdf, src, rgba_new, Sc);
    else if (per <= 2) KPN_LAUNCH(k_rgba2out<2>, grid, dim3(256), stream, R, S, rgba, z, color, depth, alpha, contrib, sdf, src, rgba_new, Sc);
    else if (per <= 4) KPN_LAUNCH(k_rgba2out<4>, grid, dim3(256), stream, R, S, rgba, z, color, depth, alpha, contrib, sdf, src, rgba_new, Sc);
    else KPN_LAUNCH(k_rgba2out<KPN_MAX_PER_LANE>, grid, dim3(256), stream, R, S, rgba, z, color, depth, alpha, contrib, sdf, src, rgba_new, Sc);
}

extern "C" int kpn_rgba2out(const float* rgba, const float* z, int64_t R, int32_t S, float* color, float* depth,
                            float* alpha, float* contrib, float* sdf, void* stream) {
    KPN_REQUIRE(rgba && z && color && depth && alpha && sdf, "null pointer");
    KPN_REQUIRE(S >= 1 && S <= 64 * KPN_MAX_PER_LANE, "samples per ray out of range (<= 512)");
    if (R <= 0) return R == 0 ? KPN_OK : fail(KPN_EINVAL, "negative ray count");
    launch_rgba2out(stream, R, (int)S, rgba, z, color, depth, alpha, contrib, sdf, nullptr, nullptr, 0);
    return check_launch("kpn_rgba2out");
}
// compositor over the merged list of the fine pass, read in place from the coarse and the new samples' records
static int rgba2out_merged(const float* rgba_c, const float* rgba_n, const int16_t* src, const float* z, int64_t R, int Sc, int Sf,
                           float* color, float* depth, float* alpha, float* sdf, void* stream) {
    launch_rgba2out(stream, R, Sc + Sf, rgba_c, z, color, depth, alpha, nullptr, sdf, src, rgba_n, Sc);
    return check_launch("kpn_render_rays");
}

extern "C" int kpn_rgba2out_backward(const float* rgba, const float* z, int64_t R, int32_t S, const float* d_color,
                                     const float* d_depth, const float* d_alpha, const float* d_sdf, float* d_rgba, void* stream) {
    KPN_REQUIRE(rgba && z && d_rgba, "null pointer");
    KPN_REQUIRE(S >= 1, "bad sample count");
    if (R <= 0) return R == 0 ? KPN_OK : fail(KPN_EINVAL, "negative ray count");
    const int per = (int)((S + 63) / 64);   // more than 512 samples per ray: one thread per ray
    const dim3 wgrid = grid1d(R * 64, 256);   // one wavefront per ray
    if (per <= 1) KPN_LAUNCH(k_rgba2out_bwd_w<1>, wgrid, dim3(256), stream, R, (int)S, rgba, z, d_color, d_depth, d_alpha, d_sdf, d_rgba);
    else if (per <= 2) KPN_LAUNCH(k_rgba2out_bwd_w<2>, wgrid, dim3(256), stream, R, (int)S, rgba, z, d_color, d_depth, d_alpha, d_sdf, d_rgba);
    else if (per <= 4) KPN_LAUNCH(k_rgba2out_bwd_w<4>, wgrid, dim3(256), stream, R, (int)S, rgba, z, d_color, d_depth, d_alpha, d_sdf, d_rgba);
    else if (per <= 8) KPN_LAUNCH(k_rgba2out_bwd_w<8>, wgrid, dim3(256), stream, R, (int)S, rgba, z, d_color, d_depth, d_alpha, d_sdf, d_rgba);
    else KPN_LAUNCH(k_rgba2out_bwd, grid1d(R, 64), dim3(64), stream, R, (int)S, rgba, z, d_color, d_depth, d_alpha, d_sdf, d_rgba);
    return check_launch("kpn_rgba2out_backward");
}

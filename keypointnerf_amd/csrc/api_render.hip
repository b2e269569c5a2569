// ---------------------------------------------------------------------------------------------
// hierarchical render
namespace {
struct RenderLayout { size_t cam_pos, dirs, nearv, farv, zc, zf, zn, src, rgba, rgba_c, rgba_n, contrib, color, depth, alpha, sdf, query, total; int64_t chunk; };
int64_t pick_chunk(const kpn_scene_desc* d, const kpn_render_args* a) {
    // default: passes of up to 262144 rays (one per 512^2 frame) — large passes amortise launch ramps and the per-workgroup
    // weight staging of the persistent field kernels (measured per 512^2 frame: 65536 rays/pass 33.6 ms, 131072 33.3 ms,
    // 262144 32.2 ms).  The row scratch no longer scales with the pass: it is capped (query_layout) and reused by batches.
    const int64_t R = (int64_t)a->nx * a->ny;
    int64_t c = a->chunk_rays;
    if (c <= 0) {
        const int64_t cmax = 262144;
        const int64_t npass = (R + cmax - 1) / cmax;
        c = ((R + npass - 1) / npass + 63) / 64 * 64;
    }
    return c < R ? c : R;
}
RenderLayout render_layout(const kpn_scene_desc* d, const kpn_render_args* a) {
    RenderLayout L;
    const int64_t R = (int64_t)a->nx * a->ny;
    const int64_t C = pick_chunk(d, a);
    const int64_t Sfull = a->n_coarse + (a->fine ? a->n_fine : 0);
    Carver c;
    L.chunk = C;
    L.cam_pos = c.take(64);
    L.dirs = c.take((size_t)R * 3 * 4);
    L.nearv = c.take((size_t)R * 4);
    L.farv = c.take((size_t)R * 4);
    L.zc = c.take((size_t)C * a->n_coarse * 4);
    L.zf = c.take((size_t)C * Sfull * 4);
    L.rgba = c.take((size_t)C * Sfull * 5 * 4);
    // eval with coarse re-use (the default): the coarse values kept for the fine pass and the values at the new samples share the
    // block a pass without re-use fills as a whole — never both in one call (round 6: 671 MB less per 512 x 512 plan)
    L.rgba_c = L.rgba;
    L.rgba_n = L.rgba + align_up((size_t)C * a->n_coarse * 5 * 4, 256);
    c.o += 256;                                                        // (the alignment of rgba_n inside the block)
    L.zn = c.take((size_t)C * (a->fine ? a->n_fine : 0) * 4);
    L.src = c.take((size_t)C * Sfull * sizeof(int16_t));
    L.contrib = c.take((size_t)C * a->n_coarse * 4);                    // the coarse compositor's weights (the fine one writes none)
    L.color = c.take((size_t)C * 3 * 4);
    L.depth = c.take((size_t)C * 4);
    L.alpha = c.take((size_t)C * 4);
    L.sdf = c.take((size_t)C * 4);
    {   // eval passes use the POOL layout of the scratch, the train branch (same workspace) the ROWS layout: room for either
        const size_t qa = query_layout(C * Sfull, d->n_views, false).total, qb = query_layout(C * Sfull, d->n_views, pool_layout_selected()).total;
        L.query = c.take(qa > qb ? qa : qb);
    }
    L.total = c.o;
    return L;
}
int check_render(const kpn_render_args* a) {
    KPN_REQUIRE(a != nullptr, "render args null");
    KPN_REQUIRE(a->K && a->RT && a->bounds, "null camera/bounds");
    KPN_REQUIRE(a->nx > 0 && a->ny > 0 && a->step > 0 && a->step_y >= 0, "bad pixel grid");
    KPN_REQUIRE(a->rows_kernel >= 0 && a->rows_kernel <= KPN_ROWS_F16X2 && a->fuse_kernel >= 0 && a->fuse_kernel <= KPN_FUSE_F16X2, "bad kernel selection");
    KPN_REQUIRE(a->n_coarse >= 3 && a->n_coarse <= 128, "sample_per_ray_c must be in [3,128]");
    KPN_REQUIRE(!a->fine || (a->n_fine >= 1 && a->n_fine <= 128), "sample_per_ray_f must be in [1,128]");
    KPN_REQUIRE((int64_t)a->nx * a->ny < (1ll << 31), "too many rays");
    return KPN_OK;
}
// the random draws of the train branch; need_fine: the call renders coarse + fine only (the backward entry points)
int check_train(const kpn_scene_desc* d, const kpn_render_args* a, const kpn_train_args* t, bool need_fine) {
    KPN_REQUIRE(t != nullptr, "train args null");
    KPN_REQUIRE(a->fine || !need_fine, "the train branch renders coarse + fine (dr_kwargs.fine)");
    KPN_REQUIRE(t->pix && t->u_coarse, "train args: pix and u_coarse are required");
    KPN_REQUIRE(!a->fine || t->u_fine, "train args: u_fine is required when fine");
    KPN_REQUIRE(t->rand_noise_std == 0.0f || (t->noise_coarse && (!a->fine || t->noise_fine)), "train args: noise tensors missing");
    KPN_REQUIRE((t->keep_coarse & ((1u << d->n_views) - 1u)) && (t->keep_fine & ((1u << d->n_views) - 1u)),
                "train args: view dropout must keep at least one view (reference src/model.py:744)");
    return KPN_OK;
}
}  // namespace

// scatter of per-chunk (rays, C) results into the planar (C, ny*nx) outputs
__global__ void k_store_planar(int64_t r0, int64_t n, int64_t R, int C, const float* __restrict__ src, float* __restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * C) return;
    const int64_t r = i / C;
    const int c = (int)(i - r * C);
    dst[(int64_t)c * R + r0 + r] = src[i];
}
// gather of a chunk's upstream gradients from the planar (C, R) layout the outputs use; src == nullptr -> zeros
__global__ void k_load_planar(int64_t r0, int64_t n, int64_t R, int C, const float* __restrict__ src, float* __restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * C) return;
    const int64_t r = i / C;
    const int c = (int)(i - r * C);
    dst[i] = src ? src[(int64_t)c * R + r0 + r] : 0.0f;
}
// rays [r0, r0 + n) of R: an output the caller did not ask for (dst == nullptr) is not stored
struct PlanarChunk {
    void* stream; int64_t r0, n, R;
    void store(float* dst, const float* src, int C) const {
        if (dst) KPN_LAUNCH(k_store_planar, grid1d(n * C, 256), dim3(256), stream, r0, n, R, C, src, dst);
    }
    void load(float* dst, const float* src, int C) const {
        KPN_LAUNCH(k_load_planar, grid1d(n * C, 256), dim3(256), stream, r0, n, R, C, src, dst);
    }
};

extern "C" size_t kpn_render_workspace_bytes(const kpn_scene_desc* d, const kpn_render_args* a) {
    if (check_desc(d) != KPN_OK || check_render(a) != KPN_OK) return 0;
    return render_layout(d, a).total;
}

// shared implementation: t == nullptr -> eval branch (model.py:1019-1022, uniform=True); otherwise the train
// branch with explicit random draws
// importance samples of the fine pass + the merged depth list (k_fine_samples_w), Sc, Sf <= 128
static void launch_fine_samples(void* stream, int64_t n, int Sc, int Sf, const float* zc, const float* contrib,
                                const float* u, float* zf, float* znew, int16_t* src) {
    const bool small = Sc <= 64 && Sf <= 64;
    const int64_t per = 4 * KPN_FINE_GROUP(small);   // rays of a workgroup: four wavefronts, a group each
    const dim3 grid((unsigned)((n + per - 1) / per < 8192 ? (n + per - 1) / per : 8192));
    if (small)
        KPN_LAUNCH(k_fine_samples_w<true>, grid, dim3(256), stream, n, Sc, Sf, zc, contrib, u, zf, znew, src);
    else
        KPN_LAUNCH(k_fine_samples_w<false>, grid, dim3(256), stream, n, Sc, Sf, zc, contrib, u, zf, znew, src);
}

static int render_impl(const kpn_scene_desc* d, const void* scene_ws, const float* wp, const kpn_render_args* a,
                       const kpn_train_args* t, void* ws, size_t ws_bytes, void* stream) {
    if (int e = check_desc(d)) return e;
    if (int e = check_render(a)) return e;
    KPN_REQUIRE(scene_ws && wp && ws, "null pointer");
    if (t) if (int e = check_train(d, a, t, false)) return e;
    const RenderLayout L = render_layout(d, a);
    if (ws_bytes < L.total) return fail(KPN_EWORKSPACE, "render workspace too small");
    char* base = static_cast<char*>(ws);
    auto F = [&](size_t off) { return reinterpret_cast<float*>(base + off); };
    kpn_scene_dev sc = scene_dev(d, scene_ws);
    const int64_t R = (int64_t)a->nx * a->ny;
    const int Sc = a->n_coarse, Sf = a->fine ? a->n_fine : 0, Sfull = Sc + Sf;
    KPN_LAUNCH(k_make_rays, grid1d(R, 256), dim3(256), stream, a->K, a->RT, a->znear, a->zfar, a->bounds, (int)a->x0, (int)a->y0,
               (int)a->step, (int)(a->step_y > 0 ? a->step_y : a->step), (int)a->nx, (int)a->ny, t ? (const int*)t->pix : (const int*)nullptr, F(L.dirs), F(L.cam_pos),
               F(L.nearv), F(L.farv));
    for (int64_t r0 = 0; r0 < R; r0 += L.chunk) {
        const int64_t n = (R - r0) < L.chunk ? (R - r0) : L.chunk;
        const float* dirs = F(L.dirs) + r0 * 3;
        const PlanarChunk pl{stream, r0, n, R};
        KPN_LAUNCH(k_coarse_z, grid1d(n * Sc, 256), dim3(256), stream, n, Sc, (const float*)(F(L.nearv) + r0),
                   (const float*)(F(L.farv) + r0), t ? t->u_coarse + r0 * Sc : (const float*)nullptr, F(L.zc));
        kpn_points ps{nullptr, nullptr, F(L.cam_pos), dirs, F(L.zc), Sc,
                      (t && t->rand_noise_std != 0.0f) ? t->noise_coarse + r0 * Sc : nullptr, t ? t->rand_noise_std : 0.0f};
        sc.keep = t ? t->keep_coarse : 0xFFFFFFFFu;
        // eval: the fine pass re-uses the coarse samples' field values (identical points, no dropout, no noise: identical
        // deterministic results) and evaluates the field at the new samples only — 128 instead of 192 evaluations per ray
        // at 64 + 64 samples.  The train branch draws fresh dropout masks and noise for the fine query and cannot.
        const char* nr = getenv("KPN_NO_COARSE_REUSE");  // A/B knob (read per call: tests flip it)
        const bool no_reuse = nr && atoi(nr);
        const bool reuse = (t == nullptr) && a->fine && !no_reuse;
        float* rgba_coarse = reuse ? F(L.rgba_c) : F(L.rgba);
        const int allow_pool = t == nullptr;   // eval: pooled inside the rows kernel; the train branch keeps the per-view rows
        if (int e = run_field(sc, ps, wp, n * Sc, 1, rgba_coarse, nullptr, base + L.query, stream, 1, 0, allow_pool, a->rows_kernel, a->fuse_kernel)) return e;   // model.py:1062
        if (int e = kpn_rgba2out(rgba_coarse, F(L.zc), n, Sc, F(L.color), F(L.depth), F(L.alpha), F(L.contrib), F(L.sdf), stream)) return e;
        const kpn_render_stages* st = a->stages;
        auto copy_out = [&](float* dst, const float* src_, size_t floats) {   // device to device, on the call's stream
#ifndef KPN_SIMT_EMU
            (void)hipMemcpyAsync(dst, src_, floats * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream);
#else
            memcpy(dst, src_, floats * sizeof(float));
#endif
        };
        if (st && st->dirs) copy_out(st->dirs + r0 * 3, dirs, (size_t)n * 3);
        if (st && st->cam_pos && r0 == 0) copy_out(st->cam_pos, F(L.cam_pos), 3);
        if (st && st->z_coarse) copy_out(st->z_coarse + r0 * Sc, F(L.zc), (size_t)n * Sc);
        if (st && st->rgba_coarse) copy_out(st->rgba_coarse + r0 * Sc * 5, rgba_coarse, (size_t)n * Sc * 5);
        pl.store(a->tex_fg, F(L.color), 3);
        pl.store(a->depth, F(L.depth), 1);
        pl.store(a->alpha, F(L.alpha), 1);
        if (a->fine) {
            const float* uf = t ? t->u_fine + r0 * Sf : (const float*)nullptr;
            float* zn = reuse ? F(L.zn) : nullptr;
            int16_t* src = reuse ? reinterpret_cast<int16_t*>(base + L.src) : nullptr;
            launch_fine_samples(stream, n, Sc, Sf, F(L.zc), F(L.contrib), uf, F(L.zf), zn, src);
            sc.keep = t ? t->keep_fine : 0xFFFFFFFFu;
            if (reuse) {
                kpn_points pn{nullptr, nullptr, F(L.cam_pos), dirs, F(L.zn), Sf, nullptr, 0.0f};
                if (int e = run_field(sc, pn, wp, n * Sf, 1, F(L.rgba_n), nullptr, base + L.query, stream, 1, 0, allow_pool, a->rows_kernel, a->fuse_kernel)) return e;  // :1082, new samples
                if (int e = rgba2out_merged(F(L.rgba_c), F(L.rgba_n), src, F(L.zf), n, Sc, Sf, F(L.color), F(L.depth), F(L.alpha), F(L.sdf), stream)) return e;
            } else {
                kpn_points pf{nullptr, nullptr, F(L.cam_pos), dirs, F(L.zf), Sfull,
                              (t && t->rand_noise_std != 0.0f) ? t->noise_fine + r0 * Sfull : nullptr, t ? t->rand_noise_std : 0.0f};
                if (int e = run_field(sc, pf, wp, n * Sfull, 1, F(L.rgba), nullptr, base + L.query, stream, 1, 0, allow_pool, a->rows_kernel, a->fuse_kernel)) return e;  // :1082
                if (int e = kpn_rgba2out(F(L.rgba), F(L.zf), n, Sfull, F(L.color), F(L.depth), F(L.alpha), nullptr, F(L.sdf), stream)) return e;
            }
            if (st && st->z_fine) copy_out(st->z_fine + r0 * Sfull, F(L.zf), (size_t)n * Sfull);
            if (st && st->rgba_fine) {
                if (reuse) KPN_LAUNCH(k_merge_rgba, grid1d(n * Sfull, 256), dim3(256), stream, n, Sfull, Sc, (const float*)F(L.rgba_c), (const float*)F(L.rgba_n),
                                      (const int16_t*)src, st->rgba_fine + r0 * Sfull * 5);
                else copy_out(st->rgba_fine + r0 * Sfull * 5, F(L.rgba), (size_t)n * Sfull * 5);
            }
            pl.store(a->tex_fg_fine, F(L.color), 3);
            pl.store(a->depth_fine, F(L.depth), 1);
            pl.store(a->alpha_fine, F(L.alpha), 1);
            pl.store(a->sdf, F(L.sdf), 1);
        }
    }
    return check_launch("kpn_render_rays");
}

extern "C" int kpn_render_rays(const kpn_scene_desc* d, const void* scene_ws, const float* wp, const kpn_render_args* a,
                               void* ws, size_t ws_bytes, void* stream) {
    return render_impl(d, scene_ws, wp, a, nullptr, ws, ws_bytes, stream);
}
extern "C" int kpn_render_rays_train(const kpn_scene_desc* d, const void* scene_ws, const float* wp, const kpn_render_args* a,
                                     const kpn_train_args* t, void* ws, size_t ws_bytes, void* stream) {
    KPN_REQUIRE(t != nullptr, "train args null");
    return render_impl(d, scene_ws, wp, a, t, ws, ws_bytes, stream);
}

// ---------------------------------------------------------------------------------------------
// backward of the train-branch render
namespace {
struct TrainBwdLayout { size_t cam_pos, dirs, nearv, farv, zc, zf, rgba_c, rgba_f, contrib, scratch, g3, g1a, g1b, g1c, drgba_c, drgba_f,
                        query, bwd, total; int64_t chunk; };
TrainBwdLayout train_bwd_layout(const kpn_scene_desc* d, const kpn_render_args* a) {
    TrainBwdLayout L;
    const int64_t R = (int64_t)a->nx * a->ny;
    const int64_t Sfull = a->n_coarse + a->n_fine;
    int64_t C = a->chunk_rays > 0 ? a->chunk_rays : kBwdChunk / Sfull;   // one backward pass per point set
    if (C * Sfull > kBwdChunk) C = kBwdChunk / Sfull;
    if (C > R) C = R;
    L.chunk = C;
    Carver c;
    L.cam_pos = c.take(64);
    L.dirs = c.take((size_t)R * 3 * 4); L.nearv = c.take((size_t)R * 4); L.farv = c.take((size_t)R * 4);
    L.zc = c.take((size_t)C * a->n_coarse * 4); L.zf = c.take((size_t)C * Sfull * 4);
    L.rgba_c = c.take((size_t)C * a->n_coarse * 5 * 4); L.rgba_f = c.take((size_t)C * Sfull * 5 * 4);
    L.contrib = c.take((size_t)C * (Sfull > 8 ? Sfull : 8) * 4);
    L.scratch = c.take((size_t)C * 8 * 4);  // colour / depth / alpha / sdf of the recomputed forward (unused results)
    L.g3 = c.take((size_t)C * 3 * 4); L.g1a = c.take((size_t)C * 4); L.g1b = c.take((size_t)C * 4); L.g1c = c.take((size_t)C * 4);
    L.drgba_c = c.take((size_t)C * a->n_coarse * 5 * 4); L.drgba_f = c.take((size_t)C * Sfull * 5 * 4);
    L.query = c.take(query_layout(C * Sfull, d->n_views).total);
    L.bwd = c.take(bwd_layout(C * Sfull, d->n_views, 2).total);
    L.total = c.o;
    return L;
}
}  // namespace

// State a train-branch forward call can leave behind for its backward call (kpn_render_rays_train_keep): rays, and per
// chunk of rays the depths, the field values and — the expensive part — the valid lists and (point, view) rows of both
// field passes.  With it the backward call skips the forward it otherwise repeats (k_make_rays, k_coarse_z, 2 x
// k_mask_compact + k_geo_rows + k_fuse_color, compositor, sampler: 1.05 of 9.1 ms at 1024 rays x 192 samples).
namespace {
struct TrainStateLayout { size_t cam_pos, dirs, nearv, farv, chunk0, zc, zf, rgba_c, rgba_f, contrib, query_c, query_f, chunk_bytes, total;
                          int64_t chunk, nchunks; };
TrainStateLayout train_state_layout(const kpn_scene_desc* d, const kpn_render_args* a) {
    TrainStateLayout S;
    const TrainBwdLayout L = train_bwd_layout(d, a);
    const int64_t R = (int64_t)a->nx * a->ny, C = L.chunk;
    const int64_t Sfull = a->n_coarse + a->n_fine;
    S.chunk = C; S.nchunks = (R + C - 1) / C;
    Carver c;
    S.cam_pos = c.take(64);
    S.dirs = c.take((size_t)R * 3 * 4); S.nearv = c.take((size_t)R * 4); S.farv = c.take((size_t)R * 4);
    S.chunk0 = c.o;
    c = Carver();   // offsets inside one chunk block
    S.zc = c.take((size_t)C * a->n_coarse * 4); S.zf = c.take((size_t)C * Sfull * 4);
    S.rgba_c = c.take((size_t)C * a->n_coarse * 5 * 4); S.rgba_f = c.take((size_t)C * Sfull * 5 * 4);
    S.contrib = c.take((size_t)C * (Sfull > 8 ? Sfull : 8) * 4);   // also stages the fine composite of a forward call (6 floats per ray)
    S.query_c = c.take(query_layout(C * a->n_coarse, d->n_views).total);
    S.query_f = c.take(query_layout(C * Sfull, d->n_views).total);
    S.chunk_bytes = c.o;
    S.total = S.chunk0 + S.chunk_bytes * (size_t)S.nchunks;
    return S;
}

// one implementation, three uses: state == nullptr: the classic backward (forward repeated inside `ws`);
// forward_only: fills `state` and writes the outputs of `a` (kpn_render_rays_train_keep); otherwise: backward from `state`
int train_impl(const kpn_scene_desc* d, const void* scene_ws, const float* wp, const kpn_render_args* a, const kpn_train_args* t,
               const kpn_render_grads* g, float* d_plain, float* d_geo0, float* d_geo1, float* d_tex, void* state, size_t state_bytes,
               bool forward_only, void* ws, size_t ws_bytes, void* stream) {
    if (int e = check_desc(d)) return e;
    if (int e = check_render(a)) return e;
    // the forward, its kept state and the backward's recompute must run the SAME kernels: the train branch follows the process-wide
    // selection only (kpn_set_geo_rows_mode / kpn_set_fuse_mode); a per-call selection is refused rather than silently replaced
    KPN_REQUIRE(a->rows_kernel == KPN_ROWS_DEFAULT && a->fuse_kernel == KPN_FUSE_DEFAULT,
                "the train branch takes the process-wide kernel selection: rows_kernel / fuse_kernel must be 0");
    KPN_REQUIRE(scene_ws && wp, "null pointer");
    if (int e = check_train(d, a, t, true)) return e;
    const bool backward = !forward_only;
    if (backward) KPN_REQUIRE(g && d_plain && d_geo0 && d_geo1 && d_tex && ws, "gradient pointers / workspace null");
    if (forward_only) KPN_REQUIRE(state != nullptr, "state null");
    const TrainBwdLayout L = train_bwd_layout(d, a);
    const TrainStateLayout S = train_state_layout(d, a);
    if (backward && ws_bytes < L.total) return fail(KPN_EWORKSPACE, "train backward workspace too small");
    if (state && state_bytes < S.total) return fail(KPN_EWORKSPACE, "train state too small");
    char* base = static_cast<char*>(ws);
    char* sbase = static_cast<char*>(state);
    auto F = [&](size_t off) { return reinterpret_cast<float*>(base + off); };
    kpn_scene_dev sc = scene_dev(d, scene_ws);
    const int64_t R = (int64_t)a->nx * a->ny;
    const int Sc = a->n_coarse, Sf = a->n_fine, Sfull = Sc + Sf;
    const bool run_forward = forward_only || state == nullptr;
    // ray set-up lives in the state when there is one
    float* cam_pos = state ? reinterpret_cast<float*>(sbase + S.cam_pos) : F(L.cam_pos);
    float* dirs_all = state ? reinterpret_cast<float*>(sbase + S.dirs) : F(L.dirs);
    float* nearv = state ? reinterpret_cast<float*>(sbase + S.nearv) : F(L.nearv);
    float* farv = state ? reinterpret_cast<float*>(sbase + S.farv) : F(L.farv);
    if (run_forward)
        KPN_LAUNCH(k_make_rays, grid1d(R, 256), dim3(256), stream, a->K, a->RT, a->znear, a->zfar, a->bounds, (int)a->x0, (int)a->y0,
                   (int)a->step, (int)a->step, (int)a->nx, (int)a->ny, (const int*)t->pix, dirs_all, cam_pos, nearv, farv);
    const float std_ = t->rand_noise_std;
    int64_t ci = 0;
    for (int64_t r0 = 0; r0 < R; r0 += L.chunk, ++ci) {
        const int64_t n = (R - r0) < L.chunk ? (R - r0) : L.chunk;
        const float* dirs = dirs_all + r0 * 3;
        const PlanarChunk pl{stream, r0, n, R};
        char* cb = state ? sbase + S.chunk0 + S.chunk_bytes * (size_t)ci : nullptr;
        auto CS = [&](size_t s_off, size_t l_off) { return state ? reinterpret_cast<float*>(cb + s_off) : F(l_off); };
        float *zc = CS(S.zc, L.zc), *zf = CS(S.zf, L.zf), *rgba_c = CS(S.rgba_c, L.rgba_c), *rgba_f = CS(S.rgba_f, L.rgba_f);
        float* contrib = CS(S.contrib, L.contrib);
        char* query_c = state ? cb + S.query_c : base + L.query;
        char* query_f = state ? cb + S.query_f : base + L.query;
        kpn_points pc{nullptr, nullptr, cam_pos, dirs, zc, Sc, std_ != 0.0f ? t->noise_coarse + r0 * Sc : nullptr, std_};
        kpn_points pf{nullptr, nullptr, cam_pos, dirs, zf, Sfull, std_ != 0.0f ? t->noise_fine + r0 * Sfull : nullptr, std_};
        float* sc4 = forward_only ? nullptr : F(L.scratch);   // per-ray results of a repeated forward (unused)
        if (run_forward) {
            // ---- forward: z, rgba of the coarse pass ----
            KPN_LAUNCH(k_coarse_z, grid1d(n * Sc, 256), dim3(256), stream, n, Sc, (const float*)(nearv + r0), (const float*)(farv + r0),
                       t->u_coarse + r0 * Sc, zc);
            sc.keep = t->keep_coarse;
            if (int e = run_field(sc, pc, wp, n * Sc, 1, rgba_c, nullptr, query_c, stream, 1, 1)) return e;
        }
        if (forward_only) {
            // per-ray composites are staged in the (still unused) head of this chunk's fine rgba buffer: 8 floats per ray
            float* st = rgba_f;
            if (int e = kpn_rgba2out(rgba_c, zc, n, Sc, st, st + 3 * n, st + 4 * n, contrib, st + 5 * n, stream)) return e;
            pl.store(a->tex_fg, st, 3);
            pl.store(a->depth, st + 3 * n, 1);
            pl.store(a->alpha, st + 4 * n, 1);
        } else if (run_forward) {
            if (int e = kpn_rgba2out(rgba_c, zc, n, Sc, sc4, sc4 + 3 * n, sc4 + 4 * n, contrib, sc4 + 5 * n, stream)) return e;
        }
        const size_t bwd_bytes = backward ? L.total - L.bwd : 0;
        if (backward) {
            // ---- coarse pass reverse (in the classic call: before the fine forward overwrites the query workspace whose
            //      valid list and row scratch it reuses); sample positions carry no gradient (model.py:1038,1118) ----
            pl.load(F(L.g3), g->d_tex_fg, 3);
            pl.load(F(L.g1a), g->d_depth, 1);
            pl.load(F(L.g1b), g->d_alpha, 1);
            if (int e = kpn_rgba2out_backward(rgba_c, zc, n, Sc, F(L.g3), F(L.g1a), F(L.g1b), nullptr, F(L.drgba_c), stream)) return e;
            if (int e = run_backward(d, scene_ws, wp, n * Sc, nullptr, nullptr, 1, t->keep_coarse, nullptr, 0.0f, nullptr, F(L.drgba_c),
                                     d_plain, d_geo0, d_geo1, d_tex, base + L.bwd, bwd_bytes, stream, &pc, query_c)) return e;
        }
        if (run_forward) {
            // ---- fine pass: samples, forward ----
            launch_fine_samples(stream, n, Sc, Sf, zc, contrib, t->u_fine + r0 * Sf, zf, nullptr, nullptr);
            sc.keep = t->keep_fine;
            if (int e = run_field(sc, pf, wp, n * Sfull, 1, rgba_f, nullptr, query_f, stream, 1, 1)) return e;
        }
        if (forward_only) {
            float* st = contrib;   // the coarse contributions have been consumed by the sampler: 8 floats per ray of staging
            if (int e = kpn_rgba2out(rgba_f, zf, n, Sfull, st, st + 3 * n, st + 4 * n, nullptr, st + 5 * n, stream)) return e;
            pl.store(a->tex_fg_fine, st, 3);
            pl.store(a->depth_fine, st + 3 * n, 1);
            pl.store(a->alpha_fine, st + 4 * n, 1);
            pl.store(a->sdf, st + 5 * n, 1);
        }
        if (backward) {
            // ---- fine pass reverse ----
            pl.load(F(L.g3), g->d_tex_fg_fine, 3);
            pl.load(F(L.g1a), g->d_depth_fine, 1);
            pl.load(F(L.g1b), g->d_alpha_fine, 1);
            pl.load(F(L.g1c), g->d_sdf, 1);
            if (int e = kpn_rgba2out_backward(rgba_f, zf, n, Sfull, F(L.g3), F(L.g1a), F(L.g1b), F(L.g1c), F(L.drgba_f), stream)) return e;
            if (int e = run_backward(d, scene_ws, wp, n * Sfull, nullptr, nullptr, 1, t->keep_fine, nullptr, 0.0f, nullptr, F(L.drgba_f),
                                     d_plain, d_geo0, d_geo1, d_tex, base + L.bwd, bwd_bytes, stream, &pf, query_f)) return e;
        }
    }
    return check_launch(forward_only ? "kpn_render_rays_train_keep" : "kpn_render_rays_train_backward");
}
}  // namespace

extern "C" size_t kpn_render_rays_train_backward_workspace_bytes(const kpn_scene_desc* d, const kpn_render_args* a) {
    if (check_desc(d) != KPN_OK || check_render(a) != KPN_OK || !a->fine) return 0;
    return train_bwd_layout(d, a).total;
}

extern "C" int kpn_render_rays_train_backward(const kpn_scene_desc* d, const void* scene_ws, const float* wp,
                                              const kpn_render_args* a, const kpn_train_args* t, const kpn_render_grads* g,
                                              float* d_plain, float* d_geo0, float* d_geo1, float* d_tex, void* ws,
                                              size_t ws_bytes, void* stream) {
    return train_impl(d, scene_ws, wp, a, t, g, d_plain, d_geo0, d_geo1, d_tex, nullptr, 0, false, ws, ws_bytes, stream);
}

extern "C" size_t kpn_render_rays_train_state_bytes(const kpn_scene_desc* d, const kpn_render_args* a) {
    if (check_desc(d) != KPN_OK || check_render(a) != KPN_OK || !a->fine) return 0;
    return train_state_layout(d, a).total;
}
extern "C" int kpn_render_rays_train_keep(const kpn_scene_desc* d, const void* scene_ws, const float* wp, const kpn_render_args* a,
                                          const kpn_train_args* t, void* state, size_t state_bytes, void* stream) {
    return train_impl(d, scene_ws, wp, a, t, nullptr, nullptr, nullptr, nullptr, nullptr, state, state_bytes, true, nullptr, 0, stream);
}
extern "C" int kpn_render_rays_train_backward_kept(const kpn_scene_desc* d, const void* scene_ws, const float* wp,
                                                   const kpn_render_args* a, const kpn_train_args* t, const kpn_render_grads* g,
                                                   float* d_plain, float* d_geo0, float* d_geo1, float* d_tex, void* state,
                                                   size_t state_bytes, void* ws, size_t ws_bytes, void* stream) {
    KPN_REQUIRE(state != nullptr, "state null");
    return train_impl(d, scene_ws, wp, a, t, g, d_plain, d_geo0, d_geo1, d_tex, state, state_bytes, false, ws, ws_bytes, stream);
}

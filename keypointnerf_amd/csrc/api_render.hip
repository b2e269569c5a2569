// ---------------------------------------------------------------------------------------------
// hierarchical render
namespace {
// ---- the two blocks every layout of this file is composed from, as offsets (Block) and as the pointers of a carved one (View) ----
// the R rays of a call
struct RayBlock { size_t cam_pos, dirs, nearv, farv; };
struct RayView { float *cam_pos, *dirs, *nearv, *farv; };
RayBlock carve_rays(Carver& c, int64_t R) { return {c.take(64), c.take((size_t)R * 3 * 4), c.take((size_t)R * 4), c.take((size_t)R * 4)}; }
// what a chunk of C rays carries from pass to pass: depths and field values at the Sc coarse and the Sfull merged samples, the coarse
// compositor's weights, the query workspace of either pass.  carve_chunk() takes the first four (train: and `contrib`); its layout the rest.
struct ChunkBlock { size_t zc, zf, rgba_c, rgba_f, contrib, query_c, query_f; };
struct ChunkView { float *zc, *zf, *rgba_c, *rgba_f, *contrib; char *query_c, *query_f; };
ChunkBlock carve_chunk(Carver& c, int64_t C, int64_t Sc, int64_t Sfull, bool train) {
    ChunkBlock k{};
    k.zc = c.take((size_t)C * Sc * 4); k.zf = c.take((size_t)C * Sfull * 4);
    if (train) {
        k.rgba_c = c.take((size_t)C * Sc * 5 * 4); k.rgba_f = c.take((size_t)C * Sfull * 5 * 4);
        // max(Sfull, 8): a forward-only call stages its per-ray composites here and in the head of rgba_f (8 floats per ray)
        k.contrib = c.take((size_t)C * (Sfull > 8 ? Sfull : 8) * 4);
    } else {
        // eval with coarse re-use (the default): the coarse values kept for the fine pass and the values at the new samples share the
        // block a pass without re-use fills as a whole — never both in one call (round 6: 671 MB less per 512 x 512 plan)
        k.rgba_c = k.rgba_f = c.take((size_t)C * Sfull * 5 * 4);
        c.o += 256;   // (the alignment of RenderLayout::rgba_n inside the block)
    }
    return k;
}
template <class T = float> T* at(void* base, size_t off) { return reinterpret_cast<T*>(static_cast<char*>(base) + off); }
RayView ray_view(void* base, const RayBlock& r) { return {at(base, r.cam_pos), at(base, r.dirs), at(base, r.nearv), at(base, r.farv)}; }
ChunkView chunk_view(void* base, const ChunkBlock& k) {
    return {at(base, k.zc), at(base, k.zf), at(base, k.rgba_c), at(base, k.rgba_f), at(base, k.contrib), at<char>(base, k.query_c), at<char>(base, k.query_f)};
}

struct RenderLayout { RayBlock rays; ChunkBlock k; size_t rgba_n, zn, src, color, depth, alpha, sdf, total; int64_t chunk; };
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
    const int64_t C = pick_chunk(d, a);
    const int64_t Sfull = a->n_coarse + (a->fine ? a->n_fine : 0);
    Carver c;
    L.chunk = C;
    L.rays = carve_rays(c, (int64_t)a->nx * a->ny);
    L.k = carve_chunk(c, C, a->n_coarse, Sfull, false);
    L.rgba_n = L.k.rgba_c + align_up((size_t)C * a->n_coarse * 5 * 4, 256);
    L.zn = c.take((size_t)C * (a->fine ? a->n_fine : 0) * 4);
    L.src = c.take((size_t)C * Sfull * sizeof(int16_t));
    L.k.contrib = c.take((size_t)C * a->n_coarse * 4);                  // the coarse compositor's weights (the fine one writes none)
    L.color = c.take((size_t)C * 3 * 4);
    L.depth = c.take((size_t)C * 4);
    L.alpha = c.take((size_t)C * 4);
    L.sdf = c.take((size_t)C * 4);
    {   // eval passes use the POOL layout of the scratch, the train branch (same workspace) the ROWS layout: room for either
        const size_t qa = query_layout(C * Sfull, d->n_views, false).total, qb = query_layout(C * Sfull, d->n_views, pool_layout_selected()).total;
        L.k.query_c = L.k.query_f = c.take(qa > qb ? qa : qb);
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

static void launch_make_rays(void* stream, const kpn_render_args* a, const int* pix, int step_y, const RayView& rays) {
    KPN_LAUNCH(k_make_rays, grid1d((int64_t)a->nx * a->ny, 256), dim3(256), stream, a->K, a->RT, a->znear, a->zfar, a->bounds, (int)a->x0, (int)a->y0,
               (int)a->step, step_y, (int)a->nx, (int)a->ny, pix, rays.dirs, rays.cam_pos, rays.nearv, rays.farv);
}

static int render_impl(const kpn_scene_desc* d, const void* scene_ws, const float* wp, const kpn_render_args* a,
                       const kpn_train_args* t, void* ws, size_t ws_bytes, void* stream) {
    if (int e = check_desc(d)) return e;
    if (int e = check_render(a)) return e;
    KPN_REQUIRE(scene_ws && wp && ws, "null pointer");
    if (t) if (int e = check_train(d, a, t, false)) return e;
    const RenderLayout L = render_layout(d, a);
    if (ws_bytes < L.total) return fail(KPN_EWORKSPACE, "render workspace too small");
    const RayView rays = ray_view(ws, L.rays);
    const ChunkView k = chunk_view(ws, L.k);
    float *rgba_n = at(ws, L.rgba_n), *zn = at(ws, L.zn), *color = at(ws, L.color), *depth = at(ws, L.depth), *alpha = at(ws, L.alpha), *sdf = at(ws, L.sdf);
    int16_t* src = at<int16_t>(ws, L.src);
    kpn_scene_dev sc = scene_dev(d, scene_ws);
    const int64_t R = (int64_t)a->nx * a->ny;
    const int Sc = a->n_coarse, Sf = a->fine ? a->n_fine : 0, Sfull = Sc + Sf;
    const float std_ = t ? t->rand_noise_std : 0.0f;
    launch_make_rays(stream, a, t ? (const int*)t->pix : (const int*)nullptr, (int)(a->step_y > 0 ? a->step_y : a->step), rays);
    for (int64_t r0 = 0; r0 < R; r0 += L.chunk) {
        const int64_t n = (R - r0) < L.chunk ? (R - r0) : L.chunk;
        const float* dirs = rays.dirs + r0 * 3;
        const PlanarChunk pl{stream, r0, n, R};
        KPN_LAUNCH(k_coarse_z, grid1d(n * Sc, 256), dim3(256), stream, n, Sc, (const float*)(rays.nearv + r0),
                   (const float*)(rays.farv + r0), t ? t->u_coarse + r0 * Sc : (const float*)nullptr, k.zc);
        // eval: the fine pass re-uses the coarse samples' field values (identical points, no dropout, no noise: identical
        // deterministic results) and evaluates the field at the new samples only — 128 instead of 192 evaluations per ray
        // at 64 + 64 samples.  The train branch draws fresh dropout masks and noise for the fine query and cannot.
        const bool reuse = (t == nullptr) && a->fine && !env_flag("KPN_NO_COARSE_REUSE");   // (read per call: tests flip it)
        // a render pass of this chunk at S samples per ray: lean; eval: pooled inside the rows kernel; the train branch keeps the per-view rows
        auto field = [&](const float* z, int S, const float* noise, float* out) {
            FieldPass p;
            p.points = kpn_points{nullptr, nullptr, rays.cam_pos, dirs, z, S, noise, std_};
            p.N = n * S; p.mode = 1; p.out = out; p.ws = k.query_c; p.lean = true; p.allow_pool = t == nullptr;
            p.rows_sel = a->rows_kernel; p.fuse_sel = a->fuse_kernel;
            return run_field(sc, wp, p, stream);
        };
        sc.keep = t ? t->keep_coarse : 0xFFFFFFFFu;
        if (int e = field(k.zc, Sc, std_ != 0.0f ? t->noise_coarse + r0 * Sc : nullptr, k.rgba_c)) return e;   // model.py:1062
        if (int e = kpn_rgba2out(k.rgba_c, k.zc, n, Sc, color, depth, alpha, k.contrib, sdf, stream)) return e;
        const kpn_render_stages* st = a->stages;
        auto copy_out = [&](float* dst, const float* src_, size_t floats) {   // device to device, on the call's stream
            (void)hipMemcpyAsync(dst, src_, floats * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream);
        };
        if (st && st->dirs) copy_out(st->dirs + r0 * 3, dirs, (size_t)n * 3);
        if (st && st->cam_pos && r0 == 0) copy_out(st->cam_pos, rays.cam_pos, 3);
        if (st && st->z_coarse) copy_out(st->z_coarse + r0 * Sc, k.zc, (size_t)n * Sc);
        if (st && st->rgba_coarse) copy_out(st->rgba_coarse + r0 * Sc * 5, k.rgba_c, (size_t)n * Sc * 5);
        pl.store(a->tex_fg, color, 3);
        pl.store(a->depth, depth, 1);
        pl.store(a->alpha, alpha, 1);
        if (!a->fine) continue;
        launch_fine_samples(stream, n, Sc, Sf, k.zc, k.contrib, t ? t->u_fine + r0 * Sf : (const float*)nullptr, k.zf, reuse ? zn : nullptr,
                            reuse ? src : nullptr);
        sc.keep = t ? t->keep_fine : 0xFFFFFFFFu;
        if (reuse) {
            if (int e = field(zn, Sf, nullptr, rgba_n)) return e;   // model.py:1082, the new samples
            if (int e = rgba2out_merged(k.rgba_c, rgba_n, src, k.zf, n, Sc, Sf, color, depth, alpha, sdf, stream)) return e;
        } else {
            if (int e = field(k.zf, Sfull, std_ != 0.0f ? t->noise_fine + r0 * Sfull : nullptr, k.rgba_f)) return e;   // model.py:1082
            if (int e = kpn_rgba2out(k.rgba_f, k.zf, n, Sfull, color, depth, alpha, nullptr, sdf, stream)) return e;
        }
        if (st && st->z_fine) copy_out(st->z_fine + r0 * Sfull, k.zf, (size_t)n * Sfull);
        if (st && st->rgba_fine) {
            if (reuse) KPN_LAUNCH(k_merge_rgba, grid1d(n * Sfull, 256), dim3(256), stream, n, Sfull, Sc, (const float*)k.rgba_c, (const float*)rgba_n,
                                  (const int16_t*)src, st->rgba_fine + r0 * Sfull * 5);
            else copy_out(st->rgba_fine + r0 * Sfull * 5, k.rgba_f, (size_t)n * Sfull * 5);
        }
        pl.store(a->tex_fg_fine, color, 3);
        pl.store(a->depth_fine, depth, 1);
        pl.store(a->alpha_fine, alpha, 1);
        pl.store(a->sdf, sdf, 1);
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
struct TrainBwdLayout { RayBlock rays; ChunkBlock k; size_t scratch, g3, g1a, g1b, g1c, drgba_c, drgba_f, bwd, total; int64_t chunk; };
TrainBwdLayout train_bwd_layout(const kpn_scene_desc* d, const kpn_render_args* a) {
    TrainBwdLayout L;
    const int64_t R = (int64_t)a->nx * a->ny;
    const int64_t Sfull = a->n_coarse + a->n_fine;
    int64_t C = a->chunk_rays > 0 ? a->chunk_rays : kBwdChunk / Sfull;   // one backward pass per point set
    if (C * Sfull > kBwdChunk) C = kBwdChunk / Sfull;
    if (C > R) C = R;
    L.chunk = C;
    Carver c;
    L.rays = carve_rays(c, R);
    L.k = carve_chunk(c, C, a->n_coarse, Sfull, true);
    L.scratch = c.take((size_t)C * 8 * 4);  // colour / depth / alpha / sdf of the recomputed forward (unused results)
    L.g3 = c.take((size_t)C * 3 * 4); L.g1a = c.take((size_t)C * 4); L.g1b = c.take((size_t)C * 4); L.g1c = c.take((size_t)C * 4);
    L.drgba_c = c.take((size_t)C * a->n_coarse * 5 * 4); L.drgba_f = c.take((size_t)C * Sfull * 5 * 4);
    L.k.query_c = L.k.query_f = c.take(query_layout(C * Sfull, d->n_views).total);   // one workspace, used by the coarse pass and then the fine one
    L.bwd = c.take(bwd_layout(C * Sfull, d->n_views, 2).total);
    L.total = c.o;
    return L;
}

// State a train-branch forward call can leave behind for its backward call (kpn_render_rays_train_keep): rays, and per
// chunk of rays the depths, the field values and — the expensive part — the valid lists and (point, view) rows of both
// field passes.  With it the backward call skips the forward it otherwise repeats (k_make_rays, k_coarse_z, 2 x
// k_mask_compact + k_geo_rows + k_fuse_color, compositor, sampler: 1.05 of 9.1 ms at 1024 rays x 192 samples).
struct TrainStateLayout { RayBlock rays; size_t chunk0; ChunkBlock k; size_t chunk_bytes, total; int64_t chunk, nchunks; };   // k: offsets inside one chunk block
TrainStateLayout train_state_layout(const kpn_scene_desc* d, const kpn_render_args* a) {
    TrainStateLayout S;
    const int64_t R = (int64_t)a->nx * a->ny, C = train_bwd_layout(d, a).chunk;
    const int64_t Sfull = a->n_coarse + a->n_fine;
    S.chunk = C; S.nchunks = (R + C - 1) / C;
    Carver c;
    S.rays = carve_rays(c, R);
    S.chunk0 = c.o;
    c = Carver();
    S.k = carve_chunk(c, C, a->n_coarse, Sfull, true);
    S.k.query_c = c.take(query_layout(C * a->n_coarse, d->n_views).total);
    S.k.query_f = c.take(query_layout(C * Sfull, d->n_views).total);
    S.chunk_bytes = c.o;
    S.total = S.chunk0 + S.chunk_bytes * (size_t)S.nchunks;
    return S;
}

// one of the two field passes of a chunk, and rays [r0, r0 + n) of a train-branch call with their buffers — in the kept state when
// the call has one, else in the workspace
struct TrainPass { bool fine; kpn_points ps; uint32_t keep; float *z, *rgba; char* query; };
struct TrainChunk { int64_t r0, n; ChunkView v; PlanarChunk pl; TrainPass coarse, fine; };
// A train-branch call and the steps its three entry points are made of.  Per chunk the order is fixed: the coarse reverse runs
// before the fine forward, which in the classic call overwrites the query workspace whose valid list and row scratch it reuses.
struct TrainCall {
    const kpn_scene_desc* d; const void* scene_ws; const float* wp; const kpn_render_args* a; const kpn_train_args* t;
    const kpn_render_grads* g; float *d_plain, *d_geo0, *d_geo1, *d_tex;
    void *state, *ws, *stream;
    TrainBwdLayout L; TrainStateLayout S;
    kpn_scene_dev sc; int64_t R; int Sc, Sf, Sfull; RayView rays;
    float* d_kpt = nullptr; int n_kpt = 0;   // optional keypoint gradient (the _kpt entries): `ws` then ends with kpt_layout()'s scratch
    size_t bwd_bytes() const { return d_kpt ? kpt_layout(L.total - L.bwd, d->n_views).total : L.total - L.bwd; }
    // the checks of every entry point, in their order, then the layouts.  forward_only: fills `state` and writes the outputs of `a`;
    // otherwise a backward: from `state`, or (state == nullptr) the classic one that repeats the forward inside `ws`
    int begin(size_t state_bytes, size_t ws_bytes, bool forward_only) {
        if (int e = check_desc(d)) return e;
        if (int e = check_render(a)) return e;
        // the forward, its kept state and the backward's recompute must run the SAME kernels: the train branch follows the process-wide
        // selection only (kpn_set_geo_rows_mode / kpn_set_fuse_mode); a per-call selection is refused rather than silently replaced
        KPN_REQUIRE(a->rows_kernel == KPN_ROWS_DEFAULT && a->fuse_kernel == KPN_FUSE_DEFAULT,
                    "the train branch takes the process-wide kernel selection: rows_kernel / fuse_kernel must be 0");
        KPN_REQUIRE(scene_ws && wp, "null pointer");
        if (int e = check_train(d, a, t, true)) return e;
        if (!forward_only) KPN_REQUIRE(g && d_plain && d_geo0 && d_geo1 && d_tex && ws, "gradient pointers / workspace null");
        if (forward_only) KPN_REQUIRE(state != nullptr, "state null");
        L = train_bwd_layout(d, a);
        S = train_state_layout(d, a);
        if (d_kpt) KPN_REQUIRE(n_kpt >= 1 && n_kpt <= KPN_NKPT, "n_kpt in 1..24");
        if (!forward_only && ws_bytes < L.bwd + bwd_bytes()) return fail(KPN_EWORKSPACE, "train backward workspace too small");
        if (state && state_bytes < S.total) return fail(KPN_EWORKSPACE, "train state too small");
        sc = scene_dev(d, scene_ws);
        R = (int64_t)a->nx * a->ny; Sc = a->n_coarse; Sf = a->n_fine; Sfull = Sc + Sf;
        rays = ray_view(state ? state : ws, L.rays);   // (both layouts start with the ray block)
        return KPN_OK;
    }
    TrainChunk chunk(int64_t ci) const {
        const int64_t r0 = ci * L.chunk, n = (R - r0) < L.chunk ? (R - r0) : L.chunk;
        const ChunkView v = state ? chunk_view(at<char>(state, S.chunk0 + S.chunk_bytes * (size_t)ci), S.k) : chunk_view(ws, L.k);
        const float std_ = t->rand_noise_std, *dirs = rays.dirs + r0 * 3;
        const kpn_points pc{nullptr, nullptr, rays.cam_pos, dirs, v.zc, Sc, std_ != 0.0f ? t->noise_coarse + r0 * Sc : nullptr, std_};
        const kpn_points pf{nullptr, nullptr, rays.cam_pos, dirs, v.zf, Sfull, std_ != 0.0f ? t->noise_fine + r0 * Sfull : nullptr, std_};
        return {r0, n, v, PlanarChunk{stream, r0, n, R}, TrainPass{false, pc, t->keep_coarse, v.zc, v.rgba_c, v.query_c},
                TrainPass{true, pf, t->keep_fine, v.zf, v.rgba_f, v.query_f}};
    }
    // an entry point: the checks, the rays unless the state holds them, then `steps` on every chunk
    template <class Steps> int run(size_t state_bytes, size_t ws_bytes, bool forward_only, Steps steps) {
        if (int e = begin(state_bytes, ws_bytes, forward_only)) return e;
        if (forward_only || !state) launch_make_rays(stream, a, (const int*)t->pix, (int)a->step, rays);
        for (int64_t ci = 0; ci < S.nchunks; ++ci) if (int e = steps(chunk(ci))) return e;
        return check_launch(forward_only ? "kpn_render_rays_train_keep" : "kpn_render_rays_train_backward");
    }
    // forward of a pass: its depths (the fine ones from the coarse composite's weights), then the field — lean, and with the valid
    // list and the per-view rows left in `query` for the reverse
    int forward(const TrainChunk& c, const TrainPass& p) const {
        if (p.fine) launch_fine_samples(stream, c.n, Sc, Sf, c.v.zc, c.v.contrib, t->u_fine + c.r0 * Sf, c.v.zf, nullptr, nullptr);
        else KPN_LAUNCH(k_coarse_z, grid1d(c.n * Sc, 256), dim3(256), stream, c.n, Sc, (const float*)(rays.nearv + c.r0), (const float*)(rays.farv + c.r0),
                        t->u_coarse + c.r0 * Sc, c.v.zc);
        kpn_scene_dev s = sc;
        s.keep = p.keep;
        FieldPass f;
        f.points = p.ps; f.N = c.n * p.ps.S; f.mode = 1; f.out = p.rgba; f.ws = p.query; f.lean = true; f.keep_rows = true;
        return run_field(s, wp, f, stream);
    }
    // the per-ray composite of a pass into 8 floats per ray at `st`: colour, depth, alpha, sdf; the coarse one also writes the sampler's weights
    int composite(const TrainChunk& c, const TrainPass& p, float* st) const {
        return kpn_rgba2out(p.rgba, p.z, c.n, p.ps.S, st, st + 3 * c.n, st + 4 * c.n, p.fine ? nullptr : c.v.contrib, st + 5 * c.n, stream);
    }
    // forward only: the composite and its planar outputs, staged in a buffer of the chunk that is idle — the coarse one in the (still
    // unused) head of the fine rgba, the fine one in the coarse weights the sampler has consumed
    int composite_and_store(const TrainChunk& c, const TrainPass& p) const {
        float* st = p.fine ? c.v.contrib : c.v.rgba_f;
        if (int e = composite(c, p, st)) return e;
        c.pl.store(p.fine ? a->tex_fg_fine : a->tex_fg, st, 3);
        c.pl.store(p.fine ? a->depth_fine : a->depth, st + 3 * c.n, 1);
        c.pl.store(p.fine ? a->alpha_fine : a->alpha, st + 4 * c.n, 1);
        if (p.fine) c.pl.store(a->sdf, st + 5 * c.n, 1);
        return KPN_OK;
    }
    // reverse of a pass: the compositor's, then the field's on the list and rows its forward left; sample positions carry no
    // gradient (model.py:1038,1118)
    int reverse(const TrainChunk& c, const TrainPass& p) const {
        float *g3 = at(ws, L.g3), *g1a = at(ws, L.g1a), *g1b = at(ws, L.g1b), *g1c = p.fine ? at(ws, L.g1c) : nullptr;
        float* drgba = at(ws, p.fine ? L.drgba_f : L.drgba_c);
        c.pl.load(g3, p.fine ? g->d_tex_fg_fine : g->d_tex_fg, 3);
        c.pl.load(g1a, p.fine ? g->d_depth_fine : g->d_depth, 1);
        c.pl.load(g1b, p.fine ? g->d_alpha_fine : g->d_alpha, 1);
        if (p.fine) c.pl.load(g1c, g->d_sdf, 1);
        if (int e = kpn_rgba2out_backward(p.rgba, p.z, c.n, p.ps.S, g3, g1a, g1b, g1c, drgba, stream)) return e;
        BackwardPass b;
        b.N = c.n * p.ps.S; b.marched = &p.ps; b.mode = 1; b.keep_mask = p.keep; b.d_out = drgba;
        b.d_plain = d_plain; b.d_geo0 = d_geo0; b.d_geo1 = d_geo1; b.d_tex = d_tex;
        b.ws = at<char>(ws, L.bwd); b.ws_bytes = bwd_bytes(); b.fwd_query_ws = p.query;
        b.d_kpt = d_kpt; b.n_kpt = n_kpt;
        return run_backward(d, scene_ws, wp, b, stream);
    }
};
}  // namespace

extern "C" size_t kpn_render_rays_train_backward_workspace_bytes(const kpn_scene_desc* d, const kpn_render_args* a) {
    if (check_desc(d) != KPN_OK || check_render(a) != KPN_OK || !a->fine) return 0;
    return train_bwd_layout(d, a).total;
}

namespace {
int train_backward_classic(TrainCall& tc, size_t ws_bytes) {
    void* const ws = tc.ws;
    return tc.run(0, ws_bytes, false, [&](const TrainChunk& c) {   // the classic backward: the forward repeated inside `ws`
        int e;   // (the coarse composite's per-ray results are not used: L.scratch)
        return ((e = tc.forward(c, c.coarse)) || (e = tc.composite(c, c.coarse, at(ws, tc.L.scratch))) || (e = tc.reverse(c, c.coarse)) ||
                (e = tc.forward(c, c.fine)) || (e = tc.reverse(c, c.fine))) ? e : KPN_OK;
    });
}
int train_backward_kept(TrainCall& tc, size_t state_bytes, size_t ws_bytes) {
    return tc.run(state_bytes, ws_bytes, false, [&](const TrainChunk& c) {
        const int e = tc.reverse(c, c.coarse);
        return e ? e : tc.reverse(c, c.fine);
    });
}
}  // namespace

extern "C" int kpn_render_rays_train_backward(const kpn_scene_desc* d, const void* scene_ws, const float* wp,
                                              const kpn_render_args* a, const kpn_train_args* t, const kpn_render_grads* g,
                                              float* d_plain, float* d_geo0, float* d_geo1, float* d_tex, void* ws,
                                              size_t ws_bytes, void* stream) {
    TrainCall tc{d, scene_ws, wp, a, t, g, d_plain, d_geo0, d_geo1, d_tex, nullptr, ws, stream};
    return train_backward_classic(tc, ws_bytes);
}

extern "C" size_t kpn_render_rays_train_backward_workspace_bytes_kpt(const kpn_scene_desc* d, const kpn_render_args* a) {
    if (check_desc(d) != KPN_OK || check_render(a) != KPN_OK || !a->fine) return 0;
    const TrainBwdLayout L = train_bwd_layout(d, a);
    return L.bwd + kpt_layout(L.total - L.bwd, d->n_views).total;
}

extern "C" int kpn_render_rays_train_backward_kpt(const kpn_scene_desc* d, const void* scene_ws, const float* wp,
                                                  const kpn_render_args* a, const kpn_train_args* t, const kpn_render_grads* g,
                                                  float* d_plain, float* d_geo0, float* d_geo1, float* d_tex, float* d_kpt3d,
                                                  int32_t n_kpt, void* ws, size_t ws_bytes, void* stream) {
    KPN_REQUIRE(d_kpt3d != nullptr, "d_kpt3d null");
    TrainCall tc{d, scene_ws, wp, a, t, g, d_plain, d_geo0, d_geo1, d_tex, nullptr, ws, stream};
    tc.d_kpt = d_kpt3d; tc.n_kpt = n_kpt;
    return train_backward_classic(tc, ws_bytes);
}

extern "C" size_t kpn_render_rays_train_state_bytes(const kpn_scene_desc* d, const kpn_render_args* a) {
    if (check_desc(d) != KPN_OK || check_render(a) != KPN_OK || !a->fine) return 0;
    return train_state_layout(d, a).total;
}
extern "C" int kpn_render_rays_train_keep(const kpn_scene_desc* d, const void* scene_ws, const float* wp, const kpn_render_args* a,
                                          const kpn_train_args* t, void* state, size_t state_bytes, void* stream) {
    TrainCall tc{d, scene_ws, wp, a, t, nullptr, nullptr, nullptr, nullptr, nullptr, state, nullptr, stream};
    return tc.run(state_bytes, 0, true, [&](const TrainChunk& c) {
        int e;
        return ((e = tc.forward(c, c.coarse)) || (e = tc.composite_and_store(c, c.coarse)) || (e = tc.forward(c, c.fine)) ||
                (e = tc.composite_and_store(c, c.fine))) ? e : KPN_OK;
    });
}
extern "C" int kpn_render_rays_train_backward_kept(const kpn_scene_desc* d, const void* scene_ws, const float* wp,
                                                   const kpn_render_args* a, const kpn_train_args* t, const kpn_render_grads* g,
                                                   float* d_plain, float* d_geo0, float* d_geo1, float* d_tex, void* state,
                                                   size_t state_bytes, void* ws, size_t ws_bytes, void* stream) {
    KPN_REQUIRE(state != nullptr, "state null");
    TrainCall tc{d, scene_ws, wp, a, t, g, d_plain, d_geo0, d_geo1, d_tex, state, ws, stream};
    return train_backward_kept(tc, state_bytes, ws_bytes);
}
extern "C" int kpn_render_rays_train_backward_kept_kpt(const kpn_scene_desc* d, const void* scene_ws, const float* wp,
                                                       const kpn_render_args* a, const kpn_train_args* t, const kpn_render_grads* g,
                                                       float* d_plain, float* d_geo0, float* d_geo1, float* d_tex, float* d_kpt3d,
                                                       int32_t n_kpt, void* state, size_t state_bytes, void* ws, size_t ws_bytes,
                                                       void* stream) {
    KPN_REQUIRE(state != nullptr, "state null");
    KPN_REQUIRE(d_kpt3d != nullptr, "d_kpt3d null");
    TrainCall tc{d, scene_ws, wp, a, t, g, d_plain, d_geo0, d_geo1, d_tex, state, ws, stream};
    tc.d_kpt = d_kpt3d; tc.n_kpt = n_kpt;
    return train_backward_kept(tc, state_bytes, ws_bytes);
}

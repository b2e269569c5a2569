// ---------------------------------------------------------------------------------------------
// backward of the field evaluation
namespace {
const int64_t kBwdChunk = 262144;  // points per pass: V=3 -> 786432 rows x 4.3 KB of dumps = 3.4 GB
static_assert(kBwdChunk <= 262144, "kUncappedPoints (query_layout) must cover a backward pass");
#ifdef KPN_SIMT_EMU
const int kGradWorkers = 3;     // row workers (one workgroup each; its waves are the column groups)
#else
#ifndef KPN_GRAD_WORKERS
#define KPN_GRAD_WORKERS 512    // 2 workgroups per CU
#endif
const int kGradWorkers = KPN_GRAD_WORKERS;
#endif
const int kPartialUnits = 72;   // capacity of the partial-tile scratch in units of (workers x 2048 floats)
// full = 1: the whole-query reverse (adds the forward row scratch, the per-point dumps and the d x_view rows)
// colour-head dumps, floats per (point, view) row, in kpn_color_bufs order (X buffers then dA buffers)
const int kColorLd[25] = {4, 16, KPN_LD_XDIR, KPN_LD_XBL, 64, 32, 32, 32, 2, 32, 32, KPN_LD_XO0, 16, 8,
                          2, 8, 16, 2, 32, KPN_LD_DV11, 32, 32, 64, KPN_LD_XDIR, 16};
struct BwdLayout { size_t count, list, X0, X1, X2, X3, D0, D1, D2, D3, partial, dbp, xscr, Xp, Xh0, Xh1, D20, D21, D22, dxrows,
                   color, color_bytes, Dcmp, total; int64_t chunk; };
// full: 0 = geometry rows only; 1 = whole query, geometry outputs; 2 = whole query incl. the colour head
BwdLayout bwd_layout(int64_t N, int V, int full) {
    BwdLayout L{};
    L.chunk = N < kBwdChunk ? N : kBwdChunk;
    const size_t ntiles = (size_t)((L.chunk + KPN_TILE - 1) / KPN_TILE);
    const size_t npts = ntiles * KPN_TILE, rows = npts * V;
    Carver c;
    L.count = c.take(256);
    L.list = c.take((size_t)L.chunk * sizeof(int));
    L.X0 = c.take(rows * KPN_LDX0 * 4); L.X1 = c.take(rows * 128 * 4); L.X2 = c.take(rows * KPN_LDX2 * 4); L.X3 = c.take(rows * 128 * 4);
    L.D0 = c.take(rows * 128 * 4); L.D1 = c.take(rows * 128 * 4); L.D2 = c.take(rows * 128 * 4); L.D3 = c.take(rows * 64 * 4);
    // partial tile blocks of all weight-gradient jobs of a pass (they run in shared launches): sum over the 19 layers of
    // column groups x MV = 65 -> 72 x workers x 8 KB (checked when the jobs are queued); bias partials per job
    L.partial = c.take((size_t)kPartialUnits * kGradWorkers * (2 * 16 * 64) * 4);
    L.dbp = c.take((size_t)KPN_WGRAD_MAX_JOBS * kGradWorkers * 4 * 64 * 4);
    if (full) {
        L.xscr = c.take(ntiles * (size_t)V * KPN_ROW_SLABS * 64 * sizeof(float4));
        L.Xp = c.take(npts * 128 * 4); L.Xh0 = c.take(npts * 64 * 4); L.Xh1 = c.take(npts * 64 * 4);
        L.D20 = c.take(npts * 64 * 4); L.D21 = c.take(npts * 64 * 4); L.D22 = c.take(npts * 2 * 4);
        L.dxrows = c.take(rows * 64 * 4);
    }
    if (full == 2) {
        size_t per_row = 0;
        for (int i = 0; i < 25; ++i) per_row += kColorLd[i];
        L.color_bytes = rows * per_row * 4;
        L.color = c.take(L.color_bytes);
        L.Dcmp = c.take(npts * 24 * 4);
    }
    L.total = c.o;
    return L;
}
}  // namespace

// rows[0] = (point, view) rows of the current pass, rows[1] = points, both padded to whole tiles
__global__ void k_bwd_rows(const int* __restrict__ count, int V, int64_t* __restrict__ rows) {
    const int64_t npts = (int64_t)((*count + KPN_TILE - 1) / KPN_TILE) * KPN_TILE;
    rows[0] = npts * V;
    rows[1] = npts;
}

namespace {
// d_x != nullptr: geometry rows only, upstream gradient given per (point, view).  Otherwise the whole-query reverse from
// d_out (N,5): its geometry columns only (d_tex == nullptr) or all five incl. the colour head (d_tex != nullptr).
int run_backward(const kpn_scene_desc* d, const void* scene_ws, const float* wp, int64_t N, const float* pts, const float* view,
                 int mode, uint32_t keep_mask, const float* noise, float noise_std, const float* d_x, const float* d_out,
                 float* d_plain, float* d_geo0, float* d_geo1, float* d_tex, void* ws, size_t ws_bytes, void* stream,
                 const kpn_points* marched = nullptr, void* fwd_query_ws = nullptr) {
    // fwd_query_ws: the workspace a run_field() call on the SAME points just used: its valid list and row scratch are
    // reused instead of being recomputed (the train-branch backward runs the forward anyway to get rgba)
    // marched: the points are ray-marched (cam_pos + dirs * z, as kpn_render_rays evaluates them) instead of explicit;
    // one pass only (N <= kBwdChunk)
    const int V = d->n_views;
    const int full = d_x != nullptr ? 0 : (d_tex ? 2 : 1);
    const BwdLayout L = bwd_layout(N, V, full);
    if (ws_bytes < L.total) return fail(KPN_EWORKSPACE, "backward workspace too small");
    if (marched && N > L.chunk) return fail(KPN_EINVAL, "ray-marched backward pass too large");
    kpn_scene_dev sc = scene_dev(d, scene_ws);
    sc.keep = keep_mask;
    char* base = static_cast<char*>(ws);
    auto fp = [&](size_t off) { return reinterpret_cast<float*>(base + off); };
    int* count = reinterpret_cast<int*>(base + L.count);  // [0] valid count, [1..3] work tickets of the three persistent kernels
    int64_t* rows_dev = reinterpret_cast<int64_t*>(base + L.count + 64);
    int* list = reinterpret_cast<int*>(base + L.list);
    kpn_bwd_bufs B;
    B.X0 = fp(L.X0); B.X1 = fp(L.X1); B.X2 = fp(L.X2); B.X3 = fp(L.X3);
    B.D0 = fp(L.D0); B.D1 = fp(L.D1); B.D2 = fp(L.D2); B.D3 = fp(L.D3);
    B.dgeo0 = d_geo0; B.dgeo1 = d_geo1;
    kpn_fuse_bwd_bufs F{};
    if (full) {
        F.Xp = fp(L.Xp); F.Xh0 = fp(L.Xh0); F.Xh1 = fp(L.Xh1); F.D20 = fp(L.D20); F.D21 = fp(L.D21); F.D22 = fp(L.D22);
        F.dxrows = fp(L.dxrows);
    }
    kpn_color_bufs C{};
    if (full == 2) {
        const size_t rows = (size_t)((L.chunk + KPN_TILE - 1) / KPN_TILE) * KPN_TILE * V;
        float* q = fp(L.color);
        float** slots[25] = {&C.Xrd, &C.Xe1, &C.Xdir, &C.Xbl, &C.Xb1, &C.Xa, &C.Xv10, &C.Xv11, &C.Xt33, &C.Xv20, &C.Xv21, &C.Xo0,
                             &C.Xo1, &C.Xo2, &C.Do2, &C.Do1, &C.Do0, &C.Dv21, &C.Dv20, &C.Dv11, &C.Dv10, &C.Dbl1, &C.Dbl0,
                             &C.Dre1, &C.Dre0};
        for (int i = 0; i < 25; ++i) { *slots[i] = q; q += rows * kColorLd[i]; }
        C.Dcmp = fp(L.Dcmp);
        C.dtex = d_tex;
        C.dani = d_plain + kpn_plain_weight_floats() - 1;
        F.Dcmp = C.Dcmp;
    }
    float* partial = fp(L.partial);
    float* dbp = fp(L.dbp);
    const int blocks = field_grid_blocks();
    // rows of views switched off by the train-time dropout are skipped by k_color_bwd (their dumps are never written) and carry a
    // zero upstream gradient in k_geo_rows_bwd: k_weight_grad reads them as zeros by the same mask (no memset of the dumps)
    const uint32_t wgrad_keep = keep_mask | ~((V >= 32) ? 0xFFFFFFFFu : ((1u << V) - 1u));
    // dW[layer] += dY^T X over the rows (which = 0) or points (which = 1) of this pass
    // weight-gradient jobs of a pass: queued while the producers are launched, then run in one launch per MV class
    // and one reduce launch
    kpn_wgrad_jobs jobs[3], all;  // MV = 1, 2, 4
    int gzmax[3];
    size_t partial_used = 0;
    bool overflow = false;
    auto reset_jobs = [&]() { jobs[0].n = jobs[1].n = jobs[2].n = all.n = 0; gzmax[0] = gzmax[1] = gzmax[2] = 0; partial_used = 0; };
    // which: 0 = (point, view) rows, 1 = points.  Kc: columns of the X dump read (even); Kt: real input features
    auto wgrad = [&](int mv, int which, const float* dY, int ldy, int M, const float* X, int ldx, int Kc, int Kt, int layer,
                     int cmap, int omap) {
        const int cls = mv == 1 ? 0 : (mv == 2 ? 1 : 2);
        const int gz = (Kc + 63) / 64;
        kpn_wgrad_job j;
        j.dY = dY; j.X = X; j.ldy = ldy; j.M = M; j.ldx = ldx; j.Kc = Kc; j.Kt = Kt; j.cmap = cmap; j.omap = omap; j.mv = mv; j.which = which;
        j.V = which == 0 ? V : 1; j.keep = which == 0 ? wgrad_keep : 0xFFFFFFFFu;
        j.partial = partial + partial_used;
        partial_used += (size_t)gz * kGradWorkers * mv * 2048;
        if (partial_used > (size_t)kPartialUnits * kGradWorkers * 2048 || all.n >= KPN_WGRAD_MAX_JOBS) { overflow = true; return; }
        j.dbp = dbp + (size_t)all.n * kGradWorkers * 4 * 64;
        j.dW = d_plain + plain_w_off(layer);
        j.dB = d_plain + plain_b_off(layer);
        j.in_dim = plain_dims[layer][1];
        jobs[cls].j[jobs[cls].n++] = j;
        all.j[all.n++] = j;
        if (gz > gzmax[cls]) gzmax[cls] = gz;
    };
    auto run_jobs = [&]() {
        if (jobs[0].n) KPN_LAUNCH(k_weight_grad<1>, dim3(kGradWorkers, jobs[0].n), dim3(64 * gzmax[0]), stream, jobs[0], (const int64_t*)rows_dev);
        if (jobs[1].n) KPN_LAUNCH(k_weight_grad<2>, dim3(kGradWorkers, jobs[1].n), dim3(64 * gzmax[1]), stream, jobs[1], (const int64_t*)rows_dev);
        if (jobs[2].n) KPN_LAUNCH(k_weight_grad<4>, dim3(kGradWorkers, jobs[2].n), dim3(64 * gzmax[2]), stream, jobs[2], (const int64_t*)rows_dev);
        int gz_all = gzmax[0] > gzmax[1] ? gzmax[0] : gzmax[1];
        if (gzmax[2] > gz_all) gz_all = gzmax[2];
        const int mv_all = jobs[2].n ? 4 : (jobs[1].n ? 2 : 1);
        if (all.n) KPN_LAUNCH(k_weight_grad_reduce, dim3((mv_all * 2048 + mv_all * 32 + 31) / 32, gz_all, all.n), dim3(256), stream, all,
                              (int)kGradWorkers);
    };
    for (int64_t c0 = 0; c0 < N; c0 += L.chunk) {
        const int64_t n = (N - c0 < L.chunk) ? (N - c0) : L.chunk;
        const kpn_points ps = marched ? *marched
                                      : kpn_points{pts + c0 * 3, (view ? view : pts) + c0 * 3, nullptr, nullptr, nullptr, 1,
                                                   noise ? noise + c0 : nullptr, noise_std};
        reset_jobs();
        hipMemsetAsync(count, 0, 8 * sizeof(int), (hipStream_t)stream);
        const int* vcount = count;  // valid count of this pass
        float* xscr = full ? fp(L.xscr) : nullptr;
        if (fwd_query_ws && full) {
            const QueryLayout Q = query_layout(n, V);
            char* qb = static_cast<char*>(fwd_query_ws);
            vcount = reinterpret_cast<const int*>(qb + Q.count);
            list = reinterpret_cast<int*>(qb + Q.list);
            xscr = reinterpret_cast<float*>(qb + Q.xscr);
        } else {
            const int ppt = mask_points_per_thread(n);
            KPN_LAUNCH(k_mask_compact, grid1d(n, 256 * ppt), dim3(256), stream, sc, ps, n, 0, 1, ppt, wp + kpn_scalar_off(), (float*)nullptr,
                       (uint8_t*)nullptr, list, count);
        }
        KPN_LAUNCH(k_bwd_rows, dim3(1), dim3(1), stream, vcount, V, rows_dev);
        bwd_prof_pass(vcount, V, keep_mask, stream);
        if (full) {
            if (!fwd_query_ws) {
                KPN_BPROF(BP_ROWS_FWD);
                KPN_LAUNCH(k_geo_rows, dim3(blocks), dim3(256), stream, sc, ps, wp, (const int*)list, vcount, count + 1, xscr,
                           kpn_batch{0, 1 << 30});
            }
            if (full == 2) {
                KPN_BPROF(BP_COLOR_BWD);
                if (V <= 3)
                    KPN_LAUNCH(k_color_bwd<3>, dim3(blocks), dim3(256), stream, sc, ps, wp, (const int*)list, vcount, count + 4,
                               (const float*)xscr, d_out + c0 * 5, C);
                else
                    KPN_LAUNCH(k_color_bwd<KPN_MAXV>, dim3(blocks), dim3(256), stream, sc, ps, wp, (const int*)list, vcount, count + 4,
                               (const float*)xscr, d_out + c0 * 5, C);
            }
            if (full == 2) {
                wgrad(1, 0, C.Do2, 2, 1, C.Xo2, 8, 8, 8, P_O_2, 0, 0);
                wgrad(1, 0, C.Do1, 8, 8, C.Xo1, 16, 16, 16, P_O_1, 0, 0);
                wgrad(1, 0, C.Do0, 16, 16, C.Xo0, KPN_LD_XO0, KPN_LD_XO0, 37, P_O_0, 0, 0);
                wgrad(1, 0, C.Dv21, 2, 1, C.Xv21, 32, 32, 32, P_V2_1, 0, 0);
                wgrad(1, 0, C.Dv20, 32, 32, C.Xv20, 32, 32, 32, P_V2_0, 0, 0);
                wgrad(2, 0, C.Dv11, KPN_LD_DV11, 33, C.Xv11, 32, 32, 32, P_V1_1, 0, 0);
                wgrad(1, 0, C.Dv10, 32, 32, C.Xv10, 32, 32, 32, P_V1_0, 0, 0);
                wgrad(1, 0, C.Dbl1, 32, 32, C.Xb1, 64, 64, 64, P_BL_1, 0, 0);
                wgrad(2, 0, C.Dbl0, 64, 64, C.Xbl, KPN_LD_XBL, KPN_LD_XBL, KPN_LD_XBL, P_BL_0, 2, 0);
                wgrad(2, 0, C.Dre1, KPN_LD_XDIR, 35, C.Xe1, 16, 16, 16, P_RE_1, 0, 1);
                wgrad(1, 0, C.Dre0, 16, 16, C.Xrd, 4, 4, 4, P_RE_0, 0, 0);
            }
            {
                KPN_BPROF(BP_FUSE_BWD);
                KPN_LAUNCH(k_fuse_bwd, dim3(blocks), dim3(256), stream, sc, ps, wp, (const int*)list, vcount, count + 2,
                           (const float*)xscr, mode, d_out + c0 * 5, F);
            }
            wgrad(2, 1, F.D20, 64, 64, F.Xp, 128, 128, 128, P_G2_0, 0, 0);
            wgrad(2, 1, F.D21, 64, 64, F.Xh0, 64, 64, 64, P_G2_1, 0, 0);
            wgrad(1, 1, F.D22, 2, 2, F.Xh1, 64, 64, 64, P_G2_2, 0, 0);
            if (full == 2) wgrad(1, 1, C.Dcmp, 24, 24, F.Xp, 128, 128, 128, P_CMP, 0, 0);
        }
        {
            KPN_BPROF(BP_ROWS_BWD);
            KPN_LAUNCH(k_geo_rows_bwd, dim3(blocks), dim3(256), stream, sc, ps, wp, (const int*)list, vcount, count + 3,
                       full ? (const float*)F.dxrows : d_x + c0 * V * 64, full ? 1 : 0, B);
        }
        wgrad(4, 0, B.D0, 128, 128, B.X0, KPN_LDX0, 232, 232, P_G1_0, 1, 0);
        wgrad(4, 0, B.D1, 128, 128, B.X1, 128, 128, 128, P_G1_1, 0, 0);
        wgrad(4, 0, B.D2, 128, 120, B.X2, KPN_LDX2, 136, 136, P_G1_2, 0, 0);
        wgrad(2, 0, B.D3, 64, 64, B.X3, 128, 120, 120, P_G1_3, 0, 0);
        if (overflow) return fail(KPN_EWORKSPACE, "weight-gradient scratch too small (internal)");
        {
            KPN_BPROF(BP_WGRAD);
            run_jobs();
        }
    }
    return check_launch("field backward");
}
}  // namespace

extern "C" size_t kpn_geo_rows_backward_workspace_bytes(int64_t N, int32_t V) {
    if (N <= 0 || V <= 0) return 0;
    return bwd_layout(N, V, 0).total;
}

extern "C" int kpn_geo_rows_backward(const kpn_scene_desc* d, const void* scene_ws, const float* wp, int64_t N,
                                     const float* pts, uint32_t keep_mask, const float* d_x, float* d_plain, float* d_geo0,
                                     float* d_geo1, void* ws, size_t ws_bytes, void* stream) {
    if (int e = check_desc(d)) return e;
    KPN_REQUIRE(N >= 0 && N < (1ll << 31), "point count out of range");
    if (N == 0) return KPN_OK;
    KPN_REQUIRE(scene_ws && wp && pts && d_x && d_plain && d_geo0 && d_geo1 && ws, "null pointer");
    return run_backward(d, scene_ws, wp, N, pts, nullptr, 0, keep_mask, nullptr, 0.0f, d_x, nullptr, d_plain, d_geo0, d_geo1, nullptr,
                        ws, ws_bytes, stream);
}

extern "C" size_t kpn_query_backward_geometry_workspace_bytes(int64_t N, int32_t V) {
    if (N <= 0 || V <= 0) return 0;
    return bwd_layout(N, V, 1).total;
}

extern "C" int kpn_query_backward_geometry(const kpn_scene_desc* d, const void* scene_ws, const float* wp, int64_t N,
                                           const float* pts, int32_t mode, uint32_t keep_mask, const float* noise,
                                           float noise_std, const float* d_out, float* d_plain, float* d_geo0, float* d_geo1,
                                           void* ws, size_t ws_bytes, void* stream) {
    if (int e = check_desc(d)) return e;
    KPN_REQUIRE(mode == 0 || mode == 1, "mode must be 0 (raw query) or 1 (eval_func)");
    KPN_REQUIRE(N >= 0 && N < (1ll << 31), "point count out of range");
    if (N == 0) return KPN_OK;
    KPN_REQUIRE(scene_ws && wp && pts && d_out && d_plain && d_geo0 && d_geo1 && ws, "null pointer");
    return run_backward(d, scene_ws, wp, N, pts, nullptr, mode, keep_mask, noise, noise_std, nullptr, d_out, d_plain, d_geo0,
                        d_geo1, nullptr, ws, ws_bytes, stream);
}

extern "C" size_t kpn_query_backward_workspace_bytes(int64_t N, int32_t V) {
    if (N <= 0 || V <= 0) return 0;
    return bwd_layout(N, V, 2).total;
}

extern "C" int kpn_query_backward(const kpn_scene_desc* d, const void* scene_ws, const float* wp, int64_t N, const float* pts,
                                  const float* view, int32_t mode, uint32_t keep_mask, const float* noise, float noise_std,
                                  const float* d_out, float* d_plain, float* d_geo0, float* d_geo1, float* d_tex, void* ws,
                                  size_t ws_bytes, void* stream) {
    if (int e = check_desc(d)) return e;
    KPN_REQUIRE(mode == 0 || mode == 1, "mode must be 0 (raw query) or 1 (eval_func)");
    KPN_REQUIRE(N >= 0 && N < (1ll << 31), "point count out of range");
    if (N == 0) return KPN_OK;
    KPN_REQUIRE(scene_ws && wp && pts && view && d_out && d_plain && d_geo0 && d_geo1 && d_tex && ws, "null pointer");
    return run_backward(d, scene_ws, wp, N, pts, view, mode, keep_mask, noise, noise_std, nullptr, d_out, d_plain, d_geo0, d_geo1,
                        d_tex, ws, ws_bytes, stream);
}

// ---------------------------------------------------------------------------------------------
// backward of the field evaluation
namespace {
const int64_t kBwdChunk = 262144;  // points per pass: V=3 -> 786432 rows x 4.3 KB of dumps = 3.4 GB
static_assert(kBwdChunk <= 262144, "kUncappedPoints (query_layout) must cover a backward pass");
#ifndef KPN_GRAD_WORKERS
#define KPN_GRAD_WORKERS 512    // 2 workgroups per CU
#endif
const int kGradWorkers = kEmu ? 3 : KPN_GRAD_WORKERS;   // row workers (one workgroup each; its waves are the column groups)
const int kPartialUnits = 72;   // capacity of the partial-tile scratch in units of (workers x 2048 floats)
// ---- the buffers one kernel of the backward dumps for another, and the weight-gradient jobs that read them: two tables ----
struct BwdBufs { kpn_bwd_bufs B; kpn_fuse_bwd_bufs F; kpn_color_bufs C; };   // what the kernels take by value
// the part of the workspace a dump is carved in, and the `full` (bwd_layout) from which a pass has it
enum { PART_GEO = 0, PART_FUSE, PART_DXROWS, PART_COLOR, PART_CMP };
const int kPartFull[5] = {0, 1, 1, 2, 2};
enum { U_X0 = 0, U_X1, U_X2, U_X3, U_D0, U_D1, U_D2, U_D3, U_XP, U_XH0, U_XH1, U_D20, U_D21, U_D22, U_DXROWS,
       U_XRD, U_XE1, U_XDIR, U_XBL, U_XB1, U_XA, U_XV10, U_XV11, U_XT33, U_XV20, U_XV21, U_XO0, U_XO1, U_XO2,
       U_DO2, U_DO1, U_DO0, U_DV21, U_DV20, U_DV11, U_DV10, U_DBL1, U_DBL0, U_DRE1, U_DRE0, U_DCMP, U_COUNT };
// ld: floats per row, one row per (point, view) or (FUSE, CMP) per point.  The only place a leading dimension is written.
struct Dump { int id; size_t member; int ld; int part; };
#define D(id, member, ld, part) {U_##id, offsetof(BwdBufs, member), ld, PART_##part}
constexpr Dump kDumps[U_COUNT] = {
    // k_geo_rows_bwd: the inputs X and the dA of layers1
    D(X0, B.X0, KPN_LDX0, GEO), D(X1, B.X1, 128, GEO), D(X2, B.X2, KPN_LDX2, GEO), D(X3, B.X3, 128, GEO),
    D(D0, B.D0, 128, GEO), D(D1, B.D1, 128, GEO), D(D2, B.D2, 128, GEO), D(D3, B.D3, 64, GEO),
    // k_fuse_bwd: layers2 per point, and the d x_view rows k_geo_rows_bwd starts from
    D(XP, F.Xp, 128, FUSE), D(XH0, F.Xh0, 64, FUSE), D(XH1, F.Xh1, 64, FUSE), D(D20, F.D20, 64, FUSE), D(D21, F.D21, 64, FUSE), D(D22, F.D22, 2, FUSE),
    D(DXROWS, F.dxrows, 64, DXROWS),
    // k_color_bwd: the colour head, in kpn_color_bufs order (X buffers then dA buffers); one block of the workspace
    D(XRD, C.Xrd, 4, COLOR), D(XE1, C.Xe1, 16, COLOR), D(XDIR, C.Xdir, KPN_LD_XDIR, COLOR), D(XBL, C.Xbl, KPN_LD_XBL, COLOR), D(XB1, C.Xb1, 64, COLOR),
    D(XA, C.Xa, 32, COLOR), D(XV10, C.Xv10, 32, COLOR), D(XV11, C.Xv11, 32, COLOR), D(XT33, C.Xt33, 2, COLOR), D(XV20, C.Xv20, 32, COLOR),
    D(XV21, C.Xv21, 32, COLOR), D(XO0, C.Xo0, KPN_LD_XO0, COLOR), D(XO1, C.Xo1, 16, COLOR), D(XO2, C.Xo2, 8, COLOR),
    D(DO2, C.Do2, 2, COLOR), D(DO1, C.Do1, 8, COLOR), D(DO0, C.Do0, 16, COLOR), D(DV21, C.Dv21, 2, COLOR), D(DV20, C.Dv20, 32, COLOR),
    D(DV11, C.Dv11, KPN_LD_DV11, COLOR), D(DV10, C.Dv10, 32, COLOR), D(DBL1, C.Dbl1, 32, COLOR), D(DBL0, C.Dbl0, 64, COLOR),
    D(DRE1, C.Dre1, KPN_LD_XDIR, COLOR), D(DRE0, C.Dre0, 16, COLOR),
    D(DCMP, C.Dcmp, 24, CMP),   // d lat per point
};
#undef D
constexpr bool dumps_in_order() { for (int i = 0; i < U_COUNT; ++i) if (kDumps[i].id != i) return false; return true; }
static_assert(dumps_in_order(), "kDumps is indexed by the U_* enumerators");
constexpr bool per_point(const Dump& m) { return m.part == PART_FUSE || m.part == PART_CMP; }
float*& dump_slot(BwdBufs& u, const Dump& m) { return *reinterpret_cast<float**>(reinterpret_cast<char*>(&u) + m.member); }

// dW[layer] += dY^T X over the (point, view) rows or the points of a pass (whichever X is dumped per); ldy / ldx are the dumps'.
// M: outputs; Kc: columns of the X dump read (even); Kt: real input features.  In the order the jobs are queued, which fixes
// their shares of the partial / bias scratch.
enum { ST_COLOR = 0, ST_LAYERS2, ST_COMPRESS, ST_LAYERS1 };
struct WgradRow { int stage, dY, X, M, Kc, Kt, layer, mv, cmap, omap; };
const WgradRow kWgrad[19] = {
    {ST_COLOR, U_DO2, U_XO2, 1, 8, 8, P_O_2, 1, 0, 0},
    {ST_COLOR, U_DO1, U_XO1, 8, 16, 16, P_O_1, 1, 0, 0},
    {ST_COLOR, U_DO0, U_XO0, 16, KPN_LD_XO0, 37, P_O_0, 1, 0, 0},
    {ST_COLOR, U_DV21, U_XV21, 1, 32, 32, P_V2_1, 1, 0, 0},
    {ST_COLOR, U_DV20, U_XV20, 32, 32, 32, P_V2_0, 1, 0, 0},
    {ST_COLOR, U_DV11, U_XV11, 33, 32, 32, P_V1_1, 2, 0, 0},
    {ST_COLOR, U_DV10, U_XV10, 32, 32, 32, P_V1_0, 1, 0, 0},
    {ST_COLOR, U_DBL1, U_XB1, 32, 64, 64, P_BL_1, 1, 0, 0},
    {ST_COLOR, U_DBL0, U_XBL, 64, KPN_LD_XBL, KPN_LD_XBL, P_BL_0, 2, 2, 0},
    {ST_COLOR, U_DRE1, U_XE1, 35, 16, 16, P_RE_1, 2, 0, 1},
    {ST_COLOR, U_DRE0, U_XRD, 16, 4, 4, P_RE_0, 1, 0, 0},
    {ST_LAYERS2, U_D20, U_XP, 64, 128, 128, P_G2_0, 2, 0, 0},
    {ST_LAYERS2, U_D21, U_XH0, 64, 64, 64, P_G2_1, 2, 0, 0},
    {ST_LAYERS2, U_D22, U_XH1, 2, 64, 64, P_G2_2, 1, 0, 0},
    {ST_COMPRESS, U_DCMP, U_XP, 24, 128, 128, P_CMP, 1, 0, 0},
    {ST_LAYERS1, U_D0, U_X0, 128, 232, 232, P_G1_0, 4, 1, 0},
    {ST_LAYERS1, U_D1, U_X1, 128, 128, 128, P_G1_1, 4, 0, 0},
    {ST_LAYERS1, U_D2, U_X2, 120, 136, 136, P_G1_2, 4, 0, 0},
    {ST_LAYERS1, U_D3, U_X3, 64, 120, 120, P_G1_3, 2, 0, 0},
};
static_assert(sizeof(kWgrad) / sizeof(kWgrad[0]) <= KPN_WGRAD_MAX_JOBS, "a pass queues every job");

struct BwdLayout { size_t count, list, partial, dbp, xscr, dump[U_COUNT], total; int64_t chunk; };
// full: 0 = geometry rows only; 1 = whole query (adds the forward row scratch, the per-point dumps and the d x_view rows), geometry
// outputs; 2 = whole query incl. the colour head
BwdLayout bwd_layout(int64_t N, int V, int full) {
    BwdLayout L{};
    L.chunk = N < kBwdChunk ? N : kBwdChunk;
    const size_t ntiles = (size_t)((L.chunk + KPN_TILE - 1) / KPN_TILE);
    const size_t npts = ntiles * KPN_TILE, rows = npts * V;
    Carver c;
    auto dump_bytes = [&](const Dump& m) { return (per_point(m) ? npts : rows) * m.ld * 4; };
    auto take_part = [&](int part) { for (const Dump& m : kDumps) if (m.part == part) L.dump[m.id] = c.take(dump_bytes(m)); };
    L.count = c.take(256);
    L.list = c.take((size_t)L.chunk * sizeof(int));
    take_part(PART_GEO);
    // partial tile blocks of all weight-gradient jobs of a pass (they run in shared launches): sum over the 19 layers of
    // column groups x MV = 65 -> 72 x workers x 8 KB (checked when the jobs are queued); bias partials per job
    L.partial = c.take((size_t)kPartialUnits * kGradWorkers * (2 * 16 * 64) * 4);
    L.dbp = c.take((size_t)KPN_WGRAD_MAX_JOBS * kGradWorkers * 4 * 64 * 4);
    if (full) {
        L.xscr = c.take(ntiles * (size_t)V * KPN_ROW_SLABS * 64 * sizeof(float4));
        take_part(PART_FUSE);
        take_part(PART_DXROWS);
    }
    if (full == 2) {
        size_t color_bytes = 0;   // the colour head's dumps follow each other in one block
        for (const Dump& m : kDumps) if (m.part == PART_COLOR) { L.dump[m.id] = c.o + color_bytes; color_bytes += dump_bytes(m); }
        c.take(color_bytes);
        take_part(PART_CMP);
    }
    L.total = c.o;
    return L;
}
size_t bwd_workspace_bytes(int64_t N, int V, int full) { return (N <= 0 || V <= 0) ? 0 : bwd_layout(N, V, full).total; }
// The keypoint gradient's scratch (kpt_grad_kernels.hip), BEHIND a pass's layout so that no existing offset or size moves: the
// transposed encoding operand of layers1.0, then the workgroups' fp64 partials [workers][V][KPN_KG_Q].
const int kKptWorkers = kEmu ? 3 : 256;   // one workgroup per CU and view
struct KptLayout { size_t wt, partial, partial_bytes, total; };
KptLayout kpt_layout(size_t base, int V) {
    KptLayout K{};
    Carver c;
    c.o = align_up(base, 256);
    K.wt = c.take((size_t)KPN_KG_WT_FLOATS * 4);
    K.partial_bytes = (size_t)kKptWorkers * V * KPN_KG_Q * sizeof(double);
    K.partial = c.take(K.partial_bytes);
    K.total = c.o;
    return K;
}
size_t bwd_workspace_bytes_kpt(int64_t N, int V, int full) { return (N <= 0 || V <= 0) ? 0 : kpt_layout(bwd_layout(N, V, full).total, V).total; }
}  // namespace

// rows[0] = (point, view) rows of the current pass, rows[1] = points, both padded to whole tiles
__global__ void k_bwd_rows(const int* __restrict__ count, int V, int64_t* __restrict__ rows) {
    const int64_t npts = (int64_t)((*count + KPN_TILE - 1) / KPN_TILE) * KPN_TILE;
    rows[0] = npts * V;
    rows[1] = npts;
}

namespace {
// One backward pass over N points, as its callers name it: explicit points (with their view and noise) or ray-marched ones (cam_pos +
// dirs * z, as kpn_render_rays evaluates them; one pass only, N <= kBwdChunk).  d_x: geometry rows only, upstream gradient per (point,
// view); otherwise the whole-query reverse from d_out (N,5): its geometry columns only (d_tex == nullptr) or all five incl. the colour
// head.  fwd_query_ws: the workspace a run_field() call on the SAME points just used: its valid list and row scratch are reused.
struct BackwardPass {
    int64_t N = 0; int mode = 0; uint32_t keep_mask = 0xFFFFFFFFu;
    const float *pts = nullptr, *view = nullptr, *noise = nullptr; float noise_std = 0.0f; const kpn_points* marched = nullptr;
    const float *d_x = nullptr, *d_out = nullptr; float *d_plain = nullptr, *d_geo0 = nullptr, *d_geo1 = nullptr, *d_tex = nullptr;
    void* ws = nullptr; size_t ws_bytes = 0; void* fwd_query_ws = nullptr;
    float* d_kpt = nullptr; int n_kpt = 0;   // optional: d loss / d kpt3d (n_kpt, 3), added to; ws then holds kpt_layout() as well
};
int run_backward(const kpn_scene_desc* d, const void* scene_ws, const float* wp, const BackwardPass& p, void* stream) {
    const int V = d->n_views;
    const int full = p.d_x != nullptr ? 0 : (p.d_tex ? 2 : 1);
    const BwdLayout L = bwd_layout(p.N, V, full);
    if (p.ws_bytes < L.total) return fail(KPN_EWORKSPACE, "backward workspace too small");
    const KptLayout K = kpt_layout(L.total, V);
    if (p.d_kpt) {
        KPN_REQUIRE(p.n_kpt >= 1 && p.n_kpt <= KPN_NKPT, "n_kpt in 1..24");
        if (p.ws_bytes < K.total) return fail(KPN_EWORKSPACE, "backward workspace too small for the keypoint gradient");
    }
    if (p.marched && p.N > L.chunk) return fail(KPN_EINVAL, "ray-marched backward pass too large");
    kpn_scene_dev sc = scene_dev(d, scene_ws);
    sc.keep = p.keep_mask;
    char* base = static_cast<char*>(p.ws);
    auto fp = [&](size_t off) { return reinterpret_cast<float*>(base + off); };
    int* count = reinterpret_cast<int*>(base + L.count);  // [0] valid count, [1..3] work tickets of the three persistent kernels
    int64_t* rows_dev = reinterpret_cast<int64_t*>(base + L.count + 64);
    int* list = reinterpret_cast<int*>(base + L.list);
    BwdBufs u{};   // the dumps this pass has; the others stay null
    for (const Dump& m : kDumps) if (full >= kPartFull[m.part]) dump_slot(u, m) = fp(L.dump[m.id]);
    u.B.dgeo0 = p.d_geo0; u.B.dgeo1 = p.d_geo1;
    if (full == 2) {
        u.C.dtex = p.d_tex;
        u.C.dani = p.d_plain + kpn_plain_weight_floats() - 1;
        u.F.Dcmp = u.C.Dcmp;
    }
    const int blocks = field_grid_blocks();
    // rows of views switched off by the train-time dropout are skipped by k_color_bwd (their dumps are never written) and carry a
    // zero upstream gradient in k_geo_rows_bwd: k_weight_grad reads them as zeros by the same mask (no memset of the dumps)
    const uint32_t wgrad_keep = p.keep_mask | ~((V >= 32) ? 0xFFFFFFFFu : ((1u << V) - 1u));
    // weight-gradient jobs of a pass: queued stage by stage while the producers are launched, then run in one launch per MV class
    // and one reduce launch
    kpn_wgrad_jobs jobs[3], all;  // MV = 1, 2, 4
    int gzmax[3];
    size_t partial_used = 0;
    bool overflow = false;
    auto queue_jobs = [&](int stage) {
        for (const WgradRow& r : kWgrad) {
            if (r.stage != stage) continue;
            const Dump &dy = kDumps[r.dY], &x = kDumps[r.X];
            const int cls = r.mv == 1 ? 0 : (r.mv == 2 ? 1 : 2);
            const int gz = (r.Kc + 63) / 64;
            kpn_wgrad_job j;
            j.dY = dump_slot(u, dy); j.X = dump_slot(u, x); j.ldy = dy.ld; j.M = r.M; j.ldx = x.ld; j.Kc = r.Kc; j.Kt = r.Kt;
            j.cmap = r.cmap; j.omap = r.omap; j.mv = r.mv;
            j.which = per_point(x) ? 1 : 0;   // rows[which] (k_bwd_rows) = the job's row count
            j.V = per_point(x) ? 1 : V; j.keep = per_point(x) ? 0xFFFFFFFFu : wgrad_keep;
            j.partial = fp(L.partial) + partial_used;
            partial_used += (size_t)gz * kGradWorkers * r.mv * 2048;
            if (partial_used > (size_t)kPartialUnits * kGradWorkers * 2048 || all.n >= KPN_WGRAD_MAX_JOBS) { overflow = true; continue; }
            j.dbp = fp(L.dbp) + (size_t)all.n * kGradWorkers * 4 * 64;
            j.dW = p.d_plain + plain_w_off(r.layer);
            j.dB = p.d_plain + plain_b_off(r.layer);
            j.in_dim = plain_dims[r.layer][1];
            jobs[cls].j[jobs[cls].n++] = j;
            all.j[all.n++] = j;
            if (gz > gzmax[cls]) gzmax[cls] = gz;
        }
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
    if (p.d_kpt) {
        hipMemsetAsync(base + K.partial, 0, K.partial_bytes, (hipStream_t)stream);
        KPN_LAUNCH(k_kpt_grad_pack, grid1d(KPN_KG_WT_FLOATS, 256), dim3(256), stream, wp, fp(K.wt));
    }
    for (int64_t c0 = 0; c0 < p.N; c0 += L.chunk) {
        const int64_t n = (p.N - c0 < L.chunk) ? (p.N - c0) : L.chunk;
        const kpn_points ps = p.marched ? *p.marched
                                        : kpn_points{p.pts + c0 * 3, (p.view ? p.view : p.pts) + c0 * 3, nullptr, nullptr, nullptr, 1,
                                                     p.noise ? p.noise + c0 : nullptr, p.noise_std};
        jobs[0].n = jobs[1].n = jobs[2].n = all.n = 0; gzmax[0] = gzmax[1] = gzmax[2] = 0; partial_used = 0;
        hipMemsetAsync(count, 0, 8 * sizeof(int), (hipStream_t)stream);
        const int* vcount = count;  // valid count of this pass
        float* xscr = full ? fp(L.xscr) : nullptr;
        if (p.fwd_query_ws && full) {
            const QueryLayout Q = query_layout(n, V);
            char* qb = static_cast<char*>(p.fwd_query_ws);
            vcount = reinterpret_cast<const int*>(qb + Q.count);
            list = reinterpret_cast<int*>(qb + Q.list);
            xscr = reinterpret_cast<float*>(qb + Q.xscr);
        } else {
            const int ppt = mask_points_per_thread(n);
            KPN_LAUNCH(k_mask_compact, grid1d(n, 256 * ppt), dim3(256), stream, sc, ps, n, 0, 1, ppt, wp + kpn_scalar_off(), (float*)nullptr,
                       (uint8_t*)nullptr, list, count);
        }
        KPN_LAUNCH(k_bwd_rows, dim3(1), dim3(1), stream, vcount, V, rows_dev);
        bwd_prof_pass(vcount, V, p.keep_mask, stream);
        if (full) {
            if (!p.fwd_query_ws) {
                KPN_BPROF(BP_ROWS_FWD);
                KPN_LAUNCH(k_geo_rows, dim3(blocks), dim3(256), stream, sc, ps, wp, (const int*)list, vcount, count + 1, xscr,
                           kpn_batch{0, 1 << 30});
            }
            if (full == 2) {
                KPN_BPROF(BP_COLOR_BWD);
                if (V <= 3)
                    KPN_LAUNCH(k_color_bwd<3>, dim3(blocks), dim3(256), stream, sc, ps, wp, (const int*)list, vcount, count + 4,
                               (const float*)xscr, p.d_out + c0 * 5, u.C);
                else
                    KPN_LAUNCH(k_color_bwd<KPN_MAXV>, dim3(blocks), dim3(256), stream, sc, ps, wp, (const int*)list, vcount, count + 4,
                               (const float*)xscr, p.d_out + c0 * 5, u.C);
            }
            if (full == 2) queue_jobs(ST_COLOR);
            {
                KPN_BPROF(BP_FUSE_BWD);
                KPN_LAUNCH(k_fuse_bwd, dim3(blocks), dim3(256), stream, sc, ps, wp, (const int*)list, vcount, count + 2,
                           (const float*)xscr, p.mode, p.d_out + c0 * 5, u.F);
            }
            queue_jobs(ST_LAYERS2);
            if (full == 2) queue_jobs(ST_COMPRESS);
        }
        {
            KPN_BPROF(BP_ROWS_BWD);
            KPN_LAUNCH(k_geo_rows_bwd, dim3(blocks), dim3(256), stream, sc, ps, wp, (const int*)list, vcount, count + 3,
                       full ? (const float*)u.F.dxrows : p.d_x + c0 * V * 64, full ? 1 : 0, u.B);
        }
        if (p.d_kpt) {   // reads the D0 and X0 dumps of the launch above
            const kpn_kpt_grad_args ka{u.B.D0, u.B.X0, fp(K.wt), reinterpret_cast<double*>(base + K.partial), p.n_kpt, wgrad_keep};
            KPN_LAUNCH(k_kpt_grad, dim3(kKptWorkers, V), dim3(256), stream, sc, ps, (const int*)list, vcount, ka);
        }
        queue_jobs(ST_LAYERS1);
        if (overflow) return fail(KPN_EWORKSPACE, "weight-gradient scratch too small (internal)");
        {
            KPN_BPROF(BP_WGRAD);
            run_jobs();
        }
    }
    if (p.d_kpt)
        KPN_LAUNCH(k_kpt_grad_finish, dim3(p.n_kpt), dim3(256), stream, sc, (const double*)reinterpret_cast<double*>(base + K.partial),
                   (int)kKptWorkers, p.d_kpt);
    return check_launch("field backward");
}
}  // namespace

extern "C" size_t kpn_geo_rows_backward_workspace_bytes(int64_t N, int32_t V) { return bwd_workspace_bytes(N, V, 0); }

extern "C" int kpn_geo_rows_backward(const kpn_scene_desc* d, const void* scene_ws, const float* wp, int64_t N,
                                     const float* pts, uint32_t keep_mask, const float* d_x, float* d_plain, float* d_geo0,
                                     float* d_geo1, void* ws, size_t ws_bytes, void* stream) {
    if (int e = check_desc(d)) return e;
    KPN_REQUIRE(N >= 0 && N < (1ll << 31), "point count out of range");
    if (N == 0) return KPN_OK;
    KPN_REQUIRE(scene_ws && wp && pts && d_x && d_plain && d_geo0 && d_geo1 && ws, "null pointer");
    BackwardPass p;
    p.N = N; p.pts = pts; p.keep_mask = keep_mask; p.d_x = d_x;
    p.d_plain = d_plain; p.d_geo0 = d_geo0; p.d_geo1 = d_geo1; p.ws = ws; p.ws_bytes = ws_bytes;
    return run_backward(d, scene_ws, wp, p, stream);
}

extern "C" size_t kpn_geo_rows_backward_workspace_bytes_kpt(int64_t N, int32_t V) { return bwd_workspace_bytes_kpt(N, V, 0); }

extern "C" int kpn_geo_rows_backward_kpt(const kpn_scene_desc* d, const void* scene_ws, const float* wp, int64_t N,
                                         const float* pts, uint32_t keep_mask, const float* d_x, float* d_plain, float* d_geo0,
                                         float* d_geo1, float* d_kpt3d, int32_t n_kpt, void* ws, size_t ws_bytes, void* stream) {
    if (int e = check_desc(d)) return e;
    KPN_REQUIRE(N >= 0 && N < (1ll << 31), "point count out of range");
    KPN_REQUIRE(n_kpt >= 1 && n_kpt <= KPN_NKPT, "n_kpt in 1..24");
    if (N == 0) return KPN_OK;
    KPN_REQUIRE(scene_ws && wp && pts && d_x && d_plain && d_geo0 && d_geo1 && d_kpt3d && ws, "null pointer");
    BackwardPass p;
    p.N = N; p.pts = pts; p.keep_mask = keep_mask; p.d_x = d_x;
    p.d_plain = d_plain; p.d_geo0 = d_geo0; p.d_geo1 = d_geo1; p.ws = ws; p.ws_bytes = ws_bytes;
    p.d_kpt = d_kpt3d; p.n_kpt = n_kpt;
    return run_backward(d, scene_ws, wp, p, stream);
}

extern "C" size_t kpn_query_backward_geometry_workspace_bytes(int64_t N, int32_t V) { return bwd_workspace_bytes(N, V, 1); }

extern "C" int kpn_query_backward_geometry(const kpn_scene_desc* d, const void* scene_ws, const float* wp, int64_t N,
                                           const float* pts, int32_t mode, uint32_t keep_mask, const float* noise,
                                           float noise_std, const float* d_out, float* d_plain, float* d_geo0, float* d_geo1,
                                           void* ws, size_t ws_bytes, void* stream) {
    if (int e = check_desc(d)) return e;
    KPN_REQUIRE(mode == 0 || mode == 1, "mode must be 0 (raw query) or 1 (eval_func)");
    KPN_REQUIRE(N >= 0 && N < (1ll << 31), "point count out of range");
    if (N == 0) return KPN_OK;
    KPN_REQUIRE(scene_ws && wp && pts && d_out && d_plain && d_geo0 && d_geo1 && ws, "null pointer");
    BackwardPass p;
    p.N = N; p.pts = pts; p.mode = mode; p.keep_mask = keep_mask; p.noise = noise; p.noise_std = noise_std; p.d_out = d_out;
    p.d_plain = d_plain; p.d_geo0 = d_geo0; p.d_geo1 = d_geo1; p.ws = ws; p.ws_bytes = ws_bytes;
    return run_backward(d, scene_ws, wp, p, stream);
}

extern "C" size_t kpn_query_backward_workspace_bytes(int64_t N, int32_t V) { return bwd_workspace_bytes(N, V, 2); }

extern "C" int kpn_query_backward(const kpn_scene_desc* d, const void* scene_ws, const float* wp, int64_t N, const float* pts,
                                  const float* view, int32_t mode, uint32_t keep_mask, const float* noise, float noise_std,
                                  const float* d_out, float* d_plain, float* d_geo0, float* d_geo1, float* d_tex, void* ws,
                                  size_t ws_bytes, void* stream) {
    if (int e = check_desc(d)) return e;
    KPN_REQUIRE(mode == 0 || mode == 1, "mode must be 0 (raw query) or 1 (eval_func)");
    KPN_REQUIRE(N >= 0 && N < (1ll << 31), "point count out of range");
    if (N == 0) return KPN_OK;
    KPN_REQUIRE(scene_ws && wp && pts && view && d_out && d_plain && d_geo0 && d_geo1 && d_tex && ws, "null pointer");
    BackwardPass p;
    p.N = N; p.pts = pts; p.view = view; p.mode = mode; p.keep_mask = keep_mask; p.noise = noise; p.noise_std = noise_std; p.d_out = d_out;
    p.d_plain = d_plain; p.d_geo0 = d_geo0; p.d_geo1 = d_geo1; p.d_tex = d_tex; p.ws = ws; p.ws_bytes = ws_bytes;
    return run_backward(d, scene_ws, wp, p, stream);
}

extern "C" size_t kpn_query_backward_workspace_bytes_kpt(int64_t N, int32_t V) { return bwd_workspace_bytes_kpt(N, V, 2); }

extern "C" int kpn_query_backward_kpt(const kpn_scene_desc* d, const void* scene_ws, const float* wp, int64_t N, const float* pts,
                                      const float* view, int32_t mode, uint32_t keep_mask, const float* noise, float noise_std,
                                      const float* d_out, float* d_plain, float* d_geo0, float* d_geo1, float* d_tex, float* d_kpt3d,
                                      int32_t n_kpt, void* ws, size_t ws_bytes, void* stream) {
    if (int e = check_desc(d)) return e;
    KPN_REQUIRE(mode == 0 || mode == 1, "mode must be 0 (raw query) or 1 (eval_func)");
    KPN_REQUIRE(N >= 0 && N < (1ll << 31), "point count out of range");
    KPN_REQUIRE(n_kpt >= 1 && n_kpt <= KPN_NKPT, "n_kpt in 1..24");
    if (N == 0) return KPN_OK;
    KPN_REQUIRE(scene_ws && wp && pts && view && d_out && d_plain && d_geo0 && d_geo1 && d_tex && d_kpt3d && ws, "null pointer");
    BackwardPass p;
    p.N = N; p.pts = pts; p.view = view; p.mode = mode; p.keep_mask = keep_mask; p.noise = noise; p.noise_std = noise_std; p.d_out = d_out;
    p.d_plain = d_plain; p.d_geo0 = d_geo0; p.d_geo1 = d_geo1; p.d_tex = d_tex; p.ws = ws; p.ws_bytes = ws_bytes;
    p.d_kpt = d_kpt3d; p.n_kpt = n_kpt;
    return run_backward(d, scene_ws, wp, p, stream);
}

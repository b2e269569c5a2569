// ---------------------------------------------------------------------------------------------
// field query
namespace {
// ---- the knobs of api_field.hip, api_backward.hip and api_render.hip: the only place they are read ----
//   knob                          default              read           set by
//   row scratch cap               3 GiB (emu: 1 MiB)   once, lazily   KPN_ROW_SCRATCH_MIB, kpn_set_row_scratch_cap_bytes (>= 1 MiB)
//   rows mode (layers1 kernel)    3                    once, lazily   kpn_set_geo_rows_mode (0 / 2 / 3); per call kpn_render_args.rows_kernel
//   fuse mode (per-point kernel)  1                    once, lazily   kpn_set_fuse_mode (0 / 1); per call kpn_render_args.fuse_kernel
//   density first                 2 (auto)             once, lazily   KPN_DENSITY_FIRST=0/1/2, kpn_set_density_first
//   range guard                   on                   once, lazily   KPN_NO_RANGE_GUARD=1, kpn_set_range_guard
//   KPN_NO_POOL                   off                  once, lazily   environment only (A/B: the ROWS layout in every pass)
//   KPN_NO_FUSE_H3                off                  per call       environment only (A/B and tests: the generic kernel for V = 3 as well)
//   KPN_NO_ZERO_SKIP              off                  per call       environment only (A/B: no zero-density short path)
//   KPN_NO_COARSE_REUSE           off                  per call       environment only (A/B and tests: the fine pass evaluates every sample)
// A process-wide integer setting: unset until its first read, which takes init() — the environment's value or the default; the
// kpn_set_* entry points overwrite it.
struct Setting { long long value = -1; template <class Init> long long get(Init init) { if (value < 0) value = init(); return value; } };
// a boolean knob of the environment: set and not 0.  Per call where it is called per call (tests flip those with monkeypatch).
bool env_flag(const char* name) { const char* e = getenv(name); return e && atoi(e) != 0; }
#ifdef KPN_SIMT_EMU   // the emulator's sizes: small, so that its tests walk the multi-block and multi-batch paths
const bool kEmu = true;
#else
const bool kEmu = false;
#endif
Setting g_row_scratch_cap, g_geo_rows_mode, g_fuse_mode, g_density_first, g_range_guard, g_no_pool;

// The row scratch (10 KB per valid tile and view) is capped: a pass with more valid tiles than fit is evaluated in
// batches that reuse it (kpn_batch, field_kernels.hip).  Sized for the worst case it was 32 GiB for a 512^2 frame at
// 64 + 64 samples — of which a scene uses the valid third; the cap keeps one pass per frame (one launch ramp, one
// weight staging) at a fixed, small footprint.  KPN_ROW_SCRATCH_MIB overrides the default of 3 GiB.
size_t row_scratch_cap_bytes() {
    return (size_t)g_row_scratch_cap.get([] {
        const char* e = getenv("KPN_ROW_SCRATCH_MIB");
        return (long long)((e ? (size_t)atoll(e) : (size_t)(kEmu ? 1 : 3072)) << 20);
    });
}
const int kMaxBatches = 60;
const size_t kCounterBytes = 2048;   // (8 + 8 * kMaxBatches) ints
static_assert((8 + 8 * kMaxBatches) * sizeof(int) <= kCounterBytes && kCounterBytes % 256 == 0, "counter block");
// passes of at most this many points always get their worst-case scratch (never batched): the backward entry points
// read a pass's rows again and work in passes of kBwdChunk points
const int64_t kUncappedPoints = kEmu ? 2048 : 262144;
struct QueryLayout { size_t count, list, live, xscr, total; int tiles_cap, nbatch; };  // byte offsets
// Rows kernel of layers1 (kpn_set_geo_rows_mode):
// 0: fp32 MFMA (v_mfma_f32_32x32x2_f32, k_geo_rows)
// 2: three bf16 pieces per operand, six products, two tiles per wave and ONE wave per SIMD (k_geo_rows_h2): fp32-class results
//    (every product term above 2^-24 relative is kept) in fp32's exponent range
// 3: two fp16 pieces per operand, three products (hh hl lh), same kernel structure (k_geo_rows_f2): the default — the same accuracy class
//    with 1.5x fewer MFMAs and a third of the split instructions; operands must stay within fp16's range, which the range guard
//    below takes care of
// (1 was the one-tile-per-wave split-bf16 kernel of round 1: not part of the library, scripts/mode1_investigation/)
#ifndef KPN_DEFAULT_GEO_ROWS_MODE
#define KPN_DEFAULT_GEO_ROWS_MODE 3
#endif
int geo_rows_mode() { return (int)g_geo_rows_mode.get([] { return (long long)KPN_DEFAULT_GEO_ROWS_MODE; }); }
// pool: the POOL layout of the scratch (kpn_field_shared.h): the render / query passes with the pair-tile rows kernels
bool pool_layout_selected() { return geo_rows_mode() >= 2 && !g_no_pool.get([] { return (long long)env_flag("KPN_NO_POOL"); }); }
QueryLayout query_layout(int64_t N, int V, bool pool = false) {
    QueryLayout L;
    Carver c;
    // [0] valid count; batch b owns ints [8 + 8b, 16 + 8b): [0] rows ticket, [1] per-point ticket, [2] live points of the batch and
    // [3] pass B's ticket (density-first render passes), [4] / [5] the tickets of the fp32-range kernels launched behind them (range
    // guard), [6] the batch's "non-finite result" flag
    L.count = c.take(kCounterBytes);
    L.list = c.take((size_t)N * sizeof(int));
    const size_t ntiles = (size_t)(N + KPN_TILE - 1) / KPN_TILE;
    const size_t tile_bytes = (size_t)kpn_tile_slabs(pool ? 1 : 0, V) * 64 * sizeof(float4);
    // monotone in N (a render workspace is laid out for its largest pass and used by smaller ones): never fewer tiles
    // than an uncapped pass of kUncappedPoints points needs
    size_t cap = row_scratch_cap_bytes() / tile_bytes;
    const size_t floor_tiles = (size_t)(kUncappedPoints + KPN_TILE - 1) / KPN_TILE;
    if (cap < floor_tiles) cap = floor_tiles;
    if ((ntiles + cap - 1) / cap > (size_t)kMaxBatches) cap = (ntiles + kMaxBatches - 1) / kMaxBatches;
    if (cap > ntiles) cap = ntiles ? ntiles : 1;
    L.tiles_cap = (int)cap;
    L.nbatch = (int)((ntiles + cap - 1) / cap);
    // the live list of ONE batch (density-first render passes, field_kernels.hip PHASE): scratch slots tile * 32 + point
    L.live = c.take(cap * KPN_TILE * sizeof(int));
    L.xscr = c.take(cap * tile_bytes);
    L.total = c.o;
    return L;
}
// persistent grid: 256 CUs x 2 blocks of 256 threads (launch_bounds(256,2) -> 8 waves per CU)
int field_grid_blocks() { return kEmu ? 8 : 512; }

// The per-point kernel: 1 = k_fuse_color_h (weights as two fp16 pieces per value on v_mfma_f32_32x32x16_f16: the default),
// 0 = k_fuse_color (fp32 weights on v_mfma_f32_32x32x2_f32).  Two mechanisms select it, no environment variable (round 5).
int fuse_mode() { return (int)g_fuse_mode.get([] { return 1ll; }); }
// Density first (field_kernels.hip, PHASE): the per-point work of a render pass as pass A (density of every listed point + the
// batch's live list) and pass B (colour of the live points) instead of the fused per-point kernel — where it applies (lean render
// passes, POOL layout, fuse mode 1).  kpn_set_density_first: 0 = never (the fused kernel), 1 = always, 2 = AUTO (the default;
// KPN_DENSITY_FIRST=0/1/2 sets the initial value): the pair wins when enough of the hull is empty and loses 0.16 ms per launch when
// nothing is (field_kernels.hip), so each render pass takes the form the dead fraction of the EARLIER passes calls for — the
// per-point kernels count listed / live points on the device (kpn_density_counts), a 16-byte copy into pinned host memory is queued
// behind every pass, and the next pass looks at whatever has arrived: no synchronisation, and since both forms give the same bits
// the choice never shows in a frame.  A stream that is being captured neither allocates nor copies (the captured graph keeps the
// form chosen at capture time).
int density_first() {
    return (int)g_density_first.get([] {
        const char* e = getenv("KPN_DENSITY_FIRST");
        return (long long)((e && e[0] >= '0' && e[0] <= '2' && e[1] == 0) ? e[0] - '0' : 2);
    });
}
const float kDensityFirstDeadFraction = 0.20f;   // AUTO: density first when at least this fraction of the hull's points was dead
struct DensityHint {
    unsigned long long* pinned = nullptr;   // [listed, live] as last copied from the device
    unsigned long long seen[2] = {0, 0};    // the snapshot the current decision was taken from
    double avg[2] = {0.0, 0.0};             // moving sums of listed / live points over the looks
    bool split = false;                     // nothing measured yet: the fused kernel
};
DensityHint g_density_hint[16];
DensityHint* density_hint() {
#ifndef KPN_SIMT_EMU
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return nullptr;
    return &g_density_hint[dev];
#else
    return &g_density_hint[0];
#endif
}
long long g_density_first_passes[2] = {0, 0};   // eligible passes run density first / on the fused kernel (kpn_density_first_passes)
// the form of THIS pass
bool density_first_now() {
    const int m = density_first();
    if (m != 2) return m == 1;
    DensityHint* hnt = density_hint();
    if (!hnt) return false;
#ifndef KPN_SIMT_EMU
    if (!hnt->pinned) return hnt->split;
    const unsigned long long now[2] = {hnt->pinned[0], hnt->pinned[1]};
#else
    const unsigned long long now[2] = {kpn_density_counts[0], kpn_density_counts[1]};
#endif
    const bool was_reset = now[0] < hnt->seen[0];
    const unsigned long long d0 = was_reset ? now[0] : now[0] - hnt->seen[0], d1 = was_reset ? now[1] : now[1] - hnt->seen[1];
    if (d0 > 0 && d1 <= d0) {
        // a look may cover one pass only (a coarse pass's hull is emptier than a fine pass's): the decision follows a moving
        // average over the last few looks, not the last one
        hnt->avg[0] = 0.5 * hnt->avg[0] + (double)d0;
        hnt->avg[1] = 0.5 * hnt->avg[1] + (double)d1;
        hnt->split = (hnt->avg[0] - hnt->avg[1]) >= (double)kDensityFirstDeadFraction * hnt->avg[0];
        hnt->seen[0] = now[0]; hnt->seen[1] = now[1];
    }
    return hnt->split;
}
// behind a pass: the counters on their way to the host
void density_hint_refresh(void* stream) {
#ifndef KPN_SIMT_EMU
    if (density_first() != 2 || stream_is_capturing(stream)) return;
    DensityHint* hnt = density_hint();
    if (!hnt) return;
    if (!hnt->pinned) {
        void* hp = nullptr;
        if (hipHostMalloc(&hp, 2 * sizeof(unsigned long long), hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return; }
        hnt->pinned = static_cast<unsigned long long*>(hp);
        hnt->pinned[0] = hnt->pinned[1] = 0;
    }
    void* dp = nullptr;
    if (hipGetSymbolAddress(&dp, HIP_SYMBOL(kpn_density_counts)) != hipSuccess) { (void)hipGetLastError(); return; }
    (void)hipMemcpyAsync(hnt->pinned, dp, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, (hipStream_t)stream);
#else
    (void)stream;
#endif
}
int pair_grid_blocks() {   // k_geo_rows_h2: one 256-thread workgroup per CU = one wave per SIMD
#ifdef KPN_SIMT_EMU
    return 8;
#else
    static int blocks = [] {
        int dev = 0, cus = 0;   // one workgroup per compute unit of the current device (256 on an MI355X)
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
        return cus;
    }();
    return blocks;
#endif
}
int fuse_grid_blocks() { return kEmu ? 4 : 256; }      // one 512-thread workgroup per CU
int records_grid_blocks() { return kEmu ? 8 : 2048; }  // k_row_records, k_row_records_live
// points per k_mask_compact thread: as many as keep >= 8 workgroups per CU in flight
static inline int mask_points_per_thread(int64_t N) {
    const int64_t min_groups = kEmu ? 2 : 2048;  // (2: so that the emulator tests walk the multi-point loop)
    int ppt = KPN_MASK_PPT;
    while (ppt > 1 && N / (256 * (int64_t)ppt) < min_groups) ppt >>= 1;
    return ppt;
}
// ---- the range guard of the two-fp16-piece kernels (kpn_field_shared.h kpn_batch) ----
// On (the default) whenever rows mode 3 or fuse mode 1 is selected: those kernels stand aside on the device when the weights or
// the maps are beyond fp16's range, the per-point kernel flags a batch with a non-finite result, and the fp32-range kernels (rows
// mode 2, or 0 if selected; fuse mode 0) launched behind them evaluate such a batch again — two launches per batch that return
// at once otherwise.  KPN_NO_RANGE_GUARD=1 / kpn_set_range_guard(0): the round-3 behaviour (an operand beyond fp16's range makes
// the point NaN), for timing comparisons.
int range_guard() { return (int)g_range_guard.get([] { return (long long)!env_flag("KPN_NO_RANGE_GUARD"); }); }
// batches evaluated again by the fp32-range kernels since the library was loaded, per device: a device GLOBAL of this module (one
// instance per device, zero-initialised when the module is loaded) that the per-point kernel of such a launch increments and
// kpn_range_guard_count reads.  No allocation, no synchronisation on the render path (round 4 hipMalloc'ed the counter inside the
// first guarded render: an advisor finding — a first frame captured into a HIP graph would have been invalidated).
#ifndef KPN_SIMT_EMU
__device__ int kpn_redone_batches;
#else
static int kpn_redone_batches;
#endif
int* redone_counter() {
#ifndef KPN_SIMT_EMU
    void* p = nullptr;
    if (hipGetSymbolAddress(&p, HIP_SYMBOL(kpn_redone_batches)) != hipSuccess) return nullptr;
    return static_cast<int*>(p);
#else
    return &kpn_redone_batches;
#endif
}

// One field pass, as its callers name it.  out == nullptr: rows only (the backward runs its own per-point kernels).  lean: a render
// pass (no per-point `valid`, the zero-density short path); keep_rows: a backward call reads the valid list and the per-view rows again
// (ROWS layout, one batch); allow_pool: the POOL layout may be used; rows_sel / fuse_sel: KPN_ROWS_* / KPN_FUSE_* (0 = process-wide)
struct FieldPass {
    kpn_points points; int64_t N = 0; int mode = 0;   // 0 = raw query, 1 = eval_func
    float* out = nullptr; uint8_t* valid = nullptr; void* ws = nullptr;   // (N, 5), (N), query_layout(N, V, ...)
    bool lean = false, keep_rows = false, allow_pool = false; int rows_sel = 0, fuse_sel = 0;
};
// what every launch of a pass shares
struct FieldLaunch { const kpn_scene_dev& sc; const kpn_points& ps; const float* wp; int *list, *count, *live; float* xscr; void* stream; };
kpn_batch make_batch(int index, int tiles_cap, bool pool, int cond = KPN_RUN_ALWAYS, int* bad = nullptr, int* redone = nullptr) {
    return kpn_batch{index, tiles_cap, cond, bad, redone, pool ? 1 : 0, nullptr};
}

void launch_rows(const FieldLaunch& f, int rows_mode, int* tickets, const kpn_batch& batch) {
    if (rows_mode >= 2)
        kpn_internal_launch_geo_rows_pair(rows_mode, pair_grid_blocks(), f.stream, &f.sc, &f.ps, f.wp, f.list, f.count, tickets, f.xscr, &batch);
    else
        KPN_LAUNCH(k_geo_rows, dim3(field_grid_blocks()), dim3(256), f.stream, f.sc, f.ps, f.wp, (const int*)f.list, (const int*)f.count, tickets, f.xscr, batch);
}
void launch_records(const FieldLaunch& f, const kpn_batch& batch) {
    kpn_internal_launch_row_records(records_grid_blocks(), f.stream, &f.sc, &f.ps, f.wp, f.list, f.count, f.xscr, &batch);
}
// the shipped view count, no view dropped: the unrolled V = 3 variants of the two-fp16-piece per-point kernels
bool use_h3(const kpn_scene_dev& sc) { return sc.V == 3 && (sc.keep & 7u) == 7u && !env_flag("KPN_NO_FUSE_H3"); }
void launch_fuse(const FieldLaunch& f, int fmode, int* tickets, int mode, float* out, const kpn_batch& batch, int zero_skip) {
    // one 512-thread workgroup per CU (two wavefronts per SIMD): its 137 / 141 KB of weights sit in LDS
    auto* kernel = fmode != 1 ? k_fuse_color : (use_h3(f.sc) ? k_fuse_color_h3 : k_fuse_color_h);
    KPN_LAUNCH(kernel, dim3(fuse_grid_blocks()), dim3(512), f.stream, f.sc, f.ps, f.wp, (const int*)f.list, (const int*)f.count, tickets, (const float*)f.xscr, mode, 0, out, batch, zero_skip);
}
// the density-first pair of a render pass's batch: pass A, the gather records of the live points, pass B
void launch_density_first(const FieldLaunch& f, int* tickets, float* out, const kpn_batch& batch) {
    const int fblocks = fuse_grid_blocks();
    KPN_LAUNCH(k_density_h, dim3(fblocks), dim3(512), f.stream, f.sc, f.ps, f.wp, (const int*)f.list, (const int*)f.count, tickets, f.xscr, f.live, out, batch);
    kpn_internal_launch_row_records_live(records_grid_blocks(), f.stream, &f.sc, &f.ps, f.wp, f.list, f.count, tickets, f.live, f.xscr, &batch);
    auto* colour = use_h3(f.sc) ? k_colour_h3 : k_colour_h;
    KPN_LAUNCH(colour, dim3(fblocks), dim3(512), f.stream, f.sc, f.ps, f.wp, (const int*)f.list, (const int*)f.count, tickets, (const float*)f.xscr, f.live, out, batch);
}

int selected_rows_mode(int sel) { return sel == KPN_ROWS_F32 ? 0 : (sel == KPN_ROWS_BF16X3 ? 2 : (sel == KPN_ROWS_F16X2 ? 3 : geo_rows_mode())); }
int selected_fuse_mode(int sel) { return sel == KPN_FUSE_F32 ? 0 : (sel == KPN_FUSE_F16X2 ? 1 : fuse_mode()); }

int run_field(const kpn_scene_dev& sc, const float* wp, const FieldPass& p, void* stream) {
    const kpn_points& ps = p.points;
    const int rmode = selected_rows_mode(p.rows_sel);
    const int fmode = !p.out ? 0 : selected_fuse_mode(p.fuse_sel);
    // POOL layout of the scratch (kpn_field_shared.h): the pair-tile rows kernels pool over the views themselves — the eval render
    // passes and kpn_query; never when a backward pass reads the per-view rows again, never in the train branch (whose kept and
    // not-kept forward must stay bit-identical)
    // (the workspace is laid out for the process-wide selection: a per-call rows kernel without the POOL layout uses the ROWS one)
    const bool pool = p.allow_pool && !p.keep_rows && p.out && pool_layout_selected() && rmode >= 2;
    const QueryLayout L = query_layout(p.N, sc.V, pool);
    char* base = static_cast<char*>(p.ws);
    int* count = reinterpret_cast<int*>(base + L.count);
    const FieldLaunch f{sc, ps, wp, reinterpret_cast<int*>(base + L.list), count, reinterpret_cast<int*>(base + L.live),
                        reinterpret_cast<float*>(base + L.xscr), stream};
    hipMemsetAsync(count, 0, kCounterBytes, (hipStream_t)stream);
    const int ppt = mask_points_per_thread(p.N);
    KPN_LAUNCH(k_mask_compact, grid1d(p.N, 256 * ppt), dim3(256), stream, sc, ps, p.N, p.mode, (int)p.lean, ppt, wp + kpn_scalar_off(), p.out, p.valid, f.list, count);
    if (p.keep_rows && L.nbatch > 1) return fail(KPN_EWORKSPACE, "a pass whose rows a backward call reads again must fit the row scratch");
    // which launches stand under the range guard: the two-fp16-piece ones; behind them the fp32-range pair
    const bool guard = range_guard() && p.out && (rmode == 3 || fmode == 1);
    int* redone = guard ? redone_counter() : nullptr;
    const int safe_rmode = rmode == 3 ? 2 : rmode;
    auto guarded = [&](bool f16) { return guard && f16 ? KPN_RUN_IF_SAFE : KPN_RUN_ALWAYS; };
    // zero-density short path: render passes only (lean), never when a backward pass reads the rows again
    const int zero_skip = (p.lean && !p.keep_rows && !env_flag("KPN_NO_ZERO_SKIP")) ? 1 : 0;
    // density first: where the exact short path applies (render passes: eval_func, no density noise), on the POOL layout with the
    // two-fp16-piece per-point arithmetic — the shipped configuration
    const bool eligible = zero_skip && p.mode == 1 && ps.noise == nullptr && pool && fmode == 1;
    const bool split = eligible && density_first_now();
    if (eligible) ++g_density_first_passes[split ? 0 : 1];
    for (int b = 0; b < L.nbatch; ++b) {
        int* slots = count + 8 + 8 * b;   // the batch's tickets and flag (query_layout)
        int* bad = guard ? slots + 6 : nullptr;
        kpn_batch b_rows = make_batch(b, L.tiles_cap, pool, guarded(rmode == 3), bad);
        {
            KPN_FPROF(b_rows, rmode >= 2, count, sc.V);
            launch_rows(f, rmode, slots + 0, b_rows);
        }
        // the colour head's gather records (the pair-tile rows kernels leave them to k_row_records; a density-first pass forms
        // them for its live points only)
        if (rmode >= 2 && !split) launch_records(f, make_batch(b, L.tiles_cap, pool));
        if (!p.out) continue;   // rows only
        const kpn_batch b_fuse = make_batch(b, L.tiles_cap, pool, guarded(fmode == 1), bad);
        if (split) launch_density_first(f, slots, p.out, b_fuse);
        else launch_fuse(f, fmode, slots, p.mode, p.out, b_fuse, zero_skip);
        if (guard) {
            // The same batch again in fp32's exponent range, IF the kernels above stood aside or flagged it: the rows first (the
            // non-finite value may have come from either kernel; the gather records are intact — after a density-first pass they
            // exist for its live points only, so every point's are formed here), then the fused per-point kernel.
            const kpn_batch r_rows = make_batch(b, L.tiles_cap, pool, KPN_RUN_IF_UNSAFE, bad);
            launch_rows(f, safe_rmode, slots + 4, r_rows);
            if (split) launch_records(f, r_rows);
            launch_fuse(f, 0, slots + 4, p.mode, p.out, make_batch(b, L.tiles_cap, pool, KPN_RUN_IF_UNSAFE, bad, redone), zero_skip);
        }
    }
    if (eligible) density_hint_refresh(stream);
    return check_launch("field query");
}
}  // namespace

extern "C" int kpn_set_geo_rows_mode(int32_t mode) {
    KPN_REQUIRE(mode == 0 || mode == 2 || mode == 3, "mode must be 0 (fp32 MFMA), 2 (three bf16 pieces) or 3 (two fp16 pieces); mode 1 is not part of the library");
    g_geo_rows_mode.value = mode;
    return KPN_OK;
}
extern "C" int kpn_get_geo_rows_mode(void) { return geo_rows_mode(); }
extern "C" int kpn_set_fuse_mode(int32_t mode) {
    KPN_REQUIRE(mode == 0 || mode == 1, "mode must be 0 (fp32 MFMA) or 1 (two fp16 pieces per operand)");
    g_fuse_mode.value = mode;
    return KPN_OK;
}
extern "C" int kpn_get_fuse_mode(void) { return fuse_mode(); }
// points whose density the render passes' per-point kernels looked at since the last reset, and how many of them were live
extern "C" int kpn_density_stats(void* stream, int64_t* listed_host, int64_t* live_host, int32_t reset) {
    KPN_REQUIRE(listed_host && live_host, "null pointer");
    unsigned long long v[2] = {0, 0};
#ifndef KPN_SIMT_EMU
    void* p = nullptr;
    if (hipGetSymbolAddress(&p, HIP_SYMBOL(kpn_density_counts)) != hipSuccess) return fail(KPN_ELAUNCH, "no density counters in this module");
    if (hipMemcpyAsync(v, p, sizeof(v), hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess ||
        (reset && hipMemsetAsync(p, 0, sizeof(v), (hipStream_t)stream) != hipSuccess) ||
        hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return fail(KPN_ELAUNCH, "could not read the density counters");
#else
    (void)stream;
    v[0] = kpn_density_counts[0]; v[1] = kpn_density_counts[1];
    if (reset) kpn_density_counts[0] = kpn_density_counts[1] = 0;
#endif
    *listed_host = (int64_t)v[0];
    *live_host = (int64_t)v[1];
    return KPN_OK;
}
#if defined(KPN_PRECISION_PROBE) && !defined(KPN_SIMT_EMU)
// probe builds only (scripts/precision_budget.py): which lo pieces the two-fp16-piece kernels replace by zero (kpn_common.h)
extern "C" int kpn_internal_probe_set_mask_pair(unsigned long long m);
extern "C" int kpn_probe_set_mask(unsigned long long m) {
    if (hipMemcpyToSymbol(HIP_SYMBOL(kpn_probe_mask_dev), &m, sizeof(m)) != hipSuccess) return fail(KPN_ELAUNCH, "probe mask");
    if (kpn_internal_probe_set_mask_pair(m)) return fail(KPN_ELAUNCH, "probe mask (pair unit)");
    return hipDeviceSynchronize() == hipSuccess ? KPN_OK : KPN_ELAUNCH;
}
#endif
extern "C" int kpn_density_first_passes(int64_t* density_first_host, int64_t* fused_host, int32_t reset) {
    KPN_REQUIRE(density_first_host && fused_host, "null pointer");
    *density_first_host = g_density_first_passes[0];
    *fused_host = g_density_first_passes[1];
    if (reset) g_density_first_passes[0] = g_density_first_passes[1] = 0;
    return KPN_OK;
}
extern "C" int kpn_set_density_first(int32_t mode) {
    KPN_REQUIRE(mode >= 0 && mode <= 2, "mode must be 0 (fused per-point kernel), 1 (density first) or 2 (auto)");
    g_density_first.value = mode;
    return KPN_OK;
}
extern "C" int kpn_get_density_first(void) { return density_first(); }
extern "C" int kpn_set_range_guard(int32_t on) { g_range_guard.value = on ? 1 : 0; return KPN_OK; }
extern "C" int kpn_get_range_guard(void) { return range_guard(); }
// Batches of (point, view) rows that the fp32-range kernels evaluated again on the current device since the library was loaded
// (0 = every pass ran on the two-fp16-piece kernels).  Synchronises `stream`.
extern "C" int kpn_range_guard_count(void* stream, int64_t* batches_host) {
    KPN_REQUIRE(batches_host != nullptr, "null pointer");
    *batches_host = 0;
    int* c = redone_counter();
    if (!c) return fail(KPN_ELAUNCH, "could not allocate the range guard's counter");
    int v = 0;
#ifndef KPN_SIMT_EMU
    if (hipMemcpyAsync(&v, c, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess ||
        hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return fail(KPN_ELAUNCH, "could not read the range guard's counter");
#else
    (void)stream; v = *c;
#endif
    *batches_host = v;
    return KPN_OK;
}

extern "C" size_t kpn_query_workspace_bytes(int64_t N, int32_t V) {
    if (N <= 0 || V <= 0) return 0;
    const size_t qa = query_layout(N, V, false).total, qb = query_layout(N, V, pool_layout_selected()).total;
    return qa > qb ? qa : qb;
}

extern "C" int kpn_query(const kpn_scene_desc* d, const void* scene_ws, const float* wp, int64_t N, const float* pts,
                         const float* view, int32_t mode, float* out, uint8_t* valid, void* ws, size_t ws_bytes,
                         void* stream) {
    if (int e = check_desc(d)) return e;
    KPN_REQUIRE(mode == 0 || mode == 1, "mode must be 0 (raw query) or 1 (eval_func)");
    KPN_REQUIRE(N >= 0 && N < (1ll << 31), "point count out of range");
    if (N == 0) return KPN_OK;  // empty input: nothing to do (pointers may be null)
    KPN_REQUIRE(scene_ws && wp && pts && view && out && ws, "null pointer");
    if (ws_bytes < query_layout(N, d->n_views, pool_layout_selected()).total) return fail(KPN_EWORKSPACE, "query workspace too small");
    FieldPass p;
    p.points = kpn_points{pts, view, nullptr, nullptr, nullptr, 1};
    p.N = N; p.mode = mode; p.out = out; p.valid = valid; p.ws = ws; p.allow_pool = true;
    return run_field(scene_dev(d, scene_ws), wp, p, stream);
}
extern "C" size_t kpn_row_scratch_cap_bytes(void) { return row_scratch_cap_bytes(); }
extern "C" int kpn_set_row_scratch_cap_bytes(size_t bytes) {
    KPN_REQUIRE(bytes >= ((size_t)1 << 20), "the row scratch cap must be at least 1 MiB");
    g_row_scratch_cap.value = (long long)bytes;   // workspaces sized before the change must be re-queried (kpn_*_workspace_bytes)
    return KPN_OK;
}

// ---------------------------------------------------------------------------------------------
// measurement hooks: HIP events around the rows launches of the field passes (kpn_profile_enable / _collect) and around the kernel
// groups of the backward (kpn_bwd_profile_enable / _collect).  The device build only; the emulator build keeps the entry points.
namespace {
#ifndef KPN_SIMT_EMU
struct ProfState {
    bool on = false;
    std::vector<hipEvent_t> ev;   // pairs
    int* counts_host = nullptr;   // pinned: the pass's valid count, one copy per recorded launch
    unsigned long long* clk_dev = nullptr;    // two shader-clock stamps per recorded launch (kpn_batch::clk), and their pinned copy
    unsigned long long* clk_host = nullptr;
    std::vector<kpn_batch> batch; // which batch of the pass the launch was
    size_t used = 0, cap = 0;
    int V = 0;
};
static ProfState g_prof;
struct FieldProfScope {                // brackets the rows launch of one batch (run_field)
    bool rec;
    const kpn_batch& batch; const int* count; int V; void* stream;
    FieldProfScope(kpn_batch& b_rows, bool stamp, const int* count_, int V_, void* st)
        : rec(g_prof.on && g_prof.used < g_prof.cap), batch(b_rows), count(count_), V(V_), stream(st) {
        if (!rec) return;
        if (stamp) b_rows.clk = g_prof.clk_dev + 2 * g_prof.used;
        (void)hipEventRecord(g_prof.ev[2 * g_prof.used], (hipStream_t)stream);
    }
    ~FieldProfScope() {
        if (!rec) return;
        (void)hipEventRecord(g_prof.ev[2 * g_prof.used + 1], (hipStream_t)stream);
        (void)hipMemcpyAsync(g_prof.counts_host + g_prof.used, count, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream);
        g_prof.batch[g_prof.used] = batch;
        g_prof.V = V;
        ++g_prof.used;
    }
};
// stamp: the kernel writes shader-clock stamps (the pair-tile rows kernels)
#define KPN_FPROF(b_rows, stamp, count, V) FieldProfScope fprof_scope_(b_rows, stamp, count, V, stream)
#else
#define KPN_FPROF(b_rows, stamp, count, V) ((void)0)
#endif
// ---- measurement hooks of the backward (kpn_bwd_profile_enable / _collect): HIP events around each kernel group of a pass ----
enum { BP_ROWS_FWD = 0, BP_COLOR_BWD, BP_FUSE_BWD, BP_ROWS_BWD, BP_WGRAD, BP_KINDS };
#ifndef KPN_SIMT_EMU
struct BwdProf {
    bool on = false;
    std::vector<hipEvent_t> ev;        // pairs
    std::vector<int> kind;
    int* counts_host = nullptr;        // pinned: per recorded PASS the valid count and the view count / keep mask
    size_t used = 0, cap = 0, passes = 0;
};
static BwdProf g_bprof;
struct BwdProfScope {                  // brackets the launches made while it lives
    int slot = -1;
    void* stream;
    BwdProfScope(int kind, void* st) : stream(st) {
        if (!g_bprof.on || g_bprof.used >= g_bprof.cap) return;
        slot = (int)g_bprof.used++;
        g_bprof.kind[slot] = kind;
        (void)hipEventRecord(g_bprof.ev[2 * slot], (hipStream_t)stream);
    }
    ~BwdProfScope() { if (slot >= 0) (void)hipEventRecord(g_bprof.ev[2 * slot + 1], (hipStream_t)stream); }
};
#define KPN_BPROF(kind) BwdProfScope bprof_scope_(kind, stream)
#else
#define KPN_BPROF(kind) ((void)0)
#endif
// a pass's valid count, view count and keep mask, for the FLOP models of kpn_bwd_profile_collect
void bwd_prof_pass(const int* vcount, int V, uint32_t keep_mask, void* stream) {
#ifndef KPN_SIMT_EMU
    if (!g_bprof.on || g_bprof.passes >= g_bprof.cap) return;
    (void)hipMemcpyAsync(g_bprof.counts_host + 3 * g_bprof.passes, vcount, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream);
    g_bprof.counts_host[3 * g_bprof.passes + 1] = V;
    g_bprof.counts_host[3 * g_bprof.passes + 2] = (int)(keep_mask & ((V >= 31) ? 0x7FFFFFFFu : ((1u << V) - 1u)));
    ++g_bprof.passes;
#else
    (void)vcount; (void)V; (void)keep_mask; (void)stream;
#endif
}
}  // namespace

extern "C" int kpn_bwd_profile_enable(int32_t on) {
#ifndef KPN_SIMT_EMU
    if (on && g_bprof.cap == 0) {
        g_bprof.cap = 4096;
        g_bprof.ev.resize(2 * g_bprof.cap);
        g_bprof.kind.resize(g_bprof.cap);
        for (auto& e : g_bprof.ev) if (hipEventCreate(&e) != hipSuccess) return fail(KPN_ELAUNCH, "hipEventCreate failed");
        if (hipHostMalloc((void**)&g_bprof.counts_host, g_bprof.cap * 3 * sizeof(int), 0) != hipSuccess) return fail(KPN_ELAUNCH, "hipHostMalloc failed");
    }
    g_bprof.on = on != 0;
    g_bprof.used = 0;
    g_bprof.passes = 0;
#endif
    return KPN_OK;
}
extern "C" int kpn_bwd_profile_collect(double* ms5, int64_t* launches5, int64_t* rows_host, int64_t* kept_rows_host, int64_t* points_host) {
    KPN_REQUIRE(ms5 && launches5 && rows_host && kept_rows_host && points_host, "null pointer");
    for (int i = 0; i < BP_KINDS; ++i) { ms5[i] = 0.0; launches5[i] = 0; }
    *rows_host = *kept_rows_host = *points_host = 0;
#ifndef KPN_SIMT_EMU
    for (size_t i = 0; i < g_bprof.used; ++i) {
        if (hipEventSynchronize(g_bprof.ev[2 * i + 1]) != hipSuccess) return fail(KPN_ELAUNCH, "hipEventSynchronize failed");
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, g_bprof.ev[2 * i], g_bprof.ev[2 * i + 1]) != hipSuccess) return fail(KPN_ELAUNCH, "hipEventElapsedTime failed");
        ms5[g_bprof.kind[i]] += ms;
        ++launches5[g_bprof.kind[i]];
    }
    if (hipDeviceSynchronize() != hipSuccess) return fail(KPN_ELAUNCH, "hipDeviceSynchronize failed");
    for (size_t p_ = 0; p_ < g_bprof.passes; ++p_) {
        const int64_t cnt = g_bprof.counts_host[3 * p_], V = g_bprof.counts_host[3 * p_ + 1];
        *points_host += cnt;
        *rows_host += cnt * V;
        *kept_rows_host += cnt * __builtin_popcount((unsigned)g_bprof.counts_host[3 * p_ + 2]);
    }
    g_bprof.used = 0;
    g_bprof.passes = 0;
#endif
    return KPN_OK;
}
extern "C" int kpn_profile_enable(int32_t on) {
#ifndef KPN_SIMT_EMU
    if (on && g_prof.cap == 0) {
        g_prof.cap = 8192;
        g_prof.ev.resize(2 * g_prof.cap);
        g_prof.batch.resize(g_prof.cap);
        for (auto& e : g_prof.ev) if (hipEventCreate(&e) != hipSuccess) return fail(KPN_ELAUNCH, "hipEventCreate failed");
        if (hipHostMalloc((void**)&g_prof.counts_host, g_prof.cap * sizeof(int), 0) != hipSuccess)
            return fail(KPN_ELAUNCH, "hipHostMalloc failed");
        if (hipMalloc((void**)&g_prof.clk_dev, g_prof.cap * 2 * sizeof(unsigned long long)) != hipSuccess ||
            hipHostMalloc((void**)&g_prof.clk_host, g_prof.cap * 2 * sizeof(unsigned long long), 0) != hipSuccess)
            return fail(KPN_ELAUNCH, "hipMalloc failed");
    }
    if (on && hipMemset(g_prof.clk_dev, 0, g_prof.cap * 2 * sizeof(unsigned long long)) != hipSuccess) return fail(KPN_ELAUNCH, "hipMemset failed");
    g_prof.on = on != 0;
    g_prof.used = 0;
#endif
    return KPN_OK;
}
extern "C" int kpn_profile_collect3(double* ms_out, int64_t* launches_out, int64_t* rows_out, int64_t* surplus_out, double* clock_ghz_out) {
    KPN_REQUIRE(ms_out && launches_out && rows_out && surplus_out, "null pointer");
    *ms_out = 0.0; *launches_out = 0; *rows_out = 0; *surplus_out = 0;
    if (clock_ghz_out) *clock_ghz_out = 0.0;
#ifndef KPN_SIMT_EMU
    double cyc = 0.0, cyc_ms = 0.0;
    if (g_prof.used && g_prof.clk_dev) {
        if (hipEventSynchronize(g_prof.ev[2 * (g_prof.used - 1) + 1]) != hipSuccess ||
            hipMemcpy(g_prof.clk_host, g_prof.clk_dev, g_prof.used * 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess)
            return fail(KPN_ELAUNCH, "could not read the clock stamps");
    }
    for (size_t i = 0; i < g_prof.used; ++i) {
        if (hipEventSynchronize(g_prof.ev[2 * i + 1]) != hipSuccess) return fail(KPN_ELAUNCH, "hipEventSynchronize failed");
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, g_prof.ev[2 * i], g_prof.ev[2 * i + 1]) != hipSuccess) return fail(KPN_ELAUNCH, "hipEventElapsedTime failed");
        // rows of this launch: the same arithmetic as kpn_batch_range (field_kernels.hip) on the pass's valid count
        const int64_t count = g_prof.counts_host[i];
        const kpn_batch b = g_prof.batch[i];
        const int64_t ntiles = (count + KPN_TILE - 1) / KPN_TILE;
        const int64_t nb = (ntiles + b.tiles_cap - 1) / b.tiles_cap;
        if (b.index >= nb) { ++*surplus_out; continue; }     // surplus batch: returned at once, nothing processed
        const int64_t p0 = ntiles * b.index / nb * KPN_TILE, p1 = ntiles * (b.index + 1) / nb * KPN_TILE;
        *rows_out += ((p1 < count ? p1 : count) - p0) * g_prof.V;
        *ms_out += ms;
        ++*launches_out;
        if (g_prof.clk_host && g_prof.clk_host[2 * i + 1] > g_prof.clk_host[2 * i]) {   // pair-tile kernels only
            cyc += (double)(g_prof.clk_host[2 * i + 1] - g_prof.clk_host[2 * i]);
            cyc_ms += ms;
        }
    }
    // shader cycles the first workgroup spent in the launches / the launches' event time: a lower bound of the sustained clock
    // (the workgroup ends a little before its launch does)
    if (clock_ghz_out && cyc_ms > 0.0) *clock_ghz_out = cyc / (cyc_ms * 1e6);
    g_prof.used = 0;
#endif
    return KPN_OK;
}
extern "C" int kpn_profile_collect2(double* ms_out, int64_t* launches_out, int64_t* rows_out, int64_t* surplus_out) {
    return kpn_profile_collect3(ms_out, launches_out, rows_out, surplus_out, nullptr);
}
extern "C" int kpn_profile_collect(double* ms_out, int64_t* launches_out, int64_t* rows_out) {
    int64_t surplus = 0;
    return kpn_profile_collect2(ms_out, launches_out, rows_out, &surplus);
}

#ifdef KPN_BWD_TIMING
extern "C" int kpn_bwd_timing(unsigned long long* out16) {   // read and clear (debug builds only; not part of the ABI)
    if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(kpn_bwd_cycles), 128) != hipSuccess) return 1;
    const unsigned long long z[16] = {0};
    return hipMemcpyToSymbol(HIP_SYMBOL(kpn_bwd_cycles), z, 128) != hipSuccess;
}
#endif
#if defined(KPN_FUSE_TIMING) && !defined(KPN_SIMT_EMU)
// debug builds only: read (and clear) the per-phase cycle sums of k_fuse_color
extern "C" int kpn_fuse_timing(unsigned long long* out8) {
    if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(kpn_fuse_cycles), 64) != hipSuccess) return 1;
    unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    return hipMemcpyToSymbol(HIP_SYMBOL(kpn_fuse_cycles), z, 64) != hipSuccess;
}
#endif

// api_common.h - what every host part of the C ABI uses: the error plumbing, launch grids and the workspace carver.
#pragma once
static thread_local std::string g_err;
static int fail(int code, const std::string& msg) { g_err = msg; return code; }
#define KPN_REQUIRE(cond, msg) do { if (!(cond)) return fail(KPN_EINVAL, std::string(msg) + " [" #cond "]"); } while (0)
static int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(KPN_ELAUNCH, std::string(what) + ": " + hipGetErrorString(e));
    return KPN_OK;
}
static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
static inline dim3 grid1d(int64_t n, int block) { return dim3((unsigned)((n + block - 1) / block)); }
// (diagnostics, kpn_selftest_mfma: every runtime call checked)
#define KPN_HIP_TRY(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return fail(KPN_ELAUNCH, std::string(#call) + ": " + hipGetErrorString(e_)); } while (0)
// carves a workspace: take() returns the offset of the next block and moves on by its aligned size (units are the caller's)
struct Carver {
    size_t o = 0;
    size_t take(size_t n, size_t align = 256) { const size_t r = o; o += align_up(n, align); return r; }
};
// The grid and the scratch of the deterministic fp64 reductions (kpn_reduce.h; kpn_mse_psnr, kpn_pix_l1_loss, kpn_ssim and, for the
// grid, kpn_train_loss): at most 2048 blocks of 256 threads, and 16,392 bytes holding the blocks' partials and then the ticket.
static inline int64_t reduce_blocks(int64_t n) { return std::min<int64_t>((n + 255) / 256, 2048); }
struct ReduceScratch { double* partial; int* ticket; };
static inline ReduceScratch reduce_scratch(void* scratch) {
    double* partial = static_cast<double*>(scratch);
    return {partial, reinterpret_cast<int*>(partial + 2048)};
}
namespace {
bool stream_is_capturing(void* stream) {
#ifndef KPN_SIMT_EMU
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing((hipStream_t)stream, &st) != hipSuccess) { (void)hipGetLastError(); return false; }
    return st != hipStreamCaptureStatusNone;
#else
    (void)stream; return false;
#endif
}
}  // namespace

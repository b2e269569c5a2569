// ---------------------------------------------------------------------------------------------
// image metrics, the MFMA self test and the FLOP models
extern "C" int kpn_frame_to_rgb8(const float* chw, int32_t H, int32_t W, int32_t bgr, uint8_t* hwc_out, void* stream) {
    KPN_REQUIRE(chw && hwc_out, "null pointer");
    KPN_REQUIRE(H > 0 && W > 0 && (int64_t)H * W < (1ll << 31), "bad frame size");
    KPN_LAUNCH(k_frame_to_rgb8, grid1d((int64_t)H * W, 256), dim3(256), stream, (int)(H * W), (int)bgr, chw, hwc_out);
    return check_launch("kpn_frame_to_rgb8");
}
extern "C" int kpn_mse_psnr(const float* pred, const float* gt, int64_t n, double* out2, void* scratch, void* stream) {
    KPN_REQUIRE(pred && gt && out2 && scratch, "null pointer");
    KPN_REQUIRE(n > 0, "empty image");
    const ReduceScratch r = reduce_scratch(scratch);
    (void)hipMemsetAsync(r.ticket, 0, sizeof(int), (hipStream_t)stream);
    KPN_LAUNCH(k_mse_psnr, dim3((unsigned)reduce_blocks(n)), dim3(256), stream, n, pred, gt, r.partial, r.ticket, out2);
    return check_launch("kpn_mse_psnr");
}

extern "C" int kpn_pix_l1_loss(const float* src, const float* tar, int64_t n, float lambda, float* loss, float* d_src, void* scratch,
                               void* stream) {
    KPN_REQUIRE(src && tar && loss && scratch, "null pointer");
    KPN_REQUIRE(n > 0, "empty image");
    const ReduceScratch r = reduce_scratch(scratch);
    (void)hipMemsetAsync(r.ticket, 0, sizeof(int), (hipStream_t)stream);
    KPN_LAUNCH(k_pix_l1, dim3((unsigned)reduce_blocks(n)), dim3(256), stream, n, lambda, src, tar, r.partial, r.ticket, loss, d_src);
    return check_launch("kpn_pix_l1_loss");
}

// compute_error_nerf's pixel and mask terms (reference src/utils.py:108-171, pix_loss :173-183) in one launch: k_train_loss
// (loss_kernels.hip).  The grid rule is kpn_pix_l1_loss's, over the 3n pixel elements, so that the L1 terms add up in the same order.
static int64_t train_loss_blocks(int64_t n) { return reduce_blocks(3 * n); }
extern "C" size_t kpn_train_loss_workspace_bytes(int64_t n) {
    if (n <= 0 || n > (int64_t)1 << 40) return 0;
    return 256 + align_up((size_t)train_loss_blocks(n) * 6 * sizeof(double), 256);
}
extern "C" int kpn_train_loss(const kpn_train_loss_args* args, void* workspace, void* stream) {
    KPN_REQUIRE(args && workspace && args->terms, "null pointer");
    KPN_REQUIRE(args->n > 0 && args->n <= (int64_t)1 << 40, "bad pixel count");
    KPN_REQUIRE(args->tar || (!args->tex && !args->tex_fine), "tex / tex_fine need tar");
    kpn_loss_kargs k;
    k.a = *args;
    const int64_t blocks = train_loss_blocks(args->n);
    k.ticket = static_cast<int*>(workspace);                          // first, so that a workspace serves any smaller n as well
    k.partial = reinterpret_cast<double*>(static_cast<char*>(workspace) + 256);
    if (args->reset_ticket) (void)hipMemsetAsync(k.ticket, 0, sizeof(int), (hipStream_t)stream);
    KPN_LAUNCH(k_train_loss, dim3((unsigned)blocks), dim3(256), stream, k);
    return check_launch("kpn_train_loss");
}

extern "C" size_t kpn_ssim_scratch_bytes(int32_t w, int32_t h) {
    if (w < 7 || h < 7) return 0;
    return align_up((size_t)5 * 3 * (h - 6) * w * sizeof(float), 256) + 2048 * sizeof(double) + 256;
}
extern "C" int kpn_ssim(const float* pred_chw, const float* gt_chw, int32_t H, int32_t W, int32_t x0, int32_t y0, int32_t w,
                        int32_t h, double* out, void* scratch, void* stream) {
    KPN_REQUIRE(pred_chw && gt_chw && out && scratch, "null pointer");
    KPN_REQUIRE(x0 >= 0 && y0 >= 0 && w >= 7 && h >= 7 && x0 + w <= W && y0 + h <= H, "crop must lie inside the image and be at least 7x7 (win_size)");
    char* base = static_cast<char*>(scratch);
    float* tmp = reinterpret_cast<float*>(base);
    const ReduceScratch r = reduce_scratch(base + align_up((size_t)5 * 3 * (h - 6) * w * sizeof(float), 256));
    (void)hipMemsetAsync(r.ticket, 0, sizeof(int), (hipStream_t)stream);
    KPN_LAUNCH(k_ssim_vertical, grid1d((int64_t)3 * (h - 6) * w, 256), dim3(256), stream, pred_chw, gt_chw, (int)H, (int)W, (int)x0, (int)y0,
               (int)w, (int)h, tmp);
    KPN_LAUNCH(k_ssim_map, dim3((unsigned)reduce_blocks((int64_t)3 * (h - 6) * (w - 6))), dim3(256), stream, (const float*)tmp, (int)w, (int)h,
               r.partial, r.ticket, out);
    return check_launch("kpn_ssim");
}
extern "C" double kpn_flops_per_row(void) { return 2.0 * 70080.0; }

extern "C" double kpn_flops_per_point(int32_t V) {
    // algorithmic MACs: per (point,view) 70,080 (layers1) + 13,256 (IBR head);
    // per point 12,416 (layers2) + 3,072 (compress)
    return 2.0 * ((70080.0 + 13256.0) * V + 12416.0 + 3072.0);
}

extern "C" int kpn_selftest_mfma(float* scratch, void* stream, float* max_err_host) {
    KPN_REQUIRE(scratch && max_err_host, "null pointer");
    float A[64], B[64], Dm[1024];
    for (int i = 0; i < 64; ++i) { A[i] = 0.37f * i - 7.0f + 0.011f * i * i; B[i] = 3.0f - 0.23f * i + (i % 5) * 0.7f; }
    // diagnostic: fully synchronous (pageable host buffers), every runtime call checked (KPN_HIP_TRY)
    for (int i = 0; i < 1024; ++i) Dm[i] = -12345.0f;
    KPN_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    KPN_HIP_TRY(hipMemcpy(scratch, A, sizeof(A), hipMemcpyHostToDevice));
    KPN_HIP_TRY(hipMemcpy(scratch + 64, B, sizeof(B), hipMemcpyHostToDevice));
    KPN_LAUNCH(k_selftest_mfma, dim3(1), dim3(64), stream, (const float*)scratch, (const float*)(scratch + 64), scratch + 128);
    if (int e = check_launch("k_selftest_mfma launch")) return e;
    KPN_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    KPN_HIP_TRY(hipMemcpy(Dm, scratch + 128, sizeof(Dm), hipMemcpyDeviceToHost));
    float me = 0.0f;
    for (int i = 0; i < 32; ++i)
        for (int j = 0; j < 32; ++j) {
            const float ref = fmaf(A[i * 2 + 1], B[32 + j], A[i * 2] * B[j]);
            me = fmaxf(me, fabsf(ref - Dm[i * 32 + j]));
        }
    *max_err_host = me;
    if (int e = check_launch("kpn_selftest_mfma")) return e;
    if (!(me < 1e-3f)) {
        char buf[256];
        snprintf(buf, sizeof(buf), "MFMA lane map mismatch: max err %g, D[0][0]=%g (ref %g), D[5][7]=%g (ref %g)", (double)me,
                 (double)Dm[0], (double)fmaf(A[1], B[32], A[0] * B[0]), (double)Dm[5 * 32 + 7],
                 (double)fmaf(A[11], B[39], A[10] * B[7]));
        return fail(KPN_ELAUNCH, buf);
    }
    return KPN_OK;
}

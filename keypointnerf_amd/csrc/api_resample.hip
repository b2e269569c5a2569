// ---------------------------------------------------------------------------------------------
// The two resampling steps between the ConvBlocks of an HourGlass, forward and backward: avg_pool2d(x, 2, stride = 2) and
// skip + interpolate(low, scale_factor = 2, mode = 'bicubic', align_corners = True) with their autograd (reference
// src/utils.py:287-306).  Kernels: encoder_kernels.hip.  The forwards are the encoder walk's own k_enc_pool2 / k_enc_upadd,
// launched through the launch layer at the head of api_encoders.hip (enc::launch_pool2 / enc::launch_upadd); the backwards are
// k_enc_pool2_bwd and k_enc_up2_bwd on its elementwise grid.  No workspace: every kernel reads its inputs and writes its one output.
namespace resample {
const char* desc_error(const kpn_resample2_desc* d) {
    if (!d) return "desc is null";
    if (d->N < 1 || d->h < 1 || d->w < 1) return "N, h, w must be positive";
    if (d->C < 4 || d->C % 4) return "C must be a positive multiple of 4";
    return nullptr;
}
inline int64_t low4(const kpn_resample2_desc* d) { return (int64_t)d->N * d->h * d->w * d->C / 4; }
}  // namespace resample

#define KPN_RESAMPLE_REQUIRE_DESC(desc) do { if (const char* e_ = resample::desc_error(desc)) return fail(KPN_EINVAL, std::string("kpn_resample2_desc: ") + e_); } while (0)

extern "C" int kpn_avg_pool2_forward(const kpn_resample2_desc* desc, const float* x_high, float* y_low, void* stream) {
    KPN_RESAMPLE_REQUIRE_DESC(desc);
    KPN_REQUIRE(x_high && y_low, "null pointer");
    KPN_REQUIRE((((uintptr_t)x_high | (uintptr_t)y_low) & 15) == 0, "x_high / y_low must be 16-byte aligned");
    enc::launch_pool2(x_high, y_low, desc->N, desc->h, desc->w, desc->C, stream);
    return check_launch("kpn_avg_pool2_forward");
}
extern "C" int kpn_avg_pool2_backward(const kpn_resample2_desc* desc, const float* dy_low, float* dx_high, void* stream) {
    KPN_RESAMPLE_REQUIRE_DESC(desc);
    KPN_REQUIRE(dy_low && dx_high, "null pointer");
    KPN_REQUIRE((((uintptr_t)dy_low | (uintptr_t)dx_high) & 15) == 0, "dy_low / dx_high must be 16-byte aligned");
    KPN_LAUNCH(k_enc_pool2_bwd, enc::grid4(4 * resample::low4(desc)), dim3(256), stream, dy_low, dx_high, (int)desc->N, (int)desc->h,
               (int)desc->w, (int)desc->C);
    return check_launch("kpn_avg_pool2_backward");
}
extern "C" int kpn_upsample2x_add_forward(const kpn_resample2_desc* desc, const float* low, const float* skip, float* y_high, void* stream) {
    KPN_RESAMPLE_REQUIRE_DESC(desc);
    KPN_REQUIRE(low && y_high, "null pointer");
    KPN_REQUIRE((((uintptr_t)low | (uintptr_t)skip | (uintptr_t)y_high) & 15) == 0, "low / skip / y_high must be 16-byte aligned");
    enc::launch_upadd(low, skip, y_high, desc->N, desc->h, desc->w, desc->C, stream);
    return check_launch("kpn_upsample2x_add_forward");
}
extern "C" int kpn_upsample2x_add_backward(const kpn_resample2_desc* desc, const float* dy_high, float* d_low, void* stream) {
    KPN_RESAMPLE_REQUIRE_DESC(desc);
    KPN_REQUIRE(dy_high && d_low, "null pointer");
    KPN_REQUIRE((((uintptr_t)dy_high | (uintptr_t)d_low) & 15) == 0, "dy_high / d_low must be 16-byte aligned");
    KPN_LAUNCH(k_enc_up2_bwd, enc::grid4(resample::low4(desc)), dim3(256), stream, dy_high, d_low, (int)desc->N, (int)desc->h, (int)desc->w,
               (int)desc->C);
    return check_launch("kpn_upsample2x_add_backward");
}

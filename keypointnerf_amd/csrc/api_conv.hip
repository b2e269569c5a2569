// ---------------------------------------------------------------------------------------------
// One stride-1 convolution, forward and its three gradients (torch.nn.functional.conv2d and its autograd, as the encoders use
// them: reference src/utils.py:416-474, 261-309, 322-414).  Kernels: encoder_kernels.hip.  The layer - its GEMMs over two packed copies
// of the weight, the weight gradient on the forward's tile, the bias gradient - and the six entry points are api_layer.hip's; this file
// says which descriptors it serves.  api_strided.hip serves the stride-2, stem and transposed layers in the same way.
struct conv_family {
    using Desc = kpn_conv2d_desc;
    static constexpr bool nchw_stem = false;
    // what the packed copies depend on
    static const char* weight_error(const Desc* d) {
        if (!d) return "desc is null";
        if (d->k != 1 && d->k != 3 && d->k != 5) return "k must be 1, 3 or 5 (square kernel, stride 1; the 7x7 stems and stride 2 are not served)";
        if (d->cin < 4 || d->cin % 4 || d->cin > 1024) return "cin must be a multiple of 4 in 4 .. 1024";
        if (d->cout < 4 || d->cout % 4 || d->cout > 1024) return "cout must be a multiple of 4 in 4 .. 1024";
        return nullptr;
    }
    static const char* desc_error(const Desc* d) {
        if (const char* e = weight_error(d)) return e;
        if (d->pad < 0 || d->pad > d->k - 1) return "pad must be in 0 .. k - 1";
        if (d->N < 1 || d->H < 1 || d->W < 1) return "N, H, W must be positive";
        if (d->H + 2 * d->pad - d->k + 1 < 1 || d->W + 2 * d->pad - d->k + 1 < 1) return "H, W: the output would be empty";
        if ((int64_t)d->N * (d->H + 2 * d->pad) * (d->W + 2 * d->pad) * std::max(d->cin, d->cout) >= (1ll << 31)) return "N * H * W * channels must stay below 2^31";
        if (d->has_bias != 0 && d->has_bias != 1) return "has_bias must be 0 or 1";
        return nullptr;
    }
    static enc::LayerSpec spec_of(const Desc* d) { return enc::LayerSpec{d->cin, d->cout, d->k, 1, d->pad, 0, 0, 0}; }
};
KPN_SINGLE_LAYER(conv_family, kpn_conv2d)

// The same six with the arithmetic of the GEMMs chosen by the caller (include/kpnerf.h): arith = KPN_CONV_F32 is the code above, bit for
// bit; KPN_CONV_BF16X3 runs encoder_split_kernels.hip, with its own tiles, packed size, split K and ranges.  An unknown arith is refused
// (the size queries return 0) before anything is launched.
#define KPN_CONV_EX_REQUIRE_ARITH(arith) do { if (const char* e_ = enc::arith_error(arith)) return fail(KPN_EINVAL, std::string("kpn_conv2d_ex: ") + e_); } while (0)
extern "C" size_t kpn_conv2d_ex_packed_floats(const kpn_conv2d_desc* desc, int32_t arith) {
    return enc::arith_error(arith) ? 0 : enc::single_packed_floats<conv_family>(desc, arith);
}
extern "C" int kpn_conv2d_ex_pack_device(const kpn_conv2d_desc* desc, int32_t arith, const float* w, float* packed, void* stream) {
    KPN_CONV_EX_REQUIRE_ARITH(arith);
    return enc::single_pack<conv_family>("kpn_conv2d", "kpn_conv2d_ex_pack_device", desc, w, packed, stream, arith);
}
extern "C" size_t kpn_conv2d_ex_workspace_bytes(const kpn_conv2d_desc* desc, int32_t arith) {
    return enc::arith_error(arith) ? 0 : enc::single_workspace_bytes<conv_family>(desc, arith);
}
extern "C" int32_t kpn_conv2d_ex_wgrad_ranges(const kpn_conv2d_desc* desc, int32_t arith) {
    return enc::arith_error(arith) ? 0 : enc::single_wgrad_ranges<conv_family>(desc, arith);
}
extern "C" int kpn_conv2d_ex_forward(const kpn_conv2d_desc* desc, int32_t arith, const float* x, const float* packed, const float* bias, float* y,
                                     void* workspace, size_t workspace_bytes, void* stream) {
    KPN_CONV_EX_REQUIRE_ARITH(arith);
    return enc::single_forward<conv_family>("kpn_conv2d", "kpn_conv2d_ex_forward", desc, x, packed, bias, y, workspace, workspace_bytes, stream, arith);
}
extern "C" int kpn_conv2d_ex_backward(const kpn_conv2d_desc* desc, int32_t arith, const float* x, const float* dy, const float* packed, float* dx,
                                      float* dw, float* db, void* workspace, size_t workspace_bytes, void* stream) {
    KPN_CONV_EX_REQUIRE_ARITH(arith);
    return enc::single_backward<conv_family>("kpn_conv2d", "kpn_conv2d_ex_backward", desc, x, dy, packed, dx, dw, db, workspace, workspace_bytes,
                                             stream, arith);
}

// ---------------------------------------------------------------------------------------------
// The three resolution-changing layers of the image encoders, forward and gradients: Conv2d(k 3, stride 2, pad 1), the stem
// Conv2d(k 7, stride 2, pad 3) on an NCHW tensor, and ConvTranspose2d(k 3, stride 2, pad 1, output_padding 1) (reference
// src/utils.py:199-247, 322-414).  Kernels: encoder_kernels.hip.  What each kind launches (the DECONV GEMM as the stride-2 layer's input
// gradient, the swapped roles of the transposed layer's weight gradient) and the six entry points are api_layer.hip's; this file says
// which descriptors it serves and which layer a kind is.
struct s2_family {
    using Desc = kpn_conv2d_s2_desc;
    static constexpr bool nchw_stem = true;
    static constexpr const char* stem_name = "KPN_S2_STEM7";
    static const char* weight_error(const Desc* d) {
        if (!d) return "desc is null";
        if (d->kind != KPN_S2_CONV3 && d->kind != KPN_S2_STEM7 && d->kind != KPN_S2_DECONV3)
            return "kind must be KPN_S2_CONV3, KPN_S2_STEM7 or KPN_S2_DECONV3";
        if (d->kind == KPN_S2_STEM7) {
            if (d->cin < 1 || d->cin > 4) return "cin must be in 1 .. 4 for KPN_S2_STEM7";
        } else if (d->cin < 4 || d->cin % 4 || d->cin > 1024) {
            return "cin must be a multiple of 4 in 4 .. 1024";
        }
        if (d->cout < 4 || d->cout % 4 || d->cout > 1024) return "cout must be a multiple of 4 in 4 .. 1024";
        return nullptr;
    }
    static const char* desc_error(const Desc* d) {
        if (const char* e = weight_error(d)) return e;
        if (d->N < 1 || d->H < 1 || d->W < 1) return "N, H, W must be positive";
        if (d->kind == KPN_S2_CONV3 && ((d->H | d->W) & 1)) return "H, W must be even for KPN_S2_CONV3 (the input gradient is a transposed convolution)";
        const int64_t big = d->kind == KPN_S2_DECONV3 ? 4 : 1;
        if ((int64_t)d->N * d->H * d->W * big * std::max(d->cin, d->cout) >= (1ll << 31)) return "N * H * W * channels must stay below 2^31 (for both x and y)";
        if (d->has_bias != 0 && d->has_bias != 1) return "has_bias must be 0 or 1";
        return nullptr;
    }
    static enc::LayerSpec spec_of(const Desc* d) {
        const int stem = d->kind == KPN_S2_STEM7;
        return enc::LayerSpec{d->cin, d->cout, stem ? 7 : 3, 2, stem ? 3 : 1, 0, d->kind == KPN_S2_DECONV3, stem};
    }
};
KPN_SINGLE_LAYER(s2_family, kpn_conv2d_s2)

// ---------------------------------------------------------------------------------------------
// The replication-padded stride-1 convolutions of the texture encoder, forward and gradients: ReplicationPad2d(k / 2) + Conv2d(k) for
// k = 3 (the two convolutions of a ResBlk), k = 7 (the output layer) and the 7x7 stem on an NCHW tensor (reference src/utils.py:199-259).
// Kernels: encoder_kernels.hip.  The pad is never materialised: the forward and the weight gradient read x through the clamped load, the
// input gradient is the adjoint of that load (a gather).  The layer and the six entry points are api_layer.hip's; this file says which
// descriptors it serves and which layer a kind is.
struct rp_family {
    using Desc = kpn_conv2d_rp_desc;
    static constexpr bool nchw_stem = true;
    static constexpr const char* stem_name = "KPN_RP_STEM7";
    static const char* weight_error(const Desc* d) {
        if (!d) return "desc is null";
        if (d->kind != KPN_RP_CONV3 && d->kind != KPN_RP_CONV7 && d->kind != KPN_RP_STEM7)
            return "kind must be KPN_RP_CONV3, KPN_RP_CONV7 or KPN_RP_STEM7";
        if (d->kind == KPN_RP_STEM7) {
            if (d->cin < 1 || d->cin > 4) return "cin must be in 1 .. 4 for KPN_RP_STEM7";
        } else if (d->cin < 4 || d->cin % 4 || d->cin > 1024) {
            return "cin must be a multiple of 4 in 4 .. 1024";
        }
        if (d->cout < 4 || d->cout % 4 || d->cout > 1024) return "cout must be a multiple of 4 in 4 .. 1024";
        return nullptr;
    }
    static const char* desc_error(const Desc* d) {
        if (const char* e = weight_error(d)) return e;
        if (d->N < 1 || d->H < 1 || d->W < 1) return "N, H, W must be positive";
        if ((int64_t)d->N * d->H * d->W * std::max(d->cin, d->cout) >= (1ll << 31)) return "N * H * W * channels must stay below 2^31 (for both x and y)";
        if (d->has_bias != 0 && d->has_bias != 1) return "has_bias must be 0 or 1";
        return nullptr;
    }
    static enc::LayerSpec spec_of(const Desc* d) {
        const int k = d->kind == KPN_RP_CONV3 ? 3 : 7;
        return enc::LayerSpec{d->cin, d->cout, k, 1, k / 2, 1, 0, d->kind == KPN_RP_STEM7};
    }
};
KPN_SINGLE_LAYER(rp_family, kpn_conv2d_rp)

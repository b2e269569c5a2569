// ---------------------------------------------------------------------------------------------
// The three resolution-changing layers of the image encoders, forward and gradients: Conv2d(k 3, stride 2, pad 1), the stem
// Conv2d(k 7, stride 2, pad 3) on an NCHW tensor, and ConvTranspose2d(k 3, stride 2, pad 1, output_padding 1) (reference
// src/utils.py:199-247, 322-414).  Kernels: encoder_kernels.hip; geometry, tiles, split K, the ranges of the weight gradient and every
// grid come from the launch layer at the head of api_encoders.hip, as for the stride-1 layer (api_conv.hip).  No GEMM of its own:
//   CONV3    y = k_enc_conv(stride 2)          dx = k_enc_conv<DECONV>(dy) over the deconv copy of the same OIHW weight (H, W even:
//            conv_transpose2d(dy, w, 2, 1, 1) is exactly the gradient)             dw = k_enc_wgrad, A from x with stride 2
//   STEM7    y = k_enc_conv<STEM>(stem_plain)  no dx                               dw = k_enc_wgrad<STEM>, K rows tap * 4 + ci
//   DECONV3  y = k_enc_conv<DECONV>            dx = k_enc_conv(stride 2)(dy) over the plain copy of the (cin, cout, 3, 3) weight read
//            as OIHW                                                               dw = k_enc_wgrad, A from dy with stride 2, R = x
namespace s2 {
const char* weight_error(const kpn_conv2d_s2_desc* d) {
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
// (Ho, Wo) of y for an (H, W) input
inline void out_hw(int kind, int H, int W, int& Ho, int& Wo) {
    if (kind == KPN_S2_DECONV3) { Ho = 2 * H; Wo = 2 * W; }
    else { Ho = (H - 1) / 2 + 1; Wo = (W - 1) / 2 + 1; }              // k 3 pad 1 and k 7 pad 3 alike
}
const char* desc_error(const kpn_conv2d_s2_desc* d) {
    if (const char* e = weight_error(d)) return e;
    if (d->N < 1 || d->H < 1 || d->W < 1) return "N, H, W must be positive";
    if (d->kind == KPN_S2_CONV3 && ((d->H | d->W) & 1)) return "H, W must be even for KPN_S2_CONV3 (the input gradient is a transposed convolution)";
    const int64_t big = d->kind == KPN_S2_DECONV3 ? 4 : 1;
    if ((int64_t)d->N * d->H * d->W * big * std::max(d->cin, d->cout) >= (1ll << 31)) return "N * H * W * channels must stay below 2^31 (for both x and y)";
    if (d->has_bias != 0 && d->has_bias != 1) return "has_bias must be 0 or 1";
    return nullptr;
}
// The GEMMs of a layer.  `fwd` and `dx` are k_enc_conv launches; `wg` is the GEMM whose im2col rows and tile the weight gradient
// takes: the forward's for the convolutions, the input gradient's for the transposed layer (the swapped roles).
struct Geoms { enc::ConvGeom fwd, dx, wg; bool has_dx; };
Geoms geoms(const kpn_conv2d_s2_desc* d, int N, int H, int W) {
    Geoms g{};
    int Ho, Wo;
    out_hw(d->kind, H, W, Ho, Wo);
    if (d->kind == KPN_S2_CONV3) {
        g.fwd = enc::conv_geom(N, Ho, Wo, d->cin, d->cout, 3, 3, 0);
        g.dx = enc::conv_geom(N, Ho, Wo, d->cout, d->cin, 3, 3, 1);          // dy (Ho, Wo) -> dx (2 Ho, 2 Wo)
        g.wg = g.fwd; g.has_dx = true;
    } else if (d->kind == KPN_S2_STEM7) {
        g.fwd = enc::conv_geom(N, Ho, Wo, d->cin, d->cout, 7, 7, 0);
        g.wg = g.fwd; g.has_dx = false;
    } else {
        g.fwd = enc::conv_geom(N, H, W, d->cin, d->cout, 3, 3, 1);           // x (H, W) -> y (2 H, 2 W)
        g.dx = enc::conv_geom(N, H, W, d->cout, d->cin, 3, 3, 0);            // dy (2 H, 2 W) -> dx (H, W), stride 2
        g.wg = g.dx; g.has_dx = true;
    }
    return g;
}
struct Plan {
    int Ho, Wo;
    Geoms g;
    enc::WgradPlan wg;
    int64_t My;                // pixels of y: the rows of the bias gradient
    size_t o_fwd, o_dx, o_wg, o_db, bytes;
};
Plan plan(const kpn_conv2d_s2_desc* d) {
    Plan p{};
    out_hw(d->kind, d->H, d->W, p.Ho, p.Wo);
    p.g = geoms(d, d->N, d->H, d->W);
    p.wg = enc::wgrad_plan(p.g.wg);
    p.My = (int64_t)d->N * p.Ho * p.Wo;
    Carver f, b;
    p.o_fwd = f.take((size_t)p.g.fwd.partial * sizeof(float));
    p.o_dx = b.take((size_t)(p.g.has_dx ? p.g.dx.partial : 0) * sizeof(float));
    p.o_wg = b.take((size_t)p.wg.partial * sizeof(float));
    p.o_db = b.take((size_t)enc::dbias_chunks(p.My) * d->cout * sizeof(double));
    p.bytes = std::max<size_t>(std::max(f.o, b.o), 256);
    return p;
}
// the source side of a stride-2 k_enc_conv / k_enc_wgrad over the NHWC tensor src (Hs, Ws, C): k 3 pad 1
inline void strided_source(kpn_enc_conv_args& a, const float* src, int Hs, int Ws) {
    a.Hs = Hs; a.Ws = Ws; a.stride = 2; a.pad = 1; a.src = src; a.src_cs = a.cin;
}
// ... of the stem over the NCHW tensor src (cin, H, W), loaded as it is: k 7 pad 3
inline void stem_source(kpn_enc_conv_args& a, const float* src, int H, int W) {
    a.Hs = H; a.Ws = W; a.Hraw = H; a.Wraw = W; a.ds = 0; a.stem_plain = 1; a.stride = 2; a.pad = 3; a.src = src; a.src_cs = a.cin;
}
// ... of the transposed convolution over the NHWC tensor src (Hs, Ws, C)
inline void deconv_source(kpn_enc_conv_args& a, const float* src, int Hs, int Ws) {
    a.Hs = Hs; a.Ws = Ws; a.stride = 1; a.pad = 0; a.src = src; a.src_cs = a.cin;
}
inline void sink(kpn_enc_conv_args& a, const enc::ConvGeom& g, const float* wp, const float* bias, float* dst, float* partial) {
    a.wp = wp; a.bias = bias; a.dst = dst; a.dst_cs = a.cout; a.partial = g.partial ? partial : nullptr;
}
}  // namespace s2

#define KPN_S2_REQUIRE_DESC(desc) do { if (const char* e_ = s2::desc_error(desc)) return fail(KPN_EINVAL, std::string("kpn_conv2d_s2_desc: ") + e_); } while (0)

extern "C" size_t kpn_conv2d_s2_packed_floats(const kpn_conv2d_s2_desc* desc) {
    if (s2::weight_error(desc)) return 0;
    const s2::Geoms g = s2::geoms(desc, 1, 2, 2);
    return (size_t)(g.fwd.packed + (g.has_dx ? g.dx.packed : 0));
}
extern "C" int kpn_conv2d_s2_pack_device(const kpn_conv2d_s2_desc* desc, const float* w, float* packed, void* stream) {
    if (const char* e = s2::weight_error(desc)) return fail(KPN_EINVAL, std::string("kpn_conv2d_s2_desc: ") + e);
    KPN_REQUIRE(w && packed, "null pointer");
    KPN_REQUIRE(((uintptr_t)packed & 15) == 0, "packed must be 16-byte aligned");
    const s2::Geoms g = s2::geoms(desc, 1, 2, 2);
    // both copies read the weight as the layer holds it: OIHW through the plain mode is [GEMM cout][GEMM cin], (cin, cout, 3, 3)
    // through the deconv mode is [GEMM cin][GEMM cout]; the input gradient exchanges the counts and so takes the other mode
    enc::launch_pack(g.fwd, 0, w, packed, stream);
    if (g.has_dx) enc::launch_pack(g.dx, 0, w, packed + g.fwd.packed, stream);
    return check_launch("kpn_conv2d_s2_pack_device");
}
extern "C" size_t kpn_conv2d_s2_workspace_bytes(const kpn_conv2d_s2_desc* desc) {
    return s2::desc_error(desc) ? 0 : s2::plan(desc).bytes;
}
extern "C" int32_t kpn_conv2d_s2_wgrad_ranges(const kpn_conv2d_s2_desc* desc) {
    return s2::desc_error(desc) ? 0 : s2::plan(desc).wg.nranges;
}
extern "C" int kpn_conv2d_s2_forward(const kpn_conv2d_s2_desc* desc, const float* x, const float* packed, const float* bias, float* y,
                                     void* workspace, size_t workspace_bytes, void* stream) {
    KPN_S2_REQUIRE_DESC(desc);
    KPN_REQUIRE(x && packed && y && workspace, "null pointer");
    KPN_REQUIRE((bias != nullptr) == (desc->has_bias != 0), "bias must be given exactly when has_bias is set");
    KPN_REQUIRE((((uintptr_t)packed | (uintptr_t)workspace) & 15) == 0, "packed / workspace must be 16-byte aligned");
    KPN_REQUIRE(desc->kind == KPN_S2_STEM7 || ((uintptr_t)x & 15) == 0, "x must be 16-byte aligned");
    const s2::Plan p = s2::plan(desc);
    KPN_REQUIRE(workspace_bytes >= p.bytes, "workspace too small (kpn_conv2d_s2_workspace_bytes)");
    kpn_enc_conv_args a = p.g.fwd.a;
    if (desc->kind == KPN_S2_CONV3) s2::strided_source(a, x, desc->H, desc->W);
    else if (desc->kind == KPN_S2_STEM7) s2::stem_source(a, x, desc->H, desc->W);
    else s2::deconv_source(a, x, desc->H, desc->W);
    s2::sink(a, p.g.fwd, packed, bias, y, reinterpret_cast<float*>(static_cast<char*>(workspace) + p.o_fwd));
    enc::launch_conv(a, p.g.fwd, desc->kind == KPN_S2_STEM7, stream);
    return check_launch("kpn_conv2d_s2_forward");
}
extern "C" int kpn_conv2d_s2_backward(const kpn_conv2d_s2_desc* desc, const float* x, const float* dy, const float* packed, float* dx,
                                      float* dw, float* db, void* workspace, size_t workspace_bytes, void* stream) {
    KPN_S2_REQUIRE_DESC(desc);
    KPN_REQUIRE(dy && workspace, "null pointer");
    KPN_REQUIRE(!dx || desc->kind != KPN_S2_STEM7, "dx must be NULL for KPN_S2_STEM7 (the stem has no input gradient)");
    KPN_REQUIRE(!dx || packed, "packed is null (the input gradient reads it)");
    KPN_REQUIRE(!dw || x, "x is null (the weight gradient reads it)");
    KPN_REQUIRE(!db || desc->has_bias, "db given for a convolution without bias (has_bias)");
    KPN_REQUIRE((((uintptr_t)dy | (uintptr_t)packed | (uintptr_t)workspace) & 15) == 0, "dy / packed / workspace must be 16-byte aligned");
    KPN_REQUIRE(desc->kind == KPN_S2_STEM7 || ((uintptr_t)x & 15) == 0, "x must be 16-byte aligned");
    const s2::Plan p = s2::plan(desc);
    KPN_REQUIRE(workspace_bytes >= p.bytes, "workspace too small (kpn_conv2d_s2_workspace_bytes)");
    char* ws = static_cast<char*>(workspace);
    if (dx) {
        kpn_enc_conv_args a = p.g.dx.a;
        if (desc->kind == KPN_S2_CONV3) s2::deconv_source(a, dy, p.Ho, p.Wo);
        else s2::strided_source(a, dy, p.Ho, p.Wo);
        s2::sink(a, p.g.dx, packed + p.g.fwd.packed, nullptr, dx, reinterpret_cast<float*>(ws + p.o_dx));
        enc::launch_conv(a, p.g.dx, 0, stream);
    }
    if (dw) {
        kpn_enc_conv_args c = p.g.wg.a;
        const float* rhs = dy;
        if (desc->kind == KPN_S2_CONV3) s2::strided_source(c, x, desc->H, desc->W);
        else if (desc->kind == KPN_S2_STEM7) s2::stem_source(c, x, desc->H, desc->W);
        else { s2::strided_source(c, dy, p.Ho, p.Wo); rhs = x; }             // the swapped roles
        enc::launch_wgrad(c, p.g.wg, p.wg, desc->kind == KPN_S2_STEM7, rhs, c.cout, reinterpret_cast<float*>(ws + p.o_wg), dw, stream);
    }
    if (db) enc::launch_dbias(dy, p.My, desc->cout, reinterpret_cast<double*>(ws + p.o_db), db, stream);
    return check_launch("kpn_conv2d_s2_backward");
}

// ---------------------------------------------------------------------------------------------
// The replication-padded stride-1 convolutions of the texture encoder, forward and gradients: ReplicationPad2d(k / 2) + Conv2d(k) for
// k = 3 (the two convolutions of a ResBlk), k = 7 (the output layer) and the 7x7 stem on an NCHW tensor (reference src/utils.py:199-259).
// Kernels: encoder_kernels.hip; geometry, tiles, split K, the ranges of the weight gradient and every grid come from the launch layer at
// the head of api_encoders.hip, as for the other layers (api_conv.hip, api_strided.hip).  The pad is never materialised:
//   CONV3 / CONV7  y = k_enc_conv(replicate)         dx = k_enc_conv<RPADJ>(dy) over the flipped copy of the weight: the adjoint of the
//                  clamped load, a gather (kpn_enc_load_a_rp_adjoint)              dw = k_enc_wgrad, A from x through the clamped load
//   STEM7          y = k_enc_conv<STEM>(stem_plain, replicate)   no dx             dw = k_enc_wgrad<STEM>, K rows tap * 4 + ci
namespace rp {
inline int k_of(int kind) { return kind == KPN_RP_CONV3 ? 3 : 7; }
const char* weight_error(const kpn_conv2d_rp_desc* d) {
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
const char* desc_error(const kpn_conv2d_rp_desc* d) {
    if (const char* e = weight_error(d)) return e;
    if (d->N < 1 || d->H < 1 || d->W < 1) return "N, H, W must be positive";
    if ((int64_t)d->N * d->H * d->W * std::max(d->cin, d->cout) >= (1ll << 31)) return "N * H * W * channels must stay below 2^31 (for both x and y)";
    if (d->has_bias != 0 && d->has_bias != 1) return "has_bias must be 0 or 1";
    return nullptr;
}
// The GEMMs of a layer: `fwd` (its tile is the weight gradient's too) and, not for the stem, `dx` with the channel counts exchanged.  The
// output grid is the input grid.
struct Geoms { enc::ConvGeom fwd, dx; bool has_dx; };
Geoms geoms(const kpn_conv2d_rp_desc* d, int N, int H, int W) {
    Geoms g{};
    const int k = k_of(d->kind);
    g.fwd = enc::conv_geom(N, H, W, d->cin, d->cout, k, k, 0);
    g.has_dx = d->kind != KPN_RP_STEM7;
    if (g.has_dx) g.dx = enc::conv_geom(N, H, W, d->cout, d->cin, k, k, 0);
    return g;
}
struct Plan {
    Geoms g;
    enc::WgradPlan wg;
    size_t o_fwd, o_dx, o_wg, o_db, bytes;
};
Plan plan(const kpn_conv2d_rp_desc* d) {
    Plan p{};
    p.g = geoms(d, d->N, d->H, d->W);
    p.wg = enc::wgrad_plan(p.g.fwd);
    // the forward and the backward never run at once on a workspace: the larger of the two
    Carver f, b;
    p.o_fwd = f.take((size_t)p.g.fwd.partial * sizeof(float));
    p.o_dx = b.take((size_t)(p.g.has_dx ? p.g.dx.partial : 0) * sizeof(float));
    p.o_wg = b.take((size_t)p.wg.partial * sizeof(float));
    p.o_db = b.take((size_t)enc::dbias_chunks(p.g.fwd.M) * d->cout * sizeof(double));
    p.bytes = std::max<size_t>(std::max(f.o, b.o), 256);
    return p;
}
// the source side of the forward / the weight gradient: the clamped load over x, NHWC (H, W, cin) or, for the stem, NCHW as it is
inline void source(kpn_enc_conv_args& a, const kpn_conv2d_rp_desc* d, const float* x) {
    a.Hs = d->H; a.Ws = d->W; a.stride = 1; a.pad = k_of(d->kind) / 2; a.replicate = 1; a.src = x; a.src_cs = a.cin;
    if (d->kind == KPN_RP_STEM7) { a.Hraw = d->H; a.Wraw = d->W; a.ds = 0; a.stem_plain = 1; }
}
}  // namespace rp

#define KPN_RP_REQUIRE_DESC(desc) do { if (const char* e_ = rp::desc_error(desc)) return fail(KPN_EINVAL, std::string("kpn_conv2d_rp_desc: ") + e_); } while (0)

extern "C" size_t kpn_conv2d_rp_packed_floats(const kpn_conv2d_rp_desc* desc) {
    if (rp::weight_error(desc)) return 0;
    const rp::Geoms g = rp::geoms(desc, 1, 1, 1);
    return (size_t)(g.fwd.packed + (g.has_dx ? g.dx.packed : 0));
}
extern "C" int kpn_conv2d_rp_pack_device(const kpn_conv2d_rp_desc* desc, const float* w_oihw, float* packed, void* stream) {
    if (const char* e = rp::weight_error(desc)) return fail(KPN_EINVAL, std::string("kpn_conv2d_rp_desc: ") + e);
    KPN_REQUIRE(w_oihw && packed, "null pointer");
    KPN_REQUIRE(((uintptr_t)packed & 15) == 0, "packed must be 16-byte aligned");
    const rp::Geoms g = rp::geoms(desc, 1, 1, 1);
    enc::launch_pack(g.fwd, 0, w_oihw, packed, stream);
    if (g.has_dx) enc::launch_pack(g.dx, 1, w_oihw, packed + g.fwd.packed, stream);      // transposed and flipped, as kpn_conv2d_pack_device
    return check_launch("kpn_conv2d_rp_pack_device");
}
extern "C" size_t kpn_conv2d_rp_workspace_bytes(const kpn_conv2d_rp_desc* desc) {
    return rp::desc_error(desc) ? 0 : rp::plan(desc).bytes;
}
extern "C" int32_t kpn_conv2d_rp_wgrad_ranges(const kpn_conv2d_rp_desc* desc) {
    return rp::desc_error(desc) ? 0 : rp::plan(desc).wg.nranges;
}
extern "C" int kpn_conv2d_rp_forward(const kpn_conv2d_rp_desc* desc, const float* x, const float* packed, const float* bias, float* y,
                                     void* workspace, size_t workspace_bytes, void* stream) {
    KPN_RP_REQUIRE_DESC(desc);
    KPN_REQUIRE(x && packed && y && workspace, "null pointer");
    KPN_REQUIRE((bias != nullptr) == (desc->has_bias != 0), "bias must be given exactly when has_bias is set");
    KPN_REQUIRE((((uintptr_t)packed | (uintptr_t)workspace) & 15) == 0, "packed / workspace must be 16-byte aligned");
    KPN_REQUIRE(desc->kind == KPN_RP_STEM7 || ((uintptr_t)x & 15) == 0, "x must be 16-byte aligned");
    const rp::Plan p = rp::plan(desc);
    KPN_REQUIRE(workspace_bytes >= p.bytes, "workspace too small (kpn_conv2d_rp_workspace_bytes)");
    kpn_enc_conv_args a = p.g.fwd.a;
    rp::source(a, desc, x);
    a.wp = packed; a.bias = bias; a.dst = y; a.dst_cs = a.cout;
    a.partial = p.g.fwd.partial ? reinterpret_cast<float*>(static_cast<char*>(workspace) + p.o_fwd) : nullptr;
    enc::launch_conv(a, p.g.fwd, desc->kind == KPN_RP_STEM7, stream);
    return check_launch("kpn_conv2d_rp_forward");
}
extern "C" int kpn_conv2d_rp_backward(const kpn_conv2d_rp_desc* desc, const float* x, const float* dy, const float* packed, float* dx,
                                      float* dw, float* db, void* workspace, size_t workspace_bytes, void* stream) {
    KPN_RP_REQUIRE_DESC(desc);
    KPN_REQUIRE(dy && workspace, "null pointer");
    KPN_REQUIRE(!dx || desc->kind != KPN_RP_STEM7, "dx must be NULL for KPN_RP_STEM7 (the stem has no input gradient)");
    KPN_REQUIRE(!dx || packed, "packed is null (the input gradient reads it)");
    KPN_REQUIRE(!dw || x, "x is null (the weight gradient reads it)");
    KPN_REQUIRE(!db || desc->has_bias, "db given for a convolution without bias (has_bias)");
    KPN_REQUIRE((((uintptr_t)dy | (uintptr_t)packed | (uintptr_t)workspace) & 15) == 0, "dy / packed / workspace must be 16-byte aligned");
    KPN_REQUIRE(desc->kind == KPN_RP_STEM7 || ((uintptr_t)x & 15) == 0, "x must be 16-byte aligned");
    const rp::Plan p = rp::plan(desc);
    KPN_REQUIRE(workspace_bytes >= p.bytes, "workspace too small (kpn_conv2d_rp_workspace_bytes)");
    char* ws = static_cast<char*>(workspace);
    if (dx) {
        kpn_enc_conv_args a = p.g.dx.a;
        a.Hs = desc->H; a.Ws = desc->W; a.stride = 1; a.pad = rp::k_of(desc->kind) / 2; a.src = dy; a.src_cs = a.cin;
        a.wp = packed + p.g.fwd.packed; a.dst = dx; a.dst_cs = a.cout;
        a.partial = p.g.dx.partial ? reinterpret_cast<float*>(ws + p.o_dx) : nullptr;
        enc::launch_conv_rp_adjoint(a, p.g.dx, stream);
    }
    if (dw) {
        kpn_enc_conv_args c = p.g.fwd.a;
        rp::source(c, desc, x);
        enc::launch_wgrad(c, p.g.fwd, p.wg, desc->kind == KPN_RP_STEM7, dy, c.cout, reinterpret_cast<float*>(ws + p.o_wg), dw, stream);
    }
    if (db) enc::launch_dbias(dy, p.g.fwd.M, desc->cout, reinterpret_cast<double*>(ws + p.o_db), db, stream);
    return check_launch("kpn_conv2d_rp_backward");
}

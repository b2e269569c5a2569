// ---------------------------------------------------------------------------------------------
// One stride-1 convolution, forward and its three gradients (torch.nn.functional.conv2d and its autograd, as the encoders use
// them: reference src/utils.py:416-474, 261-309, 322-414).  Kernels: encoder_kernels.hip.  The forward and the input gradient
// are k_enc_conv over two packed copies of the weight, sized and launched by the launch layer at the head of api_encoders.hip
// (enc::conv_geom / enc::launch_conv: the walk's own tiles and split K); the weight gradient is k_enc_wgrad / k_enc_wgrad_combine
// on the forward's tile (enc::wgrad_plan / enc::launch_wgrad), the bias gradient k_enc_dbias_partial / k_enc_dbias_final
// (enc::launch_dbias).  api_strided.hip serves the stride-2, stem and transposed layers through the same layer.
namespace conv {
// what the packed copies depend on
const char* weight_error(const kpn_conv2d_desc* d) {
    if (!d) return "desc is null";
    if (d->k != 1 && d->k != 3 && d->k != 5) return "k must be 1, 3 or 5 (square kernel, stride 1; the 7x7 stems and stride 2 are not served)";
    if (d->cin < 4 || d->cin % 4 || d->cin > 1024) return "cin must be a multiple of 4 in 4 .. 1024";
    if (d->cout < 4 || d->cout % 4 || d->cout > 1024) return "cout must be a multiple of 4 in 4 .. 1024";
    return nullptr;
}
const char* desc_error(const kpn_conv2d_desc* d) {
    if (const char* e = weight_error(d)) return e;
    if (d->pad < 0 || d->pad > d->k - 1) return "pad must be in 0 .. k - 1";
    if (d->N < 1 || d->H < 1 || d->W < 1) return "N, H, W must be positive";
    if (d->H + 2 * d->pad - d->k + 1 < 1 || d->W + 2 * d->pad - d->k + 1 < 1) return "H, W: the output would be empty";
    if ((int64_t)d->N * (d->H + 2 * d->pad) * (d->W + 2 * d->pad) * std::max(d->cin, d->cout) >= (1ll << 31)) return "N * H * W * channels must stay below 2^31";
    if (d->has_bias != 0 && d->has_bias != 1) return "has_bias must be 0 or 1";
    return nullptr;
}
// the forward's and the input gradient's GEMMs, the weight gradient's ranges (enc::wgrad_plan) and the workspace
struct Plan {
    int Ho, Wo;
    enc::ConvGeom fwd, dx;
    enc::WgradPlan wg;
    size_t o_fwd, o_dx, o_wg, o_db, bytes;
};
Plan plan(const kpn_conv2d_desc* d) {
    Plan p{};
    p.Ho = d->H + 2 * d->pad - d->k + 1; p.Wo = d->W + 2 * d->pad - d->k + 1;
    p.fwd = enc::conv_geom(d->N, p.Ho, p.Wo, d->cin, d->cout, d->k, d->k, 0);
    p.dx = enc::conv_geom(d->N, d->H, d->W, d->cout, d->cin, d->k, d->k, 0);
    p.wg = enc::wgrad_plan(p.fwd);                                  // the forward's tile over (K rows, cout)
    // the forward and the backward never run at once on a workspace: the larger of the two
    Carver f, b;
    p.o_fwd = f.take((size_t)p.fwd.partial * sizeof(float));
    p.o_dx = b.take((size_t)p.dx.partial * sizeof(float));
    p.o_wg = b.take((size_t)p.wg.partial * sizeof(float));
    p.o_db = b.take((size_t)enc::dbias_chunks(p.fwd.M) * d->cout * sizeof(double));
    p.bytes = std::max<size_t>(std::max(f.o, b.o), 256);
    return p;
}
// dst (N, Ho, Wo, cout) = conv(src (N, Hs, Ws, cin), wp, pad) [+ bias]
void run(const enc::ConvGeom& g, int Hs, int Ws, int pad, const float* src, const float* wp, const float* bias, float* dst, float* partial,
         void* stream) {
    kpn_enc_conv_args a = g.a;
    a.Hs = Hs; a.Ws = Ws; a.stride = 1; a.pad = pad;
    a.src = src; a.src_cs = a.cin;
    a.wp = wp; a.bias = bias;
    a.dst = dst; a.dst_cs = a.cout;
    a.partial = g.partial ? partial : nullptr;
    enc::launch_conv(a, g, 0, stream);
}
}  // namespace conv

#define KPN_CONV_REQUIRE_DESC(desc) do { if (const char* e_ = conv::desc_error(desc)) return fail(KPN_EINVAL, std::string("kpn_conv2d_desc: ") + e_); } while (0)

extern "C" size_t kpn_conv2d_packed_floats(const kpn_conv2d_desc* desc) {
    if (conv::weight_error(desc)) return 0;
    const int k = desc->k;
    return (size_t)(enc::conv_geom(1, 1, 1, desc->cin, desc->cout, k, k, 0).packed + enc::conv_geom(1, 1, 1, desc->cout, desc->cin, k, k, 0).packed);
}
extern "C" int kpn_conv2d_pack_device(const kpn_conv2d_desc* desc, const float* w_oihw, float* packed, void* stream) {
    if (const char* e = conv::weight_error(desc)) return fail(KPN_EINVAL, std::string("kpn_conv2d_desc: ") + e);
    KPN_REQUIRE(w_oihw && packed, "null pointer");
    KPN_REQUIRE(((uintptr_t)packed & 15) == 0, "packed must be 16-byte aligned");
    const int k = desc->k;
    const enc::ConvGeom f = enc::conv_geom(1, 1, 1, desc->cin, desc->cout, k, k, 0), b = enc::conv_geom(1, 1, 1, desc->cout, desc->cin, k, k, 0);
    enc::launch_pack(f, 0, w_oihw, packed, stream);
    enc::launch_pack(b, 1, w_oihw, packed + f.packed, stream);
    return check_launch("kpn_conv2d_pack_device");
}
extern "C" size_t kpn_conv2d_workspace_bytes(const kpn_conv2d_desc* desc) {
    return conv::desc_error(desc) ? 0 : conv::plan(desc).bytes;
}
extern "C" int32_t kpn_conv2d_wgrad_ranges(const kpn_conv2d_desc* desc) {
    return conv::desc_error(desc) ? 0 : conv::plan(desc).wg.nranges;
}
extern "C" int kpn_conv2d_forward(const kpn_conv2d_desc* desc, const float* x, const float* packed, const float* bias, float* y,
                                  void* workspace, size_t workspace_bytes, void* stream) {
    KPN_CONV_REQUIRE_DESC(desc);
    KPN_REQUIRE(x && packed && y && workspace, "null pointer");
    KPN_REQUIRE((bias != nullptr) == (desc->has_bias != 0), "bias must be given exactly when has_bias is set");
    KPN_REQUIRE((((uintptr_t)x | (uintptr_t)packed | (uintptr_t)workspace) & 15) == 0, "x / packed / workspace must be 16-byte aligned");
    const conv::Plan p = conv::plan(desc);
    KPN_REQUIRE(workspace_bytes >= p.bytes, "workspace too small (kpn_conv2d_workspace_bytes)");
    char* ws = static_cast<char*>(workspace);
    conv::run(p.fwd, desc->H, desc->W, desc->pad, x, packed, bias, y, reinterpret_cast<float*>(ws + p.o_fwd), stream);
    return check_launch("kpn_conv2d_forward");
}
extern "C" int kpn_conv2d_backward(const kpn_conv2d_desc* desc, const float* x, const float* dy, const float* packed, float* dx,
                                   float* dw, float* db, void* workspace, size_t workspace_bytes, void* stream) {
    KPN_CONV_REQUIRE_DESC(desc);
    KPN_REQUIRE(dy && workspace, "null pointer");
    KPN_REQUIRE(!dx || packed, "packed is null (the input gradient reads it)");
    KPN_REQUIRE(!dw || x, "x is null (the weight gradient reads it)");
    KPN_REQUIRE(!db || desc->has_bias, "db given for a convolution without bias (has_bias)");
    KPN_REQUIRE((((uintptr_t)x | (uintptr_t)dy | (uintptr_t)packed | (uintptr_t)workspace) & 15) == 0, "x / dy / packed / workspace must be 16-byte aligned");
    const conv::Plan p = conv::plan(desc);
    KPN_REQUIRE(workspace_bytes >= p.bytes, "workspace too small (kpn_conv2d_workspace_bytes)");
    char* ws = static_cast<char*>(workspace);
    const int k = desc->k;
    if (dx)     // dX = conv(dY, w'[ci][co][k - 1 - ky][k - 1 - kx], pad k - 1 - p)
        conv::run(p.dx, p.Ho, p.Wo, k - 1 - desc->pad, dy, packed + p.fwd.packed, nullptr, dx, reinterpret_cast<float*>(ws + p.o_dx), stream);
    if (dw) {
        kpn_enc_conv_args c = p.fwd.a;
        c.Hs = desc->H; c.Ws = desc->W; c.stride = 1; c.pad = desc->pad;
        c.src = x; c.src_cs = desc->cin;
        enc::launch_wgrad(c, p.fwd, p.wg, 0, dy, desc->cout, reinterpret_cast<float*>(ws + p.o_wg), dw, stream);
    }
    if (db) enc::launch_dbias(dy, p.fwd.M, desc->cout, reinterpret_cast<double*>(ws + p.o_db), db, stream);
    return check_launch("kpn_conv2d_backward");
}

// ---------------------------------------------------------------------------------------------
// One stride-1 convolution, forward and its three gradients (torch.nn.functional.conv2d and its autograd, as the encoders use
// them: reference src/utils.py:416-474, 261-309, 322-414).  Kernels: encoder_kernels.hip.  The forward and the input gradient
// are k_enc_conv over two packed copies of the weight, sized and launched by the launch layer at the head of api_encoders.hip
// (enc::conv_geom / enc::launch_conv: the walk's own tiles and split K); the weight gradient is k_enc_wgrad / k_enc_wgrad_combine
// on the forward's tile, the bias gradient k_enc_dbias_partial / k_enc_dbias_final.
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
// The ranges of the weight gradient: a range is `cpr` chunks of 16 output pixels, at least 20 (320 pixels: what a tile's store
// and combine are worth) and otherwise as many as leave about 1024 workgroups, at most 64 ranges.  From the shape alone.
struct Plan {
    int Ho, Wo;
    enc::ConvGeom fwd, dx;
    int wg_tiles, krows, nchunks, cpr, nranges, db_chunks;
    size_t o_fwd, o_dx, o_wg, o_db, bytes;
};
Plan plan(const kpn_conv2d_desc* d) {
    Plan p{};
    p.Ho = d->H + 2 * d->pad - d->k + 1; p.Wo = d->W + 2 * d->pad - d->k + 1;
    p.fwd = enc::conv_geom(d->N, p.Ho, p.Wo, d->cin, d->cout, d->k, d->k, 0);
    p.dx = enc::conv_geom(d->N, d->H, d->W, d->cout, d->cin, d->k, d->k, 0);
    const int64_t M = p.fwd.M;
    p.krows = d->k * d->k * d->cin;
    p.wg_tiles = (p.krows + p.fwd.bm - 1) / p.fwd.bm * (p.fwd.a.cout_p / p.fwd.bn);      // the forward's tile over (K rows, cout)
    p.nchunks = (int)((M + 15) / 16);
    const int rmax = std::max(1, std::min(64, 1024 / p.wg_tiles));
    p.cpr = std::max(20, (p.nchunks + rmax - 1) / rmax);
    p.nranges = (p.nchunks + p.cpr - 1) / p.cpr;
    p.db_chunks = (int)std::max<int64_t>(1, std::min<int64_t>(256, M / 256));
    // the forward and the backward never run at once on a workspace: the larger of the two
    Carver f, b;
    p.o_fwd = f.take((size_t)p.fwd.partial * sizeof(float));
    p.o_dx = b.take((size_t)p.dx.partial * sizeof(float));
    p.o_wg = b.take((size_t)p.nranges * p.krows * d->cout * sizeof(float));
    p.o_db = b.take((size_t)p.db_chunks * d->cout * sizeof(double));
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
    return conv::desc_error(desc) ? 0 : conv::plan(desc).nranges;
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
        kpn_enc_wgrad_args a{};
        a.c = p.fwd.a;
        a.c.Hs = desc->H; a.c.Ws = desc->W; a.c.stride = 1; a.c.pad = desc->pad;
        a.c.src = x; a.c.src_cs = desc->cin;
        a.dy = dy; a.krows = p.krows; a.nchunks = p.nchunks; a.cpr = p.cpr; a.nranges = p.nranges;
        a.partial = reinterpret_cast<float*>(ws + p.o_wg); a.dw = dw;
        const dim3 grid((unsigned)p.wg_tiles, (unsigned)p.nranges);
        if (p.fwd.bn == 64) KPN_LAUNCH((k_enc_wgrad<64, 64>), grid, dim3(256), stream, a);
        else KPN_LAUNCH((k_enc_wgrad<128, 32>), grid, dim3(256), stream, a);
        KPN_LAUNCH(k_enc_wgrad_combine, enc::grid4((int64_t)p.krows * desc->cout), dim3(256), stream, a);
    }
    if (db) {
        kpn_enc_dbias_args a{dy, (int64_t)desc->N * p.Ho * p.Wo, desc->cout, p.db_chunks, reinterpret_cast<double*>(ws + p.o_db), db};
        KPN_LAUNCH(k_enc_dbias_partial, dim3((unsigned)p.db_chunks), dim3(256), stream, a);
        KPN_LAUNCH(k_enc_dbias_final, dim3((unsigned)((desc->cout + 63) / 64)), dim3(64), stream, a);
    }
    return check_launch("kpn_conv2d_backward");
}

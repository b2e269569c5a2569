// ---------------------------------------------------------------------------------------------
// A whole ConvBlock (reference src/utils.py:416-474, norm = "group") as one differentiable operator: the encoder walk's fused forward
// (enc::conv_block in api_encoders.hip) with what a backward needs kept, and a backward fused in the same way.  Kernels:
// encoder_kernels.hip, launched through the launch layer at the head of api_encoders.hip, so a block, a walk and the single layers
// (api_conv.hip, api_norm.hip) share tiles, split K, weight-gradient ranges and chunk counts - and with them the order of every sum.
//
// With c = cout, widths (w1, w2, w3) = (c / 2, c / 4, c / 4), slices s1 = [0, w1), s2 = [w1, w1 + w2), s3 = [w1 + w2, c), P = N H W:
//   forward   ss_i = stats(source_i) -> o_i = conv_i(relu(fma(source_i, scale_i, shift_i)))  (the norm and the ReLU in the A loads);
//             source_1 = x, source_2 = o_1, source_3 = o_2.  o_1 and o_2 go, un-added, to S (P x 3c/4, the kept activations);
//             base = x (cin == cout) or conv_4(relu(fma(x, scale_4, shift_4))) written to y (the downsample leg, 1 x 1);
//             y[s3] = o_3 + base[s3] in the epilogue of conv_3 (o_3 is never stored), y[s1, s2] = S + base[s1, s2] (k_enc_add_cs).
//             No normalised tensor and no concatenation exists.
//   backward  dO = dy.  For the legs i = 3, 2, 1 with R_3 = dO[s3] (a slice: src_cs / rhs_cs = c), R_2 = G_2, R_1 = G_1:
//               d(n_i) = conv(R_i, flipped copy of w_i)           (k_enc_conv, the input gradient of api_conv.hip)
//               dW_i   = wgrad(A = relu(fma(source_i, ss_i)) in the loads, R = R_i)
//               G_{i-1}, dgamma_i, dbeta_i = norm backward over (x = source_i, dy = d(n_i)) with add = dO[s_{i-1}]
//             - the addend is the part of dO that reached o_{i-1} through the concatenation.  Leg 1 writes dX: with add = dO for the
//             identity residual, without an addend in front of leg 4 = the same three steps over (x, ss_4, R = dO), whose norm
//             backward runs with add = dX in place.
// The order of the dX sum: dX = dO + (g a + (x c2 + c3))_bn1 for cin == cout; dX = (g a + (x c2 + c3))_bn1 first, then
// dX = dX + (g a + (x c2 + c3))_bn4, for cin != cout.  Every sum runs in the fixed order its kernel has: no atomics, equal bits from
// run to run, and an image's y and dX do not depend on its batch.
namespace blk {
inline bool pow2_width(int v) { return v >= 4 && v <= 1024 && !(v & (v - 1)); }
const char* desc_error(const kpn_conv_block_desc* d) {
    if (!d) return "desc is null";
    if (!pow2_width(d->cin)) return "cin must be a power of two in 4 .. 1024";
    if (d->cout < 8 || d->cout % 4 || !pow2_width(d->cout / 2)) return "cout / 2 must be a power of two in 4 .. 1024";
    if (!pow2_width(d->cout / 4)) return "cout / 4 must be a power of two in 4 .. 1024";
    if (d->cin != d->cout && d->cout > 1024) return "cout must be at most 1024 with a downsample leg (cin != cout)";
    if (d->N < 1 || d->H < 1 || d->W < 1) return "N, H, W must be positive";
    if (d->N > 65535) return "N must be at most 65535 (one grid row per image)";
    if ((int64_t)d->H * d->W >= (1ll << 31) || (int64_t)d->N * d->H * d->W * std::max(d->cin, d->cout) >= (1ll << 31))
        return "N * H * W * max(cin, cout) must stay below 2^31";
    if (!(d->eps > 0.0f)) return "eps must be positive";
    return nullptr;
}
// leg i: GroupNorm(min(32, cin), cin) + ReLU in the loads of a k x k convolution cin -> cout
struct Leg {
    int cin, cout, G, nchunks;
    enc::Layer e;               // the convolution (api_layer.hip): zero pad k / 2, k 3 or (the downsample leg) 1
    int64_t stat_doubles;
    size_t ss, mr;              // offsets (floats) in `state`
};
struct Plan {
    int nlegs, HW, cs;          // cs = 3 cout / 4: the channel stride of S
    int64_t P;
    Leg leg[4];
    size_t state_floats;
    size_t f_stats, f_conv;                                 // the forward's workspace (byte offsets)
    size_t b_dn, b_g2, b_g1, b_conv, b_wg, b_stats, b_coef; // the backward's
    size_t bytes;
};
// arith: the arithmetic of every leg's three GEMMs (KPN_CONV_F32 / KPN_CONV_BF16X3); the norms, the adds and the order of the legs do not
// depend on it
Plan plan(const kpn_conv_block_desc* d, int arith = KPN_CONV_F32) {
    Plan p{};
    const int c = d->cout;
    p.nlegs = d->cin != c ? 4 : 3;
    p.HW = d->H * d->W; p.P = (int64_t)d->N * p.HW; p.cs = c / 2 + c / 4;
    const int cin[4] = {d->cin, c / 2, c / 4, d->cin}, co[4] = {c / 2, c / 4, c / 4, c};
    size_t st = (size_t)p.P * p.cs;
    size_t stat = 0, fconv = 0, bconv = 0, wg = 0, dn = 0, coef = 0;
    for (int i = 0; i < p.nlegs; ++i) {
        Leg& l = p.leg[i];
        const int k = i < 3 ? 3 : 1;
        l.cin = cin[i]; l.cout = co[i]; l.G = std::min(32, l.cin);
        l.e = enc::layer(enc::LayerSpec{l.cin, l.cout, k, 1, k / 2, 0, 0, 0, arith}, d->N, d->H, d->W);
        l.nchunks = enc::stats_chunks(d->N, p.HW, l.cin, &l.stat_doubles);
        l.ss = st; st += (size_t)2 * d->N * l.cin;
        l.mr = st; st += (size_t)2 * d->N * l.G;
        stat = std::max(stat, (size_t)l.stat_doubles * sizeof(double));
        fconv = std::max(fconv, (size_t)l.e.fwd.partial * sizeof(float));
        bconv = std::max(bconv, (size_t)l.e.dx.partial * sizeof(float));
        wg = std::max(wg, (size_t)l.e.wgp.partial * sizeof(float));
        dn = std::max(dn, (size_t)p.P * l.cin * sizeof(float));
        coef = std::max(coef, (size_t)3 * d->N * l.cin * sizeof(float));
    }
    p.state_floats = st;
    // the forward and the backward never run at once on a workspace: the larger of the two
    Carver f, b;
    p.f_stats = f.take(stat);
    p.f_conv = f.take(fconv);
    p.b_dn = b.take(dn);
    p.b_g2 = b.take((size_t)p.P * (c / 4) * sizeof(float));
    p.b_g1 = b.take((size_t)p.P * (c / 2) * sizeof(float));
    p.b_conv = b.take(bconv);
    p.b_wg = b.take(wg);
    p.b_stats = b.take(stat);
    p.b_coef = b.take(coef);
    p.bytes = std::max<size_t>(std::max(f.o, b.o), 256);
    return p;
}
// The launches of a block's forward for a plan of its descriptor: arguments checked by the caller, `ws` the block's workspace (p.bytes).
// kpn_conv_block_ex_forward and the operators that contain blocks (api_geo_train.hip) run this one body
void forward(const Plan& p, const kpn_conv_block_desc* desc, const float* x, const kpn_conv_block_params* params, float* y, float* state,
             char* ws, void* stream) {
    double* stat = reinterpret_cast<double*>(ws + p.f_stats);
    float* part = reinterpret_cast<float*>(ws + p.f_conv);
    const int N = desc->N, c = desc->cout;
    // leg i: dst = conv_i(src normalised and rectified in the loads with ss_i) [+ res], every tensor with its own channel stride
    auto conv = [&](int i, const float* src, int src_cs, float* dst, int dst_cs, const float* res, int res_cs) {
        enc::layer_forward(p.leg[i].e, src, src_cs, state + p.leg[i].ss, params->packed[i], nullptr, dst, dst_cs, res, res_cs, part, stream);
    };
    auto stats = [&](int i, const float* src, int cs) {
        const blk::Leg& l = p.leg[i];
        kpn_enc_stats_args a{};
        a.src = src; a.cs = cs; a.C = l.cin; a.HW = p.HW; a.nchunks = l.nchunks; a.nimg = N;
        a.partial = stat;
        a.G = l.G; a.gamma = params->gamma[i]; a.beta = params->beta[i]; a.eps = desc->eps;
        a.ss = state + l.ss; a.mr = state + l.mr;
        enc::launch_stats(a, stream);
    };
    const float* base = x;
    int base_cs = desc->cin;
    if (p.nlegs == 4) {         // the downsample leg first: y = conv4(relu(bn4(x))), the base the three slices are added to
        stats(3, x, desc->cin);
        conv(3, x, desc->cin, y, c, nullptr, 0);
        base = y; base_cs = c;
    }
    stats(0, x, desc->cin);
    conv(0, x, desc->cin, state, p.cs, nullptr, 0);
    stats(1, state, p.cs);
    conv(1, state, p.cs, state + c / 2, p.cs, nullptr, 0);
    stats(2, state + c / 2, p.cs);
    conv(2, state + c / 2, p.cs, y + p.cs, c, base + p.cs, base_cs);
    enc::launch_add_cs(state, p.cs, base, base_cs, y, c, p.P, p.cs, stream);
}
// The launches of a block's backward, in the same way
void backward(const Plan& p, const kpn_conv_block_desc* desc, const float* x, const float* dy, const kpn_conv_block_params* params,
              const float* state, float* dx, const kpn_conv_block_grads* grads, char* ws, void* stream) {
    float* dn = reinterpret_cast<float*>(ws + p.b_dn);
    float* g1 = reinterpret_cast<float*>(ws + p.b_g1);       // what leg 2 hands to leg 1 (c / 2 channels)
    float* g2 = reinterpret_cast<float*>(ws + p.b_g2);       // what leg 3 hands to leg 2 (c / 4 channels)
    float* cpart = reinterpret_cast<float*>(ws + p.b_conv);
    float* wpart = reinterpret_cast<float*>(ws + p.b_wg);
    double* stat = reinterpret_cast<double*>(ws + p.b_stats);
    float* coef = reinterpret_cast<float*>(ws + p.b_coef);
    const int N = desc->N, c = desc->cout;
    const bool down = p.nlegs == 4;
    // one leg: R (channel stride r_cs) is the gradient of the leg's convolution output; src (stride src_cs) the un-normalised source
    auto leg = [&](int i, const float* src, int src_cs, const float* R, int r_cs, float* gout, const float* add, int add_cs) {
        const blk::Leg& l = p.leg[i];
        float* dgm = grads->dgamma[i];
        float* dbt = grads->dbeta[i];
        if (grads->dw[i]) enc::layer_wgrad(l.e, src, src_cs, state + l.ss, R, r_cs, wpart, grads->dw[i], stream);
        if (!gout && !dgm && !dbt) return;
        enc::layer_dgrad(l.e, R, r_cs, params->packed[i], dn, l.cin, nullptr, 0, cpart, stream);        // d(n_i)
        kpn_enc_norm_bwd_args a{};
        a.x = src; a.x_cs = src_cs; a.dy = dn; a.ss = state + l.ss; a.mr = state + l.mr; a.gamma = params->gamma[i];
        a.relu = 1; a.C = l.cin; a.HW = p.HW; a.nchunks = l.nchunks; a.nimg = N; a.G = l.G;
        a.partial = stat;
        a.coef = gout ? coef : nullptr;
        a.dx = gout; a.dgamma = dgm; a.dbeta = dbt;
        a.add = gout ? add : nullptr; a.add_cs = add_cs;
        enc::launch_norm_bwd(a, stream);
    };
    // what a leg must hand upstream: dX, or a parameter gradient of an earlier leg
    auto wants = [&](int i) { return grads->dgamma[i] || grads->dbeta[i] || grads->dw[i]; };
    const bool up1 = dx != nullptr, up2 = up1 || wants(0), up3 = up2 || wants(1);
    leg(2, state + c / 2, p.cs, dy + p.cs, c, up3 ? g2 : nullptr, dy + c / 2, c);
    if (up3) leg(1, state, p.cs, g2, c / 4, up2 ? g1 : nullptr, dy, c);
    if (up2) leg(0, x, desc->cin, g1, c / 2, up1 ? dx : nullptr, down ? nullptr : dy, c);
    if (down) leg(3, x, desc->cin, dy, c, dx, dx, desc->cin);
}
}  // namespace blk

#define KPN_BLOCK_REQUIRE_DESC(desc) do { if (const char* e_ = blk::desc_error(desc)) return fail(KPN_EINVAL, std::string("kpn_conv_block_desc: ") + e_); } while (0)

#define KPN_BLOCK_REQUIRE_ARITH(arith) do { if (const char* e_ = enc::arith_error(arith)) return fail(KPN_EINVAL, std::string("kpn_conv_block_ex: ") + e_); } while (0)

// The four entry points with the arithmetic chosen by the caller; kpn_conv_block_* below are their arith = KPN_CONV_F32 case.
extern "C" size_t kpn_conv_block_ex_workspace_bytes(const kpn_conv_block_desc* desc, int32_t arith) {
    return blk::desc_error(desc) || enc::arith_error(arith) ? 0 : blk::plan(desc, arith).bytes;
}
extern "C" size_t kpn_conv_block_ex_state_floats(const kpn_conv_block_desc* desc, int32_t arith) {
    return blk::desc_error(desc) || enc::arith_error(arith) ? 0 : blk::plan(desc, arith).state_floats;
}
extern "C" int kpn_conv_block_ex_forward(const kpn_conv_block_desc* desc, int32_t arith, const float* x, const kpn_conv_block_params* params,
                                         float* y, float* state, void* workspace, size_t workspace_bytes, void* stream) {
    KPN_BLOCK_REQUIRE_DESC(desc);
    KPN_BLOCK_REQUIRE_ARITH(arith);
    KPN_REQUIRE(x && params && y && state && workspace, "null pointer");
    const blk::Plan p = blk::plan(desc, arith);
    for (int i = 0; i < p.nlegs; ++i) {
        KPN_REQUIRE(params->gamma[i] && params->beta[i] && params->packed[i], "params: gamma / beta / packed of a leg is null");
        KPN_REQUIRE(enc::aligned16({params->gamma[i], params->beta[i], params->packed[i]}), "params: gamma / beta / packed must be 16-byte aligned");
    }
    KPN_REQUIRE(enc::aligned16({x, y, state, workspace}), "x / y / state / workspace must be 16-byte aligned");
    KPN_REQUIRE(workspace_bytes >= p.bytes, "workspace too small (kpn_conv_block_workspace_bytes)");
    blk::forward(p, desc, x, params, y, state, static_cast<char*>(workspace), stream);
    return check_launch("kpn_conv_block_forward");
}
extern "C" int kpn_conv_block_ex_backward(const kpn_conv_block_desc* desc, int32_t arith, const float* x, const float* dy,
                                          const kpn_conv_block_params* params, const float* state, float* dx, const kpn_conv_block_grads* grads,
                                          void* workspace, size_t workspace_bytes, void* stream) {
    KPN_BLOCK_REQUIRE_DESC(desc);
    KPN_BLOCK_REQUIRE_ARITH(arith);
    KPN_REQUIRE(x && dy && params && state && grads && workspace, "null pointer");
    const blk::Plan p = blk::plan(desc, arith);
    for (int i = 0; i < p.nlegs; ++i) {
        KPN_REQUIRE(params->gamma[i] && params->packed[i], "params: gamma / packed of a leg is null");
        KPN_REQUIRE(enc::aligned16({params->gamma[i], params->packed[i], grads->dgamma[i], grads->dbeta[i], grads->dw[i]}),
                    "params / grads: gamma / packed / dgamma / dbeta / dw must be 16-byte aligned");
    }
    KPN_REQUIRE(p.nlegs == 4 || !(grads->dgamma[3] || grads->dbeta[3] || grads->dw[3]), "grads of the downsample leg given for cin == cout");
    KPN_REQUIRE(enc::aligned16({x, dy, state, dx, workspace}), "x / dy / state / dx / workspace must be 16-byte aligned");
    KPN_REQUIRE(workspace_bytes >= p.bytes, "workspace too small (kpn_conv_block_workspace_bytes)");
    blk::backward(p, desc, x, dy, params, state, dx, grads, static_cast<char*>(workspace), stream);
    return check_launch("kpn_conv_block_backward");
}

extern "C" size_t kpn_conv_block_workspace_bytes(const kpn_conv_block_desc* desc) { return kpn_conv_block_ex_workspace_bytes(desc, KPN_CONV_F32); }
extern "C" size_t kpn_conv_block_state_floats(const kpn_conv_block_desc* desc) { return kpn_conv_block_ex_state_floats(desc, KPN_CONV_F32); }
extern "C" int kpn_conv_block_forward(const kpn_conv_block_desc* desc, const float* x, const kpn_conv_block_params* params, float* y,
                                      float* state, void* workspace, size_t workspace_bytes, void* stream) {
    return kpn_conv_block_ex_forward(desc, KPN_CONV_F32, x, params, y, state, workspace, workspace_bytes, stream);
}
extern "C" int kpn_conv_block_backward(const kpn_conv_block_desc* desc, const float* x, const float* dy, const kpn_conv_block_params* params,
                                       const float* state, float* dx, const kpn_conv_block_grads* grads, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    return kpn_conv_block_ex_backward(desc, KPN_CONV_F32, x, dy, params, state, dx, grads, workspace, workspace_bytes, stream);
}

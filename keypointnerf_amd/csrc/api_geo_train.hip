// ---------------------------------------------------------------------------------------------
// A whole HGFilterV2 (reference src/utils.py:322-414; n_stack = 1, hd = False, norm = "group") as one differentiable operator: the encoder
// walk's forward (enc::geo_walk in api_encoders.hip) with nothing released and what a backward needs kept, and the same walk in reverse.
// Kernels: encoder_kernels.hip, launched through the launch layer at the head of api_encoders.hip, the layers of api_layer.hip and the
// block bodies of api_block.hip (blk::forward / blk::backward), so this operator, the inference walk and the single operators
// (api_conv.hip, api_strided.hip, api_norm.hip, api_block.hip, api_resample.hip) share tiles, split K, weight-gradient ranges and chunk
// counts - and with them the order of every sum.
//   forward   t0 = stem(x);  a1 = relu(bn1(t0)) (k_enc_affine: a block input);  x2 = conv2(a1);
//             d = deconv(x2), x_hd = conv_out(relu(fma(d, ss_unpack)))  (the norm and the ReLU in the A loads);
//             p = pool(x2);  x4 = conv4(conv3(p));  hg = HourGlass(x4);  top = top_m_0(hg);
//             c = conv_last0(top);  out = l0(relu(fma(c, ss_end))).
//             HourGlass level on input inp: up1 = b1(inp); low = pool(inp); low1 = b2(low); low2 = next level(low1) or b2_plus(low1);
//             low3 = b3(low2) (workspace); up1 += U(low3) in place - the level's output.
//   backward  tail: dW, db of l0 with A = relu(fma(c, ss_end)) in the loads, its input gradient, the norm backward of bn_end0 in place;
//             conv_last0; top_m_0.  Level with output gradient dY: d(low3) = up2_bwd(dY); b3; the next level or b2_plus; b2 -> g_low;
//             b1 with dy = dY writes the level's input gradient; then k_enc_pool2_bwd_acc adds 0.25 g_low onto it.  conv4, conv3 -> d(p).
//             hd: dW, db of conv_out with the lazily normalised source, its input gradient, the norm backward of unpack1.norm in place,
//             the transposed layer's dW and input gradient -> d(x2), onto which k_enc_pool2_bwd_acc adds d(p) (d_x_hd NULL:
//             k_enc_pool2_bwd writes d(x2); d_out NULL: nothing of the pooled branch runs).  Head: conv2, the norm backward of bn1 (x = t0)
//             in place, the stem's dW and db.
// Gradient buffers: two per resolution, alternating (a step reads one and writes the other).  Every fan-in is one fp32 add of two finished
// values.  No atomics: equal bits from run to run, and an image's results do not depend on its batch.
namespace hgf {
struct Block {
    kpn_conv_block_desc d;
    blk::Plan p;
    int t0;                         // index of the block's first tensor (9 or 12 of them)
    size_t x, y, st;                // offsets (floats) in `state`: input, output (not b3: the workspace), the block's own state
    size_t packed[4];               // offsets (floats) in the packed weights
};
struct Conv {
    enc::Layer e;
    int tw, tb;                     // tensor indices of weight and bias (-1: none)
    size_t packed;
};
struct Norm {
    int C, G, HW, nchunks, tw;      // tw: tensor index of the weight; the bias follows
    int64_t pd;
    size_t ss, mr;                  // offsets (floats) in `state`
};
struct Level {
    int h, w;                       // the level's grid (its input and output)
    int b1, b2, b3, plus;           // block indices; plus = -1 but at the innermost level
    size_t inp, hg, low, low1, low2;
};
struct Plan {
    std::vector<Block> B;           // conv2, conv3, conv4, the HourGlass in dataflow order, top_m_0
    std::vector<Level> lv;          // outermost first
    int top;
    Conv stem, un, co, cl, l0;
    Norm bn1, unn, bne;
    int N, h1, w1, h2, w2, ntensors;
    size_t s_t0, s_a1, s_x2, s_d, s_p, s_x3, s_x4, s_top, s_cl;
    std::vector<size_t> numel;      // of every tensor, in tensor order
    size_t packed_floats, state_floats;
    size_t f_blk, f_low3, f_stats, f_conv;                                              // the forward's workspace (byte offsets)
    size_t b_blk, b_r0, b_r1[2], b_conv, b_wg, b_stats, b_coef, b_db;                    // the backward's
    std::vector<size_t> b_g[2];                                                          // per resolution from (h2, w2) down
    size_t bytes;
};
const char* weight_error(const kpn_hg_filter_desc* d) {
    if (!d) return "desc is null";
    if (d->in_ch < 1 || d->in_ch > 4) return "in_ch must be in 1 .. 4 (the stem reads an NCHW image)";
    if (d->depth < 1 || d->depth > 8) return "depth must be in 1 .. 8";
    if (!blk::pow2_width(d->c_stem)) return "c_stem must be a power of two in 4 .. 1024";
    if (!blk::pow2_width(d->c_hd)) return "c_hd must be a power of two in 4 .. 1024";
    if (d->out_ch < 4 || d->out_ch % 4 || d->out_ch > 1024) return "out_ch must be a multiple of 4 in 4 .. 1024";
    if (d->out_ch_hd < 4 || d->out_ch_hd % 4 || d->out_ch_hd > 1024) return "out_ch_hd must be a multiple of 4 in 4 .. 1024";
    const int w[5] = {d->c_stem, d->c2, d->c3, d->c4, d->c4};
    static const char* const what[4] = {"c_stem -> c2 (conv2): ", "c2 -> c3 (conv3): ", "c3 -> c4 (conv4): ", "c4 -> c4 (the HourGlass and top_m_0): "};
    static std::string msg;
    for (int i = 0; i < 4; ++i) {
        const kpn_conv_block_desc b{1, 1, 1, w[i], w[i + 1], 1e-5f};
        if (const char* e = blk::desc_error(&b)) { msg = std::string("the ConvBlock ") + what[i] + e; return msg.c_str(); }
    }
    return nullptr;
}
const char* desc_error(const kpn_hg_filter_desc* d) {
    if (const char* e = weight_error(d)) return e;
    if (d->N < 1 || d->H < 1 || d->W < 1) return "N, H, W must be positive";
    if (d->N > 65535) return "N must be at most 65535 (one grid row per image)";
    const int f = 1 << (d->depth + 1);
    if (d->H % 2 || d->W % 2 || (d->H / 2) % f || (d->W / 2) % f) return "H / 2 and W / 2 must be divisible by 2^(depth + 1) (H, W even)";
    const int64_t P0 = (int64_t)d->N * d->H * d->W;
    if ((int64_t)d->H * d->W >= (1ll << 31) || P0 * std::max(d->c_hd, d->out_ch_hd) >= (1ll << 31) ||
        P0 / 4 * std::max(d->c_stem, d->c2) >= (1ll << 31) || P0 / 16 * std::max(std::max(d->c2, d->c3), std::max(d->c4, d->out_ch)) >= (1ll << 31))
        return "N * H * W * channels must stay below 2^31 (for every layer's input and output)";
    if (!(d->eps > 0.0f)) return "eps must be positive";
    return nullptr;
}
inline int block_tensors(const Block& b) { return 3 * b.p.nlegs; }
Plan plan(const kpn_hg_filter_desc* d, int N, int H, int W) {
    Plan p{};
    p.N = N; p.h1 = H / 2; p.w1 = W / 2; p.h2 = H / 4; p.w2 = W / 4;
    const int c4 = d->c4;
    auto add_block = [&](int cin, int cout, int h, int w) {
        Block b{};
        b.d = kpn_conv_block_desc{N, h, w, cin, cout, d->eps};
        b.p = blk::plan(&b.d);
        p.B.push_back(b);
        return (int)p.B.size() - 1;
    };
    auto norm = [&](Norm& n, int C, int HW) { n.C = C; n.G = std::min(32, C); n.HW = HW; n.nchunks = enc::stats_chunks(N, HW, C, &n.pd); };
    // ---- the layers
    p.stem.e = enc::layer(enc::LayerSpec{d->in_ch, d->c_stem, 7, 2, 3, 0, 0, 1}, N, H, W);
    norm(p.bn1, d->c_stem, p.h1 * p.w1);
    add_block(d->c_stem, d->c2, p.h1, p.w1);
    p.un.e = enc::layer(enc::LayerSpec{d->c2, d->c_hd, 3, 2, 1, 0, 1, 0}, N, p.h1, p.w1);
    norm(p.unn, d->c_hd, H * W);
    p.co.e = enc::layer(enc::LayerSpec{d->c_hd, d->out_ch_hd, 5, 1, 2, 0, 0, 0}, N, H, W);
    add_block(d->c2, d->c3, p.h2, p.w2);
    add_block(d->c3, c4, p.h2, p.w2);
    for (int k = 0, h = p.h2, w = p.w2; k < d->depth; ++k, h /= 2, w /= 2) {
        Level l{};
        l.h = h; l.w = w; l.plus = -1;
        l.b1 = add_block(c4, c4, h, w);
        l.b2 = add_block(c4, c4, h / 2, w / 2);
        p.lv.push_back(l);
    }
    p.lv.back().plus = add_block(c4, c4, p.lv.back().h / 2, p.lv.back().w / 2);
    for (int k = d->depth - 1; k >= 0; --k) p.lv[k].b3 = add_block(c4, c4, p.lv[k].h / 2, p.lv[k].w / 2);
    p.top = add_block(c4, c4, p.h2, p.w2);
    p.cl.e = enc::layer(enc::LayerSpec{c4, c4, 1, 1, 0, 0, 0, 0}, N, p.h2, p.w2);
    norm(p.bne, c4, p.h2 * p.w2);
    p.l0.e = enc::layer(enc::LayerSpec{c4, d->out_ch, 1, 1, 0, 0, 0, 0}, N, p.h2, p.w2);
    // ---- tensor indices and packed offsets, in tensor order
    int t = 0;
    size_t pk = 0;
    auto conv_t = [&](Conv& c, bool bias) {
        const enc::LayerSpec& s = c.e.s;
        c.tw = t++; p.numel.push_back((size_t)s.cout * s.cin * s.k * s.k);
        c.tb = bias ? t++ : -1;
        if (bias) p.numel.push_back((size_t)s.cout);
        c.packed = pk; pk += c.e.packed_floats;
    };
    auto norm_t = [&](Norm& n) { n.tw = t; t += 2; p.numel.insert(p.numel.end(), 2, (size_t)n.C); };
    conv_t(p.stem, true); norm_t(p.bn1);
    for (Block& b : p.B) {
        b.t0 = t; t += block_tensors(b);
        for (int i = 0; i < b.p.nlegs; ++i) {
            const blk::Leg& l = b.p.leg[i];
            b.packed[i] = pk; pk += l.e.packed_floats;
            p.numel.insert(p.numel.end(), 2, (size_t)l.cin);
            p.numel.push_back((size_t)l.cout * l.cin * l.e.s.k * l.e.s.k);
        }
    }
    conv_t(p.un, false); norm_t(p.unn); conv_t(p.co, true); conv_t(p.cl, true); norm_t(p.bne); conv_t(p.l0, true);
    p.ntensors = t; p.packed_floats = pk;
    // ---- `state`, in dataflow order
    size_t st = 0;
    auto take = [&](size_t n) { const size_t o = st; st += n; return o; };
    auto take_norm = [&](Norm& n) { n.ss = take((size_t)2 * N * n.C); n.mr = take((size_t)2 * N * n.G); };
    auto block_at = [&](int i, size_t x, bool keep_y) {
        Block& b = p.B[i];
        b.x = x; b.st = take(b.p.state_floats);
        b.y = keep_y ? take((size_t)b.p.P * b.d.cout) : 0;
        return b.y;
    };
    const size_t P1 = (size_t)N * p.h1 * p.w1, P2 = (size_t)N * p.h2 * p.w2;
    p.s_t0 = take(P1 * d->c_stem); take_norm(p.bn1); p.s_a1 = take(P1 * d->c_stem);
    p.s_x2 = block_at(0, p.s_a1, true);
    p.s_d = take((size_t)N * H * W * d->c_hd); take_norm(p.unn);
    p.s_p = take(P2 * d->c2);
    p.s_x3 = block_at(1, p.s_p, true);
    p.s_x4 = block_at(2, p.s_x3, true);
    size_t inp = p.s_x4;
    for (Level& l : p.lv) {
        l.inp = inp;
        l.hg = block_at(l.b1, inp, true);
        l.low = take((size_t)N * (l.h / 2) * (l.w / 2) * c4);
        l.low1 = block_at(l.b2, l.low, true);
        inp = l.low1;
    }
    for (int k = d->depth - 1; k >= 0; --k) {
        Level& l = p.lv[k];
        l.low2 = l.plus >= 0 ? block_at(l.plus, l.low1, true) : p.lv[k + 1].hg;
        block_at(l.b3, l.low2, false);
    }
    p.s_top = block_at(p.top, p.lv[0].hg, true);
    p.s_cl = take(P2 * c4); take_norm(p.bne);
    p.state_floats = st;
    // ---- the workspace: the forward and the backward never run at once on it: the larger of the two
    size_t blkws = 0;
    for (const Block& b : p.B) blkws = std::max(blkws, b.p.bytes);
    const Conv* convs[5] = {&p.stem, &p.un, &p.co, &p.cl, &p.l0};
    size_t fconv = 0, bconv = 0, wg = 0, db = 0, stat = 0, coef = 0;
    for (const Conv* c : convs) {
        fconv = std::max(fconv, (size_t)c->e.fwd.partial * sizeof(float));
        bconv = std::max(bconv, (size_t)c->e.dx.partial * sizeof(float));
        wg = std::max(wg, (size_t)c->e.wgp.partial * sizeof(float));
        if (c->tb >= 0) db = std::max(db, (size_t)enc::dbias_chunks(c->e.My) * c->e.s.cout * sizeof(double));
    }
    for (const Norm* n : {&p.bn1, &p.unn, &p.bne}) {
        stat = std::max(stat, (size_t)n->pd * sizeof(double));
        coef = std::max(coef, (size_t)3 * N * n->C * sizeof(float));
    }
    Carver f, b;
    p.f_blk = f.take(blkws);
    p.f_low3 = f.take(P2 / 4 * c4 * sizeof(float));
    p.f_stats = f.take(stat);
    p.f_conv = f.take(fconv);
    // The backward runs in three phases: the pooled branch (blocks on (h2, w2) and below, the buffers b_g), the hd branch (no block: the
    // gradient of the unpack1.conv output, b_r0, and d(x2), b_r1[0]) and the head (the conv2 block, b_r1).  Of the first phase only d(p),
    // in b_g[1][0], is read later, so b_r0 lies over the blocks' workspace and the other b_g buffers, which the second phase does not use
    p.b_blk = b.take(blkws);
    for (int k = 0; k <= d->depth; ++k)
        for (int i = 0; i < 2; ++i)
            if (k || !i) p.b_g[i].push_back(b.take((P2 >> (2 * k)) * (k ? c4 : std::max(std::max(d->c2, d->c3), c4)) * sizeof(float)));
    p.b_r0 = p.b_blk;
    const size_t r0 = (size_t)N * H * W * d->c_hd * sizeof(float);
    if (b.o - p.b_blk < r0) b.take(r0 - (b.o - p.b_blk));
    p.b_g[1].insert(p.b_g[1].begin(), b.take(P2 * std::max(std::max(d->c2, d->c3), c4) * sizeof(float)));
    p.b_r1[0] = b.take(P1 * d->c2 * sizeof(float));
    p.b_r1[1] = b.take(P1 * d->c_stem * sizeof(float));
    p.b_conv = b.take(bconv);
    p.b_wg = b.take(wg);
    p.b_stats = b.take(stat);
    p.b_coef = b.take(coef);
    p.b_db = b.take(db);
    p.bytes = std::max<size_t>(std::max(f.o, b.o), 256);
    return p;
}
inline Plan plan(const kpn_hg_filter_desc* d) { return plan(d, d->N, d->H, d->W); }
// the smallest input the descriptor's depth admits: what the packed weights and the tensor count are planned on
inline Plan weight_plan(const kpn_hg_filter_desc* d) { return plan(d, 1, 4 << d->depth, 4 << d->depth); }
inline kpn_conv_block_params block_params(const Plan& p, const Block& b, const kpn_hg_filter_params* pr) {
    kpn_conv_block_params q{};
    for (int i = 0; i < b.p.nlegs; ++i) {
        q.gamma[i] = pr->tensors[b.t0 + 3 * i];
        q.beta[i] = pr->tensors[b.t0 + 3 * i + 1];
        q.packed[i] = pr->packed + b.packed[i];
    }
    return q;
}
// which tensors the forward and the backward read: every norm parameter and every bias, not the plain convolution weights
inline bool reads_tensor(const Plan& p, int t) {
    for (const Conv* c : {&p.stem, &p.un, &p.co, &p.cl, &p.l0})
        if (t == c->tw) return false;
    for (const Block& b : p.B)
        if (t >= b.t0 && t < b.t0 + block_tensors(b) && (t - b.t0) % 3 == 2) return false;
    return true;
}
}  // namespace hgf

#define KPN_HGF_REQUIRE_DESC(desc) do { if (const char* e_ = hgf::desc_error(desc)) return fail(KPN_EINVAL, std::string("kpn_hg_filter_desc: ") + e_); } while (0)

extern "C" int32_t kpn_hg_filter_tensors(const kpn_hg_filter_desc* desc) {
    return hgf::weight_error(desc) ? 0 : hgf::weight_plan(desc).ntensors;
}
extern "C" size_t kpn_hg_filter_workspace_bytes(const kpn_hg_filter_desc* desc) {
    return hgf::desc_error(desc) ? 0 : hgf::plan(desc).bytes;
}
extern "C" size_t kpn_hg_filter_state_floats(const kpn_hg_filter_desc* desc) {
    return hgf::desc_error(desc) ? 0 : hgf::plan(desc).state_floats;
}
extern "C" size_t kpn_hg_filter_packed_floats(const kpn_hg_filter_desc* desc) {
    return hgf::weight_error(desc) ? 0 : hgf::weight_plan(desc).packed_floats;
}
extern "C" int kpn_hg_filter_pack_device(const kpn_hg_filter_desc* desc, const float* const* tensors, float* packed, void* stream) {
    if (const char* e = hgf::weight_error(desc)) return fail(KPN_EINVAL, std::string("kpn_hg_filter_desc: ") + e);
    KPN_REQUIRE(tensors && packed, "null pointer");
    KPN_REQUIRE(((uintptr_t)packed & 15) == 0, "packed must be 16-byte aligned");
    const hgf::Plan p = hgf::weight_plan(desc);
    const hgf::Conv* convs[5] = {&p.stem, &p.un, &p.co, &p.cl, &p.l0};
    for (const hgf::Conv* c : convs) KPN_REQUIRE(tensors[c->tw], "tensors: the weight of a convolution is null");
    for (const hgf::Block& b : p.B)
        for (int i = 0; i < b.p.nlegs; ++i) KPN_REQUIRE(tensors[b.t0 + 3 * i + 2], "tensors: the weight of a block's convolution is null");
    for (const hgf::Conv* c : convs) enc::layer_pack(c->e, tensors[c->tw], packed + c->packed, stream);
    for (const hgf::Block& b : p.B)
        for (int i = 0; i < b.p.nlegs; ++i) enc::layer_pack(b.p.leg[i].e, tensors[b.t0 + 3 * i + 2], packed + b.packed[i], stream);
    return check_launch("kpn_hg_filter_pack_device");
}
extern "C" int kpn_hg_filter_forward(const kpn_hg_filter_desc* desc, const float* x, const kpn_hg_filter_params* params, float* out,
                                     float* x_hd, float* state, void* workspace, size_t workspace_bytes, void* stream) {
    KPN_HGF_REQUIRE_DESC(desc);
    KPN_REQUIRE(x && params && out && x_hd && state && workspace, "null pointer");
    KPN_REQUIRE(params->tensors && params->packed, "params: tensors / packed is null");
    const hgf::Plan p = hgf::plan(desc);
    const float* const* T = params->tensors;
    for (int t = 0; t < p.ntensors; ++t)
        if (hgf::reads_tensor(p, t)) {
            KPN_REQUIRE(T[t], "params: a norm parameter or a bias is null");
            KPN_REQUIRE(((uintptr_t)T[t] & 15) == 0, "params: every norm parameter and bias must be 16-byte aligned");
        }
    KPN_REQUIRE(enc::aligned16({params->packed, out, x_hd, state, workspace}), "packed / out / x_hd / state / workspace must be 16-byte aligned");
    KPN_REQUIRE(workspace_bytes >= p.bytes, "workspace too small (kpn_hg_filter_workspace_bytes)");
    char* ws = static_cast<char*>(workspace);
    double* stat = reinterpret_cast<double*>(ws + p.f_stats);
    float* part = reinterpret_cast<float*>(ws + p.f_conv);
    float* low3 = reinterpret_cast<float*>(ws + p.f_low3);
    const int N = desc->N, c4 = desc->c4;
    auto conv = [&](const hgf::Conv& c, const float* src, const float* ss, float* dst) {
        enc::layer_forward(c.e, src, c.e.s.cin, ss, params->packed + c.packed, c.tb >= 0 ? T[c.tb] : nullptr, dst, c.e.s.cout, nullptr, 0, part, stream);
    };
    auto stats = [&](const hgf::Norm& n, const float* src) {
        kpn_enc_stats_args a{};
        a.src = src; a.cs = n.C; a.C = n.C; a.HW = n.HW; a.nchunks = n.nchunks; a.nimg = N;
        a.partial = stat;
        a.G = n.G; a.gamma = T[n.tw]; a.beta = T[n.tw + 1]; a.eps = desc->eps;
        a.ss = state + n.ss; a.mr = state + n.mr;
        enc::launch_stats(a, stream);
    };
    auto block = [&](int i, float* y) {
        const hgf::Block& b = p.B[i];
        const kpn_conv_block_params q = hgf::block_params(p, b, params);
        blk::forward(b.p, &b.d, state + b.x, &q, y ? y : state + b.y, state + b.st, ws + p.f_blk, stream);
    };
    conv(p.stem, x, nullptr, state + p.s_t0);
    stats(p.bn1, state + p.s_t0);
    enc::launch_affine(state + p.s_t0, state + p.bn1.ss, 1, nullptr, state + p.s_a1, N, p.bn1.HW, p.bn1.C, stream);
    block(0, nullptr);
    conv(p.un, state + p.s_x2, nullptr, state + p.s_d);
    stats(p.unn, state + p.s_d);
    conv(p.co, state + p.s_d, state + p.unn.ss, x_hd);
    enc::launch_pool2(state + p.s_x2, state + p.s_p, N, p.h2, p.w2, desc->c2, stream);
    block(1, nullptr);
    block(2, nullptr);
    for (const hgf::Level& l : p.lv) {
        block(l.b1, nullptr);
        enc::launch_pool2(state + l.inp, state + l.low, N, l.h / 2, l.w / 2, c4, stream);
        block(l.b2, nullptr);
    }
    for (int k = desc->depth - 1; k >= 0; --k) {
        const hgf::Level& l = p.lv[k];
        if (l.plus >= 0) block(l.plus, nullptr);
        block(l.b3, low3);
        enc::launch_upadd(low3, state + l.hg, state + l.hg, N, l.h / 2, l.w / 2, c4, stream);
    }
    block(p.top, nullptr);
    conv(p.cl, state + p.s_top, nullptr, state + p.s_cl);
    stats(p.bne, state + p.s_cl);
    conv(p.l0, state + p.s_cl, state + p.bne.ss, out);
    return check_launch("kpn_hg_filter_forward");
}
extern "C" int kpn_hg_filter_backward(const kpn_hg_filter_desc* desc, const float* x, const float* d_out, const float* d_x_hd,
                                      const kpn_hg_filter_params* params, const float* state, const kpn_hg_filter_grads* grads,
                                      void* workspace, size_t workspace_bytes, void* stream) {
    KPN_HGF_REQUIRE_DESC(desc);
    KPN_REQUIRE(d_out || d_x_hd, "d_out and d_x_hd are both null (at least one output gradient must be given)");
    KPN_REQUIRE(x && params && state && grads && workspace, "null pointer");
    KPN_REQUIRE(params->tensors && params->packed && grads->tensors, "params / grads: tensors / packed is null");
    const hgf::Plan p = hgf::plan(desc);
    const float* const* T = params->tensors;
    float* const* D = grads->tensors;
    for (int t = 0; t < p.ntensors; ++t) {
        if (hgf::reads_tensor(p, t)) {
            KPN_REQUIRE(T[t], "params: a norm parameter or a bias is null");
            KPN_REQUIRE(((uintptr_t)T[t] & 15) == 0, "params: every norm parameter and bias must be 16-byte aligned");
        }
        KPN_REQUIRE(((uintptr_t)D[t] & 15) == 0, "grads: every gradient must be 16-byte aligned");
    }
    KPN_REQUIRE(enc::aligned16({d_out, d_x_hd, params->packed, state, workspace}), "d_out / d_x_hd / packed / state / workspace must be 16-byte aligned");
    KPN_REQUIRE(workspace_bytes >= p.bytes, "workspace too small (kpn_hg_filter_workspace_bytes)");
    char* ws = static_cast<char*>(workspace);
    auto fbuf = [&](size_t off) { return reinterpret_cast<float*>(ws + off); };
    float* cpart = fbuf(p.b_conv);
    float* wpart = fbuf(p.b_wg);
    double* stat = reinterpret_cast<double*>(ws + p.b_stats);
    double* dbp = reinterpret_cast<double*>(ws + p.b_db);
    float* coef = fbuf(p.b_coef);
    const int N = desc->N, c4 = desc->c4, depth = desc->depth;
    // ---- what is wanted, and with it how far down each branch has to walk
    auto want_conv = [&](const hgf::Conv& c) { return D[c.tw] || (c.tb >= 0 && D[c.tb]); };
    auto want_norm = [&](const hgf::Norm& n) { return D[n.tw] || D[n.tw + 1]; };
    auto want_block = [&](int i) {
        const hgf::Block& b = p.B[i];
        for (int k = 0; k < hgf::block_tensors(b); ++k)
            if (D[b.t0 + k]) return true;
        return false;
    };
    const bool need_t0 = want_conv(p.stem);                        // a gradient of the stem output is needed, ...
    const bool need_a1 = need_t0 || want_norm(p.bn1);
    const bool need_x2 = need_a1 || want_block(0);                // ... of the conv2 output: both branches walk all the way down
    // ---- the layers
    auto wgrad = [&](const hgf::Conv& c, const float* src, const float* ss, const float* R) {
        if (D[c.tw]) enc::layer_wgrad(c.e, src, c.e.s.cin, ss, R, c.e.s.cout, wpart, D[c.tw], stream);
    };
    auto dbias = [&](const hgf::Conv& c, const float* R) {
        if (c.tb >= 0 && D[c.tb]) enc::launch_dbias(R, c.e.My, c.e.s.cout, dbp, D[c.tb], stream);
    };
    auto dgrad = [&](const hgf::Conv& c, const float* R, float* dn) {
        enc::layer_dgrad(c.e, R, c.e.s.cout, params->packed + c.packed, dn, c.e.s.cin, nullptr, 0, cpart, stream);
    };
    // the gradient of norm n (+ ReLU) for the gradient g of its output: dx (may be g, or NULL), dgamma, dbeta
    auto norm_bwd = [&](const hgf::Norm& n, const float* xs, const float* g, float* dx) {
        kpn_enc_norm_bwd_args a{};
        a.x = xs; a.x_cs = n.C; a.dy = g; a.ss = state + n.ss; a.mr = state + n.mr; a.gamma = T[n.tw];
        a.relu = 1; a.C = n.C; a.HW = n.HW; a.nchunks = n.nchunks; a.nimg = N; a.G = n.G;
        a.partial = stat; a.coef = dx ? coef : nullptr;
        a.dx = dx; a.dgamma = D[n.tw]; a.dbeta = D[n.tw + 1];
        enc::launch_norm_bwd(a, stream);
    };
    auto block = [&](int i, const float* dy, float* dx) {
        const hgf::Block& b = p.B[i];
        const kpn_conv_block_params q = hgf::block_params(p, b, params);
        kpn_conv_block_grads g{};
        for (int k = 0; k < b.p.nlegs; ++k) { g.dgamma[k] = D[b.t0 + 3 * k]; g.dbeta[k] = D[b.t0 + 3 * k + 1]; g.dw[k] = D[b.t0 + 3 * k + 2]; }
        blk::backward(b.p, &b.d, state + b.x, dy, &q, state + b.st, dx, &g, ws + p.b_blk, stream);
    };
    auto pool_bwd = [&](const float* g_low, float* dst, int h, int w, int C, bool acc) {      // (h, w): the low grid
        const int64_t n4 = (int64_t)N * h * w * C;                                            // float4s of the high tensor
        if (acc) KPN_LAUNCH(k_enc_pool2_bwd_acc, enc::grid4(n4), dim3(256), stream, g_low, dst, N, h, w, C);
        else KPN_LAUNCH(k_enc_pool2_bwd, enc::grid4(n4), dim3(256), stream, g_low, dst, N, h, w, C);
    };
    // a wanted gradient that no given output gradient reaches - the hd branch's parameters without d_x_hd, everything behind the pool
    // without d_out - is exactly zero: zeros are written, nothing is launched for it
    {
        hipError_t zero_err = hipSuccess;
        for (int t = 0; t < p.ntensors; ++t) {
            const bool hd = t >= p.un.tw && t <= p.co.tb;
            const bool pooled = (t >= p.B[1].t0 && t < p.un.tw) || t > p.co.tb;
            if (!D[t] || !((hd && !d_x_hd) || (pooled && !d_out))) continue;
            const hipError_t e = hipMemsetAsync(D[t], 0, p.numel[t] * sizeof(float), (hipStream_t)stream);
            if (e != hipSuccess && zero_err == hipSuccess) zero_err = e;
        }
        if (zero_err != hipSuccess) return fail(KPN_ELAUNCH, std::string("kpn_hg_filter_backward: zeroing a gradient failed: ") + hipGetErrorString(zero_err));
    }
    const float* dp = nullptr;                                     // d(p): the gradient of the pooled conv2 output, if it was walked to
    if (d_out) {
        // per level, from the outermost: need_in - its input gradient is needed; need_low1 - the gradient of its b2 output; below - that
        // of its b3 input (something in the next level or in b2_plus, or need_low1); any - the level has to be entered at all
        std::vector<char> any(depth, 0), need_in(depth, 0), need_low1(depth, 0), below(depth, 0);
        const bool need_x4 = need_x2 || want_block(1) || want_block(2);
        for (int k = 0; k < depth; ++k) {
            need_in[k] = k ? need_low1[k - 1] : need_x4;
            need_low1[k] = need_in[k] || want_block(p.lv[k].b2);
        }
        for (int k = depth - 1; k >= 0; --k) {
            const hgf::Level& l = p.lv[k];
            below[k] = k == depth - 1 ? (need_low1[k] || want_block(l.plus)) : any[k + 1];
            any[k] = below[k] || want_block(l.b3) || want_block(l.b1) || need_in[k];
        }
        const bool need_hg = any[0];
        const bool need_top = need_hg || want_block(p.top);
        const bool need_cl = need_top || want_conv(p.cl);
        float* A = fbuf(p.b_g[0][0]);
        float* Bf = fbuf(p.b_g[1][0]);
        // the tail: l0, bn_end0, conv_last0, top_m_0
        wgrad(p.l0, state + p.s_cl, state + p.bne.ss, d_out);
        dbias(p.l0, d_out);
        if (need_cl || want_norm(p.bne)) {
            dgrad(p.l0, d_out, A);
            norm_bwd(p.bne, state + p.s_cl, A, need_cl ? A : nullptr);
        }
        if (need_cl) {
            wgrad(p.cl, state + p.s_top, nullptr, A);
            dbias(p.cl, A);
            if (need_top) dgrad(p.cl, A, Bf);
        }
        if (need_top) block(p.top, Bf, need_hg ? A : nullptr);
        // the HourGlass: level k reads its output gradient from dY[k] and writes its input gradient to dIn[k], the other buffer of its
        // resolution; t1 = dIn[k + 1] holds d(low3) and then d(low1), t2 = dY[k + 1] holds d(low2) and then g_low
        if (need_hg) {
            std::vector<float*> dY(depth + 1), dIn(depth + 1);
            dY[0] = A; dIn[0] = Bf;
            for (int k = 0; k < depth; ++k) { dIn[k + 1] = fbuf(p.b_g[0][k + 1]); dY[k + 1] = fbuf(p.b_g[1][k + 1]); }
            int last = 0;                                          // the innermost level entered
            for (int k = 0; k < depth; ++k) {                      // inwards: up2_bwd, b3, then the next level or b2_plus
                const hgf::Level& l = p.lv[k];
                last = k;
                if (below[k] || want_block(l.b3)) {
                    KPN_LAUNCH(k_enc_up2_bwd, enc::grid4((int64_t)N * (l.h / 2) * (l.w / 2) * c4 / 4), dim3(256), stream, (const float*)dY[k],
                               dIn[k + 1], N, l.h / 2, l.w / 2, c4);
                    block(l.b3, dIn[k + 1], below[k] ? dY[k + 1] : nullptr);
                }
                if (!below[k]) break;
                if (k == depth - 1) block(l.plus, dY[k + 1], need_low1[k] ? dIn[k + 1] : nullptr);
            }
            for (int k = last; k >= 0; --k) {                      // outwards: b2 -> g_low, b1 -> the input gradient, the fan-in
                const hgf::Level& l = p.lv[k];
                if (below[k] && need_low1[k]) block(l.b2, dIn[k + 1], need_in[k] ? dY[k + 1] : nullptr);
                if (want_block(l.b1) || need_in[k]) block(l.b1, dY[k], need_in[k] ? dIn[k] : nullptr);
                if (need_in[k]) pool_bwd(dY[k + 1], dIn[k], l.h / 2, l.w / 2, c4, true);
            }
        }
        if (need_x4) {                                             // d(x4) in Bf
            block(2, Bf, (need_x2 || want_block(1)) ? A : nullptr);
            if (need_x2 || want_block(1)) block(1, A, need_x2 ? Bf : nullptr);
            if (need_x2) dp = Bf;
        }
    }
    float* X0 = fbuf(p.b_r1[0]);
    float* X1 = fbuf(p.b_r1[1]);
    bool have_x2 = false;                                          // d(x2) in X0
    if (d_x_hd) {
        const bool need_d = need_x2 || D[p.un.tw];                 // the gradient of the unpack1.conv output
        wgrad(p.co, state + p.s_d, state + p.unn.ss, d_x_hd);
        dbias(p.co, d_x_hd);
        if (need_d || want_norm(p.unn)) {
            float* gD = fbuf(p.b_r0);
            dgrad(p.co, d_x_hd, gD);
            norm_bwd(p.unn, state + p.s_d, gD, need_d ? gD : nullptr);
            if (need_d) {
                wgrad(p.un, state + p.s_x2, nullptr, gD);
                if (need_x2) { dgrad(p.un, gD, X0); have_x2 = true; }
            }
        }
    }
    if (need_x2) {
        if (dp) pool_bwd(dp, X0, p.h2, p.w2, desc->c2, have_x2);
        // the head: conv2, bn1, the stem
        block(0, X0, need_a1 ? X1 : nullptr);
        if (need_a1) {
            norm_bwd(p.bn1, state + p.s_t0, X1, need_t0 ? X1 : nullptr);
            if (need_t0) {
                wgrad(p.stem, x, nullptr, X1);
                dbias(p.stem, X1);
            }
        }
    }
    return check_launch("kpn_hg_filter_backward");
}

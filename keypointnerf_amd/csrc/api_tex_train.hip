// ---------------------------------------------------------------------------------------------
// A whole ResBlkEncoder (reference src/utils.py:199-259, norm = "instance") as one differentiable operator: the encoder walk's fused
// forward (enc::tex_walk in api_encoders.hip, with stem_plain = 1 and ds = 0) with what a backward needs kept, and a backward fused in the
// same way.  Kernels: encoder_kernels.hip, launched through the launch layer at the head of api_encoders.hip, so this operator, the walk
// and the single layers (api_reppad.hip, api_strided.hip, api_norm.hip) share tiles, split K, weight-gradient ranges and chunk counts -
// and with them the order of every sum.
//
// Layers, in module order: the 7x7 stem, n_down stride-2 convolutions, two 3x3 convolutions per ResBlk, n_up transposed convolutions,
// the 7x7 output layer.  Every layer but the last has an InstanceNorm2d behind it (statistics only: scale / shift `ss`, mean / rstd `mr`).
//   forward   c_0 = rp7(x);  c_i = s2conv(relu(fma(c_{i-1}, ss_{i-1})))  (the norm and the ReLU in the A loads);
//             a_0 = relu(fma(c_down, ss_down))                                  (k_enc_affine: the first residual needs the tensor)
//             per ResBlk: c1 = rp3(a), c2 = rp3(relu(fma(c1, ss1))), a' = fma(c2, ss2) + a   (k_enc_affine with res)
//             c = deconv(a_last), then deconv(relu(fma(c, ss))) from the second transposed layer on;  y = rp7(relu(fma(c, ss))) + bias.
//             No normalised tensor of a non-residual layer and no padded tensor exists.
//   backward  the layers in reverse.  With R = dL/dc of a layer and its source s, either (c_prev, ss_prev) or a materialised a_k:
//               dW = wgrad(A = act(s) in the loads, R)   (transposed layers: A = R with stride 2, rhs = act(s) through rhs_ss)
//               dn = the layer kind's input gradient of R (rp adjoint / DECONV GEMM / stride-2 GEMM)
//               R_prev = norm backward(c_prev, dn, relu = 1), in place over dn
//             a ResBlk with G = dL/da_k: dc2 = norm backward(c2, G, relu = 0); dW2; dn1 = rp-adjoint(dc2); dc1 = norm backward(c1, dn1,
//             relu = 1); dW1 = wgrad(a_{k-1}, dc1); dL/da_{k-1} = rp-adjoint(dc1) + G (the res epilogue of the GEMM or of its combine).
//             The stem gets dW only.  The bias of a layer in front of an InstanceNorm2d has the gradient zero (IN(c + b) = IN(c)): zeros
//             are written, nothing is reduced; the output layer's db is a real sum.
// Every sum runs in the fixed order its kernel has: no atomics, equal bits from run to run, and an image's y does not depend on its batch.
namespace rte {
enum Kind { STEM = 0, DOWN = 1, RES = 2, UP = 3, OUT = 4 };
// what the packed weights depend on
const char* weight_error(const kpn_res_encoder_desc* d) {
    if (!d) return "desc is null";
    if (d->in_ch < 1 || d->in_ch > 4) return "in_ch must be in 1 .. 4 (the stem reads an NCHW image)";
    if (d->ngf < 4 || (d->ngf & (d->ngf - 1))) return "ngf must be a power of two, at least 4";
    if (d->n_down < 0 || d->n_down > 8 || ((int64_t)d->ngf << d->n_down) > 1024) return "ngf << n_down must be at most 1024";
    if (d->n_up < 1) return "n_up must be at least 1 (n_upsample = 0 drops the output layer)";
    if (d->n_up > d->n_down) return "n_up must be at most n_down";
    if (d->n_blocks < 0 || d->n_blocks > 64) return "n_blocks must be in 0 .. 64";
    if (d->out_ch < 4 || d->out_ch % 4 || d->out_ch > 1024) return "out_ch must be a multiple of 4 in 4 .. 1024";
    return nullptr;
}
const char* desc_error(const kpn_res_encoder_desc* d) {
    if (const char* e = weight_error(d)) return e;
    if (d->N < 1 || d->H < 1 || d->W < 1) return "N, H, W must be positive";
    if (d->N > 65535) return "N must be at most 65535 (one grid row per image)";
    const int f = 1 << d->n_down;
    if (d->H % f || d->W % f) return "H and W must be divisible by 2^n_down";
    // the largest tensors: the stem's output, and y and the last transposed layer's output on the output grid
    const int64_t P = (int64_t)d->N * d->H * d->W, Po = P >> (2 * (d->n_down - d->n_up));
    if ((int64_t)d->H * d->W >= (1ll << 31) || P * d->ngf >= (1ll << 31) || Po * std::max(d->out_ch, (d->ngf << d->n_down) >> d->n_up) >= (1ll << 31))
        return "N * H * W * channels must stay below 2^31 (for every layer's input and output)";
    if (!(d->eps > 0.0f)) return "eps must be positive";
    return nullptr;
}
struct Layer {
    int kind;
    enc::Layer e;                   // the layer itself (api_layer.hip), as the single layers make it
    size_t packed;                  // offset (floats) in the packed weights: each layer as its own packer writes it
    int nchunks;                    // of the norm behind the layer (not OUT)
    size_t c, ss, mr;               // offsets (floats) in `state`: the layer's output and its norm's statistics (not OUT)
    size_t out_floats;
};
struct Plan {
    std::vector<Layer> L;
    std::vector<size_t> a;          // offsets (floats) in `state` of a_0 .. a_{n_blocks}
    int Hb, Wb, Cb;                 // the ResBlks' grid and width
    size_t packed_floats, state_floats;
    size_t f_stats, f_conv;                                    // the forward's workspace (byte offsets)
    size_t b_buf[3], b_conv, b_wg, b_stats, b_coef, b_db;      // the backward's
    size_t bytes;
};
Plan plan(const kpn_res_encoder_desc* d, int N, int H, int W) {
    Plan p{};
    auto add = [&](int kind, int cin, int cout, int k, int Hi, int Wi) {
        Layer l{};
        l.kind = kind;
        const bool s2 = kind == DOWN || kind == UP;                // zero pad; the others pad by replication
        l.e = enc::layer(enc::LayerSpec{cin, cout, k, s2 ? 2 : 1, k / 2, !s2, kind == UP, kind == STEM}, N, Hi, Wi);
        l.out_floats = (size_t)l.e.My * cout;
        p.L.push_back(l);
    };
    int C = d->ngf, h = H, w = W;
    add(STEM, d->in_ch, C, 7, h, w);
    for (int i = 0; i < d->n_down; ++i) { add(DOWN, C, 2 * C, 3, h, w); C *= 2; h /= 2; w /= 2; }
    p.Hb = h; p.Wb = w; p.Cb = C;
    for (int i = 0; i < 2 * d->n_blocks; ++i) add(RES, C, C, 3, h, w);
    for (int i = 0; i < d->n_up; ++i) { add(UP, C, C / 2, 3, h, w); C /= 2; h *= 2; w *= 2; }
    add(OUT, C, d->out_ch, 7, h, w);
    const size_t blk = (size_t)N * p.Hb * p.Wb * p.Cb;
    size_t st = 0, pk = 0;
    for (Layer& l : p.L) {
        l.packed = pk; pk += l.e.packed_floats;
        if (l.kind != OUT) { l.c = st; st += l.out_floats; }
    }
    for (int k = 0; k <= d->n_blocks; ++k) { p.a.push_back(st); st += blk; }
    size_t stat = 0, fconv = 0, bconv = 0, wg = 0, coef = 0;
    for (Layer& l : p.L) {
        fconv = std::max(fconv, (size_t)l.e.fwd.partial * sizeof(float));
        bconv = std::max(bconv, (size_t)l.e.dx.partial * sizeof(float));
        wg = std::max(wg, (size_t)l.e.wgp.partial * sizeof(float));
        if (l.kind == OUT) continue;
        const int cout = l.e.s.cout;
        int64_t pd;
        l.nchunks = enc::stats_chunks(N, l.e.Ho * l.e.Wo, cout, &pd);
        l.ss = st; st += (size_t)2 * N * cout;
        l.mr = st; st += (size_t)2 * N * cout;
        stat = std::max(stat, (size_t)pd * sizeof(double));
        coef = std::max(coef, (size_t)3 * N * cout * sizeof(float));
    }
    p.packed_floats = pk; p.state_floats = st;
    // The backward's gradient buffers.  Two alternate down the layers (a layer reads R from one and writes dn, normalised in place, to
    // the other); a ResBlk needs a third: G stays in one while dc2 and then dL/da_{k-1} take the other and dn1 / dc1 the third.  The walk
    // below is the backward's own, for the sizes
    size_t need[3] = {0, 0, blk};
    {
        int cur = 0;
        const int n = (int)p.L.size();
        auto in_floats = [&](const Layer& l) { return (size_t)N * l.e.Hi * l.e.Wi * l.e.s.cin; };
        need[0] = in_floats(p.L[n - 1]);
        for (int i = n - 2; i >= 1; --i) {
            const Layer& l = p.L[i];
            if (l.kind == RES && (i - 1 - d->n_down) % 2 == 0) continue;        // the first convolution of a ResBlk: with the second
            cur ^= 1;
            need[cur] = std::max(need[cur], in_floats(l));
        }
    }
    // the forward and the backward never run at once on a workspace: the larger of the two
    Carver f, b;
    p.f_stats = f.take(stat);
    p.f_conv = f.take(fconv);
    for (int i = 0; i < 3; ++i) p.b_buf[i] = b.take(need[i] * sizeof(float));
    p.b_conv = b.take(bconv);
    p.b_wg = b.take(wg);
    p.b_stats = b.take(stat);
    p.b_coef = b.take(coef);
    const enc::Layer& o = p.L.back().e;
    p.b_db = b.take((size_t)enc::dbias_chunks(o.My) * o.s.cout * sizeof(double));
    p.bytes = std::max<size_t>(std::max(f.o, b.o), 256);
    return p;
}
inline Plan plan(const kpn_res_encoder_desc* d) { return plan(d, d->N, d->H, d->W); }
inline int n_layers(const kpn_res_encoder_desc* d) { return 2 + d->n_down + 2 * d->n_blocks + d->n_up; }
}  // namespace rte

#define KPN_RTE_REQUIRE_DESC(desc) do { if (const char* e_ = rte::desc_error(desc)) return fail(KPN_EINVAL, std::string("kpn_res_encoder_desc: ") + e_); } while (0)

extern "C" int32_t kpn_res_encoder_layers(const kpn_res_encoder_desc* desc) {
    return rte::weight_error(desc) ? 0 : rte::n_layers(desc);
}
extern "C" size_t kpn_res_encoder_workspace_bytes(const kpn_res_encoder_desc* desc) {
    return rte::desc_error(desc) ? 0 : rte::plan(desc).bytes;
}
extern "C" size_t kpn_res_encoder_state_floats(const kpn_res_encoder_desc* desc) {
    return rte::desc_error(desc) ? 0 : rte::plan(desc).state_floats;
}
extern "C" size_t kpn_res_encoder_packed_floats(const kpn_res_encoder_desc* desc) {
    return rte::weight_error(desc) ? 0 : rte::plan(desc, 1, 1 << desc->n_down, 1 << desc->n_down).packed_floats;
}
extern "C" int kpn_res_encoder_pack_device(const kpn_res_encoder_desc* desc, const float* const* weights, float* packed, void* stream) {
    if (const char* e = rte::weight_error(desc)) return fail(KPN_EINVAL, std::string("kpn_res_encoder_desc: ") + e);
    KPN_REQUIRE(weights && packed, "null pointer");
    KPN_REQUIRE(((uintptr_t)packed & 15) == 0, "packed must be 16-byte aligned");
    const rte::Plan p = rte::plan(desc, 1, 1 << desc->n_down, 1 << desc->n_down);
    for (size_t i = 0; i < p.L.size(); ++i) KPN_REQUIRE(weights[i], "weights: the weight of a layer is null");
    for (size_t i = 0; i < p.L.size(); ++i) enc::layer_pack(p.L[i].e, weights[i], packed + p.L[i].packed, stream);
    return check_launch("kpn_res_encoder_pack_device");
}
extern "C" int kpn_res_encoder_forward(const kpn_res_encoder_desc* desc, const float* x, const float* packed, const float* const* bias,
                                       float* y, float* state, void* workspace, size_t workspace_bytes, void* stream) {
    KPN_RTE_REQUIRE_DESC(desc);
    KPN_REQUIRE(x && packed && bias && y && state && workspace, "null pointer");
    const rte::Plan p = rte::plan(desc);
    const int n = (int)p.L.size(), N = desc->N;
    for (int i = 0; i < n; ++i) KPN_REQUIRE(bias[i], "bias: the bias of a layer is null");
    KPN_REQUIRE(enc::aligned16({packed, y, state, workspace}), "packed / y / state / workspace must be 16-byte aligned");
    KPN_REQUIRE(workspace_bytes >= p.bytes, "workspace too small (kpn_res_encoder_workspace_bytes)");
    char* ws = static_cast<char*>(workspace);
    double* stat = reinterpret_cast<double*>(ws + p.f_stats);
    float* part = reinterpret_cast<float*>(ws + p.f_conv);
    auto conv = [&](int i, const float* src, const float* ss, float* dst) {
        const enc::Layer& e = p.L[i].e;
        enc::layer_forward(e, src, e.s.cin, ss, packed + p.L[i].packed, bias[i], dst, e.s.cout, nullptr, 0, part, stream);
    };
    auto stats = [&](int i) {
        const rte::Layer& l = p.L[i];
        const int C = l.e.s.cout;
        kpn_enc_stats_args a{};
        a.src = state + l.c; a.cs = C; a.C = C; a.HW = l.e.Ho * l.e.Wo; a.nchunks = l.nchunks; a.nimg = N;
        a.partial = stat;
        a.G = C; a.eps = desc->eps;
        a.ss = state + l.ss; a.mr = state + l.mr;
        enc::launch_stats(a, stream);
    };
    const int HWb = p.Hb * p.Wb;
    int i = 0;
    conv(0, x, nullptr, state + p.L[0].c);
    stats(0);
    for (i = 1; i <= desc->n_down; ++i) {
        conv(i, state + p.L[i - 1].c, state + p.L[i - 1].ss, state + p.L[i].c);
        stats(i);
    }
    enc::launch_affine(state + p.L[i - 1].c, state + p.L[i - 1].ss, 1, nullptr, state + p.a[0], N, HWb, p.Cb, stream);
    for (int b = 0; b < desc->n_blocks; ++b, i += 2) {
        conv(i, state + p.a[b], nullptr, state + p.L[i].c);
        stats(i);
        conv(i + 1, state + p.L[i].c, state + p.L[i].ss, state + p.L[i + 1].c);
        stats(i + 1);
        enc::launch_affine(state + p.L[i + 1].c, state + p.L[i + 1].ss, 0, state + p.a[b], state + p.a[b + 1], N, HWb, p.Cb, stream);
    }
    for (int u = 0; u < desc->n_up; ++u, ++i) {
        if (u == 0) conv(i, state + p.a[desc->n_blocks], nullptr, state + p.L[i].c);
        else conv(i, state + p.L[i - 1].c, state + p.L[i - 1].ss, state + p.L[i].c);
        stats(i);
    }
    conv(i, state + p.L[i - 1].c, state + p.L[i - 1].ss, y);
    return check_launch("kpn_res_encoder_forward");
}
extern "C" int kpn_res_encoder_backward(const kpn_res_encoder_desc* desc, const float* x, const float* dy, const float* packed,
                                        const float* state, float* const* dw, float* const* db, void* workspace, size_t workspace_bytes,
                                        void* stream) {
    KPN_RTE_REQUIRE_DESC(desc);
    KPN_REQUIRE(x && dy && packed && state && dw && db && workspace, "null pointer");
    const rte::Plan p = rte::plan(desc);
    const int n = (int)p.L.size(), N = desc->N, nd = desc->n_down, nb = desc->n_blocks;
    for (int i = 0; i < n; ++i) KPN_REQUIRE(enc::aligned16({dw[i], db[i]}), "dw / db must be 16-byte aligned");
    KPN_REQUIRE(enc::aligned16({dy, packed, state, workspace}), "dy / packed / state / workspace must be 16-byte aligned");
    KPN_REQUIRE(workspace_bytes >= p.bytes, "workspace too small (kpn_res_encoder_workspace_bytes)");
    char* ws = static_cast<char*>(workspace);
    float* buf[3] = {reinterpret_cast<float*>(ws + p.b_buf[0]), reinterpret_cast<float*>(ws + p.b_buf[1]), reinterpret_cast<float*>(ws + p.b_buf[2])};
    float* cpart = reinterpret_cast<float*>(ws + p.b_conv);
    float* wpart = reinterpret_cast<float*>(ws + p.b_wg);
    double* stat = reinterpret_cast<double*>(ws + p.b_stats);
    float* coef = reinterpret_cast<float*>(ws + p.b_coef);
    // the layers below `first` need nothing: the walk ends there.  A bias in front of an InstanceNorm2d has the gradient zero
    int first = n;
    for (int i = n - 1; i >= 0; --i)
        if (dw[i]) first = i;
    hipError_t zero_err = hipSuccess;
    for (int i = 0; i < n - 1; ++i)
        if (db[i]) {
            const hipError_t e = hipMemsetAsync(db[i], 0, (size_t)p.L[i].e.s.cout * sizeof(float), (hipStream_t)stream);
            if (e != hipSuccess && zero_err == hipSuccess) zero_err = e;
        }
    if (zero_err != hipSuccess) return fail(KPN_ELAUNCH, std::string("kpn_res_encoder_backward: zeroing a bias gradient failed: ") + hipGetErrorString(zero_err));
    // dW of layer i for R = dL/dc_i; its source is `src`, lazily normalised with `ss` or (ss = NULL) a materialised tensor
    auto wgrad = [&](int i, const float* src, const float* ss, const float* R) {
        const enc::Layer& e = p.L[i].e;
        if (dw[i]) enc::layer_wgrad(e, src, e.s.cin, ss, R, e.s.cout, wpart, dw[i], stream);
    };
    // dn = the input gradient of layer i for R [+ res]
    auto dgrad = [&](int i, const float* R, float* dn, const float* res) {
        const enc::Layer& e = p.L[i].e;
        enc::layer_dgrad(e, R, e.s.cout, packed + p.L[i].packed, dn, e.s.cin, res, e.s.cin, cpart, stream);
    };
    // dst = the gradient of the norm behind layer i (with its ReLU or without) for the gradient g of its output; dst may be g
    auto norm_bwd = [&](int i, const float* g, int relu, float* dst) {
        const rte::Layer& l = p.L[i];
        kpn_enc_norm_bwd_args a{};
        const int C = l.e.s.cout;
        a.x = state + l.c; a.x_cs = C; a.dy = g; a.ss = state + l.ss; a.mr = state + l.mr;
        a.relu = relu; a.C = C; a.HW = l.e.Ho * l.e.Wo; a.nchunks = l.nchunks; a.nimg = N; a.G = C;
        a.partial = stat; a.coef = coef; a.dx = dst;
        enc::launch_norm_bwd(a, stream);
    };
    int i = n - 1, cur = 0;
    const float* R = dy;
    {   // the output layer
        const enc::Layer& e = p.L[i].e;
        wgrad(i, state + p.L[i - 1].c, state + p.L[i - 1].ss, R);
        if (db[i]) enc::launch_dbias(dy, e.My, e.s.cout, reinterpret_cast<double*>(ws + p.b_db), db[i], stream);
        if (first < i) {
            dgrad(i, R, buf[0], nullptr);
            norm_bwd(i - 1, buf[0], 1, buf[0]);
            R = buf[0];
        }
    }
    for (--i; i > nd + 2 * nb && first <= i; --i) {      // the transposed layers
        const bool lazy = i > nd + 2 * nb + 1;
        wgrad(i, lazy ? state + p.L[i - 1].c : state + p.a[nb], lazy ? state + p.L[i - 1].ss : nullptr, R);
        if (first < i) {
            cur ^= 1;
            dgrad(i, R, buf[cur], nullptr);
            if (lazy) norm_bwd(i - 1, buf[cur], 1, buf[cur]);
            R = buf[cur];                                  // i == nd + 2 nb + 1: dL/da_{n_blocks}
        }
    }
    for (int b = nb - 1; b >= 0 && first <= i; --b, i -= 2) {      // the ResBlks: i is the block's second convolution, R = G = dL/da_{b+1}
        const float* G = R;
        float* dc2 = buf[cur ^ 1];
        norm_bwd(i, G, 0, dc2);
        wgrad(i, state + p.L[i - 1].c, state + p.L[i - 1].ss, dc2);
        if (first < i) {
            dgrad(i, dc2, buf[2], nullptr);
            norm_bwd(i - 1, buf[2], 1, buf[2]);              // dc1
            wgrad(i - 1, state + p.a[b], nullptr, buf[2]);
            if (first < i - 1) dgrad(i - 1, buf[2], dc2, G);      // dL/da_b = rp-adjoint(dc1) + G; dc2 is done with
        }
        cur ^= 1;
        R = buf[cur];
    }
    if (first <= i && i == nd) {                                    // a_0: R = dL/da_0 -> dL/dc of the last stride-2 layer, in place
        norm_bwd(i, R, 1, buf[cur]);
        R = buf[cur];
    }
    for (; i >= 1 && first <= i; --i) {                             // the stride-2 layers
        wgrad(i, state + p.L[i - 1].c, state + p.L[i - 1].ss, R);
        if (first < i) {
            cur ^= 1;
            dgrad(i, R, buf[cur], nullptr);
            norm_bwd(i - 1, buf[cur], 1, buf[cur]);
            R = buf[cur];
        }
    }
    if (first == 0 && i == 0) wgrad(0, x, nullptr, R);
    return check_launch("kpn_res_encoder_backward");
}

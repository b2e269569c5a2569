// ---------------------------------------------------------------------------------------------
// The image encoders, HGFilterV2 and ResBlkEncoder (reference src/utils.py:199-474), forward.  Kernels: encoder_kernels.hip.
// Each network is written once, as a walk over its layers (enc::geo_walk / enc::tex_walk) that a context runs in one of
// three modes: COUNT (sizes of the plain and packed parameter vectors, the workspace and the stage buffer), PACK (launch the
// packers) and RUN (launch the forward).  The order in which a walk asks for parameters defines the plain layout
// (keypointnerf_amd/encoders.py builds it from the caller's module in the same order).
//
// In front of the walks, the launch layer of encoder_kernels.hip: every launch policy of the kernels that the walks share with
// the differentiable layers (api_conv.hip, api_strided.hip, api_reppad.hip, api_norm.hip, api_block.hip, api_resample.hip) - tiles,
// split K, the ranges of a weight gradient, chunk counts, grids - is written there once, and all of these files launch through it.  The split-K rule and the chunk rule fix the order of floating-point sums,
// so a walk and a layer agree bit for bit only while they share this code.  What one differentiable convolution layer is in terms of these
// launches (enc::Layer) follows in api_layer.hip.
namespace enc {

// the grid of the elementwise kernels (grid-stride loops over n items): blocks of 256 threads, at most 8192 of them
inline dim3 grid4(int64_t n) { return dim3((unsigned)std::min<int64_t>((n + 255) / 256, 8192)); }

// one k_enc_conv GEMM: cin -> cout over nimg * Ho * Wo rows (DECONV: (Ho, Wo) is the source grid, one GEMM per parity class)
// The arithmetic of a GEMM (KPN_CONV_F32 / KPN_CONV_BF16X3, include/kpnerf.h) is part of its geometry: tile, K chunk, packed size, the
// split-K rule's inputs and the weight-gradient plan follow from it, and every launch below dispatches on it.  KPN_CONV_BF16X3 exists
// for the plain NHWC stride-1 GEMM only (encoder_split_kernels.hip): no stem, no deconv, no replication padding.
struct ConvGeom {
    kpn_enc_conv_args a;   // what the geometry decides (sizes, cin_p, cout_p, nk, wofs, ksplit); the caller adds tensors, padding, epilogue
    int arith;
    int bn, bm;            // tile: 64 x 64, or 128 x 32 for at most 32 output channels; KPN_CONV_BF16X3: 128 x 64, or 256 x 32
    int deconv, ncls;      // parity classes: 4 or 1
    int64_t packed;        // floats: the packed weight, every class
    int64_t M;             // GEMM rows
    int64_t partial;       // floats: the split-K scratch, 0 without a split
};
inline ConvGeom conv_geom(int nimg, int Ho, int Wo, int cin, int cout, int kh, int kw, int deconv, int arith = KPN_CONV_F32) {
    ConvGeom g{};
    kpn_enc_conv_args& a = g.a;
    a.nimg = nimg; a.Ho = Ho; a.Wo = Wo; a.cin = cin; a.cout = cout; a.kh = kh; a.kw = kw;
    g.arith = arith;
    const bool b3 = arith == KPN_CONV_BF16X3;
    g.bn = cout > 32 ? 64 : 32; g.bm = (g.bn == 64 ? 64 : 128) * (b3 ? 2 : 1);
    const int kc = b3 ? 32 : 16;                    // K chunk
    const int cfl = b3 ? 48 : 16;                   // floats of the packed weight per chunk and output channel (bf16 x 3: 32 x 6 bytes)
    // the 3-channel stems pad to 4; api_conv.hip admits only cin % 4 == 0, for which cin_p == cin: one formula serves both
    a.cin_p = (cin + 3) / 4 * 4;
    a.cout_p = (cout + g.bn - 1) / g.bn * g.bn;
    g.deconv = deconv; g.ncls = deconv ? 4 : 1;
    int nkmin = 1 << 30;
    for (int c = 0; c < g.ncls; ++c) {
        const int taps = deconv ? (1 + (c >> 1)) * (1 + (c & 1)) : kh * kw;
        a.nk[c] = (taps * a.cin_p + kc - 1) / kc;
        a.wofs[c] = g.packed;
        g.packed += (int64_t)a.nk[c] * a.cout_p * cfl;
        nkmin = std::min(nkmin, a.nk[c]);
    }
    // split K by the per-image geometry only: an image's result must not depend on how many images are encoded with it
    const int64_t tiles_img = ((int64_t)Ho * Wo + g.bm - 1) / g.bm * (a.cout_p / g.bn) * g.ncls;
    a.ksplit = 1;
    if (tiles_img < 128) a.ksplit = (int)std::max<int64_t>(1, std::min<int64_t>(std::min(nkmin, 16), (256 + tiles_img - 1) / tiles_img));
    g.M = (int64_t)nimg * Ho * Wo;
    g.partial = a.ksplit > 1 ? (int64_t)g.ncls * a.ksplit * g.M * a.cout_p : 0;
    return g;
}
// `a`: g.a with the caller's fields filled in
inline void launch_conv(const kpn_enc_conv_args& a, const ConvGeom& g, int stem, void* stream) {
    const dim3 grid((unsigned)((g.M + g.bm - 1) / g.bm * (a.cout_p / g.bn)), (unsigned)a.ksplit, (unsigned)g.ncls);
    if (g.arith == KPN_CONV_BF16X3) {
        if (g.bn == 64) KPN_LAUNCH((k_enc_conv_b3<128, 64>), grid, dim3(256), stream, a);
        else KPN_LAUNCH((k_enc_conv_b3<256, 32>), grid, dim3(256), stream, a);
    } else if (stem) {
        if (g.bn == 64) KPN_LAUNCH((k_enc_conv<64, 64, true, false>), grid, dim3(256), stream, a);
        else KPN_LAUNCH((k_enc_conv<128, 32, true, false>), grid, dim3(256), stream, a);
    } else if (g.deconv) {
        if (g.bn == 64) KPN_LAUNCH((k_enc_conv<64, 64, false, true>), grid, dim3(256), stream, a);
        else KPN_LAUNCH((k_enc_conv<128, 32, false, true>), grid, dim3(256), stream, a);
    } else {
        if (g.bn == 64) KPN_LAUNCH((k_enc_conv<64, 64, false, false>), grid, dim3(256), stream, a);
        else KPN_LAUNCH((k_enc_conv<128, 32, false, false>), grid, dim3(256), stream, a);
    }
    if (a.ksplit > 1) KPN_LAUNCH(k_enc_combine, grid4((int64_t)g.ncls * g.M * a.cout), dim3(256), stream, a, g.deconv);
}
// the input gradient of a replication-padded stride-1 convolution (enc::layer_dgrad): the same GEMM, tiles, split K and combine, with
// the adjoint of the clamped load in place of the load.  `a`: g.a of conv_geom(N, H, W, layer cout, layer cin, k, k, 0) with src = dy,
// (Hs, Ws) = (H, W), pad = k / 2 and the tflip copy of the weight
inline void launch_conv_rp_adjoint(const kpn_enc_conv_args& a, const ConvGeom& g, void* stream) {
    const dim3 grid((unsigned)((g.M + g.bm - 1) / g.bm * (a.cout_p / g.bn)), (unsigned)a.ksplit, 1u);
    if (g.bn == 64) KPN_LAUNCH((k_enc_conv<64, 64, false, false, true>), grid, dim3(256), stream, a);
    else KPN_LAUNCH((k_enc_conv<128, 32, false, false, true>), grid, dim3(256), stream, a);
    if (a.ksplit > 1) KPN_LAUNCH(k_enc_combine, grid4(g.M * a.cout), dim3(256), stream, a, 0);
}
// plain OIHW (DECONV: IOHW) weight `w` -> the packed weight `wp`, every class.  tflip: the operand of the input gradient
inline void launch_pack(const ConvGeom& g, int tflip, const float* w, float* wp, void* stream) {
    for (int c = 0; c < g.ncls; ++c) {
        kpn_enc_pack_args pa{w, wp + g.a.wofs[c], g.a.cin, g.a.cin_p, g.a.cout, g.a.cout_p, g.a.kh, g.a.kw, g.a.nk[c], g.deconv, c, tflip};
        if (g.arith == KPN_CONV_BF16X3) {       // one thread per 16-byte unit of each piece
            const int64_t n = (int64_t)g.a.nk[c] * g.a.cout_p * 4;
            KPN_LAUNCH(k_enc_pack_b3, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 4096)), dim3(256), stream, pa);
            continue;
        }
        const int64_t n = (int64_t)g.a.nk[c] * g.a.cout_p * 16;
        KPN_LAUNCH(k_enc_pack, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 4096)), dim3(256), stream, pa);
    }
}
// The weight gradient of the GEMM `g` (k_enc_wgrad on g's tile over (K rows, cout), then k_enc_wgrad_combine).  Its ranges: a range is
// `cpr` chunks of 16 GEMM pixels, at least 20 (320 pixels: what a tile's store and combine are worth) and otherwise as many as leave
// about 1024 workgroups, at most 64 ranges.  From the shape alone - and the arithmetic, whose tile (g.bm x g.bn) counts the tiles:
// k_enc_wgrad_b3 takes 128 x 64 / 256 x 32 of (K rows, cout), so it has half the tiles and may take twice the ranges.
struct WgradPlan {
    int krows;                     // kh * kw * cin: the rows of `partial` and of dW
    int tiles, nchunks, cpr, nranges;
    int64_t partial;               // floats: [range][krows][cout]
};
inline WgradPlan wgrad_plan(const ConvGeom& g) {
    WgradPlan p{};
    const kpn_enc_conv_args& a = g.a;
    p.krows = a.kh * a.kw * a.cin;
    p.tiles = (a.kh * a.kw * a.cin_p + g.bm - 1) / g.bm * (a.cout_p / g.bn);
    p.nchunks = (int)((g.M + 15) / 16);
    const int rmax = std::max(1, std::min(64, 1024 / p.tiles));
    p.cpr = std::max(20, (p.nchunks + rmax - 1) / rmax);
    p.nranges = (p.nchunks + p.cpr - 1) / p.cpr;
    p.partial = (int64_t)p.nranges * p.krows * a.cout;
    return p;
}
// `c`: g.a with the source of A filled in (Hs, Ws, stride, pad, src, src_cs; the stem's Hraw, Wraw, stem_plain; ss and relu_in = 1 for
// a norm fused into the loads); rhs (g.M, cout) with channel stride rhs_cs; rhs_ss: the scale / shift of a norm + ReLU fused into the
// loads of rhs, or NULL
inline void launch_wgrad(const kpn_enc_conv_args& c, const ConvGeom& g, const WgradPlan& p, int stem, const float* rhs, int rhs_cs,
                         float* partial, float* dw, void* stream, const float* rhs_ss = nullptr) {
    kpn_enc_wgrad_args a{};
    a.c = c;
    a.rhs = rhs; a.rhs_cs = rhs_cs; a.rhs_ss = rhs_ss; a.rhs_relu = rhs_ss != nullptr; a.krows = p.krows; a.nchunks = p.nchunks; a.cpr = p.cpr; a.nranges = p.nranges;
    a.partial = partial; a.dw = dw;
    const dim3 grid((unsigned)p.tiles, (unsigned)p.nranges);
    if (g.arith == KPN_CONV_BF16X3) {
        if (g.bn == 64) KPN_LAUNCH((k_enc_wgrad_b3<128, 64>), grid, dim3(256), stream, a);
        else KPN_LAUNCH((k_enc_wgrad_b3<256, 32>), grid, dim3(256), stream, a);
    } else if (stem) {
        if (g.bn == 64) KPN_LAUNCH((k_enc_wgrad<64, 64, true>), grid, dim3(256), stream, a);
        else KPN_LAUNCH((k_enc_wgrad<128, 32, true>), grid, dim3(256), stream, a);
    } else {
        if (g.bn == 64) KPN_LAUNCH((k_enc_wgrad<64, 64, false>), grid, dim3(256), stream, a);
        else KPN_LAUNCH((k_enc_wgrad<128, 32, false>), grid, dim3(256), stream, a);
    }
    KPN_LAUNCH(k_enc_wgrad_combine, grid4((int64_t)c.kh * c.kw * c.cin_p * c.cout), dim3(256), stream, a);
}
// the bias gradient: db[c] = sum over the M rows of dy (M, C); `partial` holds dbias_chunks(M) * C doubles
inline int dbias_chunks(int64_t M) { return (int)std::max<int64_t>(1, std::min<int64_t>(256, M / 256)); }
inline void launch_dbias(const float* dy, int64_t M, int C, double* partial, float* db, void* stream) {
    kpn_enc_dbias_args a{dy, M, C, dbias_chunks(M), partial, db};
    KPN_LAUNCH(k_enc_dbias_partial, dim3((unsigned)a.nchunks), dim3(256), stream, a);
    KPN_LAUNCH(k_enc_dbias_final, dim3((unsigned)((C + 63) / 64)), dim3(64), stream, a);
}
// statistics: pixel chunks per image (from the shape alone; the forward and the backward of a norm share it) and the doubles of
// the partials [image][chunk][channel][2]
inline int stats_chunks(int nimg, int HW, int C, int64_t* partial_doubles) {
    const int nchunks = std::max(1, std::min(64, HW / 256));
    *partial_doubles = (int64_t)nimg * nchunks * C * 2;
    return nchunks;
}
inline void launch_stats(const kpn_enc_stats_args& a, void* stream) {
    KPN_LAUNCH(k_enc_stats_partial, dim3((unsigned)a.nchunks, (unsigned)a.nimg), dim3(256), stream, a);
    KPN_LAUNCH(k_enc_stats_final, dim3((unsigned)((a.nimg * a.G + 63) / 64)), dim3(64), stream, a);
}
// the three passes of a norm's gradient (pass 3 only with a.coef); a.nchunks is stats_chunks' of the same shape
inline void launch_norm_bwd(const kpn_enc_norm_bwd_args& a, void* stream) {
    KPN_LAUNCH(k_enc_norm_bwd_partial, dim3((unsigned)a.nchunks, (unsigned)a.nimg), dim3(256), stream, a);
    KPN_LAUNCH(k_enc_norm_bwd_final, dim3((unsigned)((a.nimg * a.G + a.C + 63) / 64)), dim3(64), stream, a);
    if (a.coef) KPN_LAUNCH(k_enc_norm_bwd_dx, grid4((int64_t)a.nimg * a.HW * a.C / 4), dim3(256), stream, a);
}
inline void launch_add_cs(const float* a, int a_cs, const float* b, int b_cs, float* dst, int dst_cs, int64_t M, int C, void* stream) {
    KPN_LAUNCH(k_enc_add_cs, grid4(M * C / 4), dim3(256), stream, a, a_cs, b, b_cs, dst, dst_cs, M, C);
}
inline void launch_affine(const float* src, const float* ss, int relu, const float* res, float* dst, int nimg, int HW, int C, void* stream) {
    KPN_LAUNCH(k_enc_affine, grid4((int64_t)nimg * HW * C / 4), dim3(256), stream, src, ss, relu, res, dst, nimg, HW, C);
}
// (h, w) is the low grid of both; a thread writes one float4 (C % 4 == 0) of the output, the high one having 4 h w C / 4 of them
inline void launch_pool2(const float* high, float* low, int nimg, int h, int w, int C, void* stream) {
    KPN_LAUNCH(k_enc_pool2, grid4((int64_t)nimg * h * w * C / 4), dim3(256), stream, high, low, nimg, h, w, C);
}
inline void launch_upadd(const float* low, const float* skip, float* high, int nimg, int h, int w, int C, void* stream) {
    KPN_LAUNCH(k_enc_upadd, grid4((int64_t)nimg * h * w * C), dim3(256), stream, low, skip, high, nimg, h, w, C);
}

// ---- The walks.
enum Mode { COUNT, PACK, RUN };
struct View {              // NHWC activations (or a channel slice of them): workspace offset or caller memory
    int64_t off;
    float* ext;
    int H, W, C, cs;
};
struct ConvSpec { int cin, cout, kh, kw, stride, pad, replicate, deconv, bias; };
struct StageInfo { std::string name; int64_t off; int H, W, C; };
struct Ctx {
    Mode mode = COUNT;
    void* stream = nullptr;
    const float* plain = nullptr;   // PACK
    float* packed = nullptr;        // PACK (written) / RUN (read)
    float* ws = nullptr;
    float* stages = nullptr;
    const float* img = nullptr;     // (nimg, 3, Hraw, Wraw)
    int nimg = 1, Hraw = 0, Wraw = 0, ds = 0;
    float eps = 1e-5f;
    int64_t plain_off = 0, packed_off = 0, stage_off = 0;
    std::vector<StageInfo> stage_list;
    // workspace: first fit over a free list, so that COUNT and RUN place every tensor alike
    std::vector<std::pair<int64_t, int64_t>> free_;
    int64_t brk = 0, high = 0;
    hipError_t copy_err = hipSuccess;       // the first failed parameter / stage copy
    void copy(void* d, const void* s, size_t n) {
        const hipError_t e = hipMemcpyAsync(d, s, n, hipMemcpyDeviceToDevice, (hipStream_t)stream);
        if (e != hipSuccess && copy_err == hipSuccess) copy_err = e;
    }

    static int64_t r4(int64_t n) { return (n + 3) / 4 * 4; }
    int64_t alloc_raw(int64_t n) {
        n = r4(n);
        for (size_t i = 0; i < free_.size(); ++i)
            if (free_[i].second >= n) {
                const int64_t off = free_[i].first;
                free_[i].first += n; free_[i].second -= n;
                if (free_[i].second == 0) free_.erase(free_.begin() + i);
                return off;
            }
        const int64_t off = brk;
        brk += n;
        if (brk > high) high = brk;
        return off;
    }
    void release_raw(int64_t off, int64_t n) {
        n = r4(n);
        size_t i = 0;
        while (i < free_.size() && free_[i].first < off) ++i;
        free_.insert(free_.begin() + i, {off, n});
        if (i + 1 < free_.size() && free_[i].first + free_[i].second == free_[i + 1].first) {
            free_[i].second += free_[i + 1].second;
            free_.erase(free_.begin() + i + 1);
        }
        if (i > 0 && free_[i - 1].first + free_[i - 1].second == free_[i].first) {
            free_[i - 1].second += free_[i].second;
            free_.erase(free_.begin() + i);
        }
        if (!free_.empty() && free_.back().first + free_.back().second == brk) {
            brk = free_.back().first;
            free_.pop_back();
        }
    }
    View alloc(int H, int W, int C) { return View{alloc_raw((int64_t)nimg * H * W * C), nullptr, H, W, C, C}; }
    void release(const View& v) { if (!v.ext) release_raw(v.off, (int64_t)nimg * v.H * v.W * v.C); }
    float* ptr(const View& v) const { return v.ext ? v.ext : ws + v.off; }
    static View slice(View v, int c0, int C) {
        if (v.ext) v.ext += c0; else v.off += c0;
        v.C = C;
        return v;
    }
    // a parameter vector (bias, gamma, beta): copied as it is
    const float* vec(int n) {
        const float* p = packed ? packed + packed_off : nullptr;
        if (mode == PACK) copy(packed + packed_off, plain + plain_off, (size_t)n * sizeof(float));
        plain_off += n;
        packed_off += r4(n);
        return p;
    }
    void stage(const char* name, const View& v) {
        const int64_t n = (int64_t)nimg * v.H * v.W * v.C;
        if (mode == COUNT) stage_list.push_back(StageInfo{name, stage_off, v.H, v.W, v.C});
        if (mode == RUN && stages) copy(stages + stage_off, ptr(v), (size_t)n * sizeof(float));
        stage_off += n;
    }

    // src: the stem reads `img` instead (stem != 0).  ss: offset of scale / shift in the workspace or -1
    void conv(const ConvSpec& s, const View& src, int64_t ss, int relu_in, const View& dst, const View* res, int relu_out, int stem = 0) {
        const ConvGeom g = conv_geom(nimg, s.deconv ? src.H : dst.H, s.deconv ? src.W : dst.W, s.cin, s.cout, s.kh, s.kw, s.deconv);
        // parameters: weight, then bias
        const float* wp = packed ? packed + packed_off : nullptr;
        if (mode == PACK) launch_pack(g, 0, plain + plain_off, packed + packed_off, stream);
        plain_off += (int64_t)s.cout * s.cin * s.kh * s.kw;
        packed_off += g.packed;
        const float* bias = s.bias ? vec(s.cout) : nullptr;
        const int64_t poff = g.partial ? alloc_raw(g.partial) : 0;
        if (mode == RUN) {
            kpn_enc_conv_args a = g.a;
            a.Hs = src.H; a.Ws = src.W;
            a.stride = s.stride; a.pad = s.pad; a.replicate = s.replicate;
            a.src = stem ? img : ptr(src);
            a.src_cs = src.cs; a.Hraw = Hraw; a.Wraw = Wraw; a.ds = ds;
            a.ss = ss >= 0 ? ws + ss : nullptr;
            a.relu_in = relu_in;
            a.wp = wp; a.bias = bias;
            a.dst = ptr(dst); a.dst_cs = dst.cs;
            a.res = res ? ptr(*res) : nullptr; a.res_cs = res ? res->cs : 0;
            a.relu_out = relu_out;
            a.partial = g.partial ? ws + poff : nullptr;
            launch_conv(a, g, stem, stream);
        }
        if (g.partial) release_raw(poff, g.partial);
    }
    // GroupNorm(G, C) (affine) or InstanceNorm2d (G = C, no affine) statistics of x -> offset of scale / shift
    int64_t stats(const View& x, int G, int affine) {
        const float* gamma = affine ? vec(x.C) : nullptr;
        const float* beta = affine ? vec(x.C) : nullptr;
        int64_t pd;
        const int nchunks = stats_chunks(nimg, x.H * x.W, x.C, &pd);
        const int64_t ss = alloc_raw((int64_t)2 * nimg * x.C);
        const int64_t pn = pd * 2;                                       // doubles, counted in floats
        const int64_t po = alloc_raw(pn);
        if (mode == RUN) {
            kpn_enc_stats_args a{};
            a.src = ptr(x); a.cs = x.cs; a.C = x.C; a.HW = x.H * x.W; a.nchunks = nchunks; a.nimg = nimg;
            a.partial = reinterpret_cast<double*>(ws + po);
            a.G = G; a.gamma = gamma; a.beta = beta; a.eps = eps; a.ss = ws + ss;
            launch_stats(a, stream);
        }
        release_raw(po, pn);
        return ss;
    }
    void free_ss(int64_t ss, int C) { release_raw(ss, (int64_t)2 * nimg * C); }
    void affine(const View& src, int64_t ss, int relu, const View* res, const View& dst) {
        if (mode != RUN) return;
        launch_affine(ptr(src), ss >= 0 ? ws + ss : nullptr, relu, res ? ptr(*res) : nullptr, ptr(dst), nimg, src.H * src.W, src.C, stream);
    }
    View pool(const View& x) {
        View o = alloc(x.H / 2, x.W / 2, x.C);
        if (mode == RUN) launch_pool2(ptr(x), ptr(o), nimg, o.H, o.W, o.C, stream);
        return o;
    }
    void upadd(const View& low, const View& up) {
        if (mode == RUN) launch_upadd(ptr(low), ptr(up), ptr(up), nimg, low.H, low.W, low.C, stream);
    }
};

// ConvBlock (src/utils.py:416-474, norm = "group"): the three convolutions write their slices of the concatenation
View conv_block(Ctx& c, const View& x, int cout) {
    const int cin = x.C;
    View O = c.alloc(x.H, x.W, cout);
    const int w[3] = {cout / 2, cout / 4, cout / 4}, at[3] = {0, cout / 2, cout / 2 + cout / 4};
    View in = x;
    for (int i = 0; i < 3; ++i) {
        const int64_t ss = c.stats(in, std::min(32, in.C), 1);
        const View out = Ctx::slice(O, at[i], w[i]);
        c.conv(ConvSpec{in.C, w[i], 3, 3, 1, 1, 0, 0, 0}, in, ss, 1, out, nullptr, 0);
        c.free_ss(ss, in.C);
        in = out;
    }
    if (cin != cout) {          // downsample: bn4, ReLU, 1x1 convolution, added to the concatenation in the epilogue
        const int64_t ss = c.stats(x, std::min(32, cin), 1);
        c.conv(ConvSpec{cin, cout, 1, 1, 1, 0, 0, 0, 0}, x, ss, 1, O, &O, 0);
        c.free_ss(ss, cin);
    } else {
        c.affine(O, -1, 0, &x, O);
    }
    return O;
}
// HourGlass._forward (src/utils.py:282-303); takes ownership of inp
View hourglass(Ctx& c, int level, const View& inp) {
    char nm[24];
    View up1 = conv_block(c, inp, inp.C);                 // b1
    snprintf(nm, sizeof nm, "m0.b1_%d", level); c.stage(nm, up1);
    View low = c.pool(inp);
    c.release(inp);
    View low1 = conv_block(c, low, low.C);                // b2
    c.release(low);
    View low2;
    if (level > 1) low2 = hourglass(c, level - 1, low1);
    else { low2 = conv_block(c, low1, low1.C); c.release(low1); }     // b2_plus
    View low3 = conv_block(c, low2, low2.C);              // b3
    c.release(low2);
    snprintf(nm, sizeof nm, "m0.b3_%d", level); c.stage(nm, low3);
    c.upadd(low3, up1);
    c.release(low3);
    return up1;
}
bool geo_shape_ok(int V, int H, int W, int ds, int out_ch, int out_ch_hd) {
    if (V < 1 || ds < 0 || ds > 1 || out_ch < 1 || out_ch > 512 || out_ch_hd < 1 || out_ch_hd > 512 || H < 1 || W < 1) return false;
    const int h = H >> ds, w = W >> ds;
    return h >= 64 && w >= 64 && h % 64 == 0 && w % 64 == 0 && (int64_t)V * h * w * 32 < (1ll << 30);
}
// HGFilterV2.forward (src/utils.py:370-414) for n_stack = 1, n_downsample = 4, hd = False, norm = "group"
void geo_walk(Ctx& c, int out_ch, int out_ch_hd, float* feat, float* feat_hd) {
    const int h = c.Hraw >> c.ds, w = c.Wraw >> c.ds;
    View im{0, nullptr, h, w, 3, 3};
    View t0 = c.alloc(h / 2, w / 2, 64);
    c.conv(ConvSpec{3, 64, 7, 7, 2, 3, 0, 0, 1}, im, -1, 0, t0, nullptr, 0, 1);          // conv1
    c.stage("conv1", t0);
    int64_t ss = c.stats(t0, 32, 1);                                                       // bn1
    c.affine(t0, ss, 1, nullptr, t0);
    c.free_ss(ss, 64);
    View x2 = conv_block(c, t0, 128);                                                      // conv2
    c.release(t0);
    c.stage("conv2", x2);
    {   // x_hd = conv_out(unpack1(x))
        View d = c.alloc(h, w, 32);
        c.conv(ConvSpec{128, 32, 3, 3, 2, 1, 0, 1, 0}, x2, -1, 0, d, nullptr, 0);
        c.stage("unpack1.conv", d);
        ss = c.stats(d, 32, 1);
        View hd{0, feat_hd, h, w, out_ch_hd, out_ch_hd};
        c.conv(ConvSpec{32, out_ch_hd, 5, 5, 1, 2, 0, 0, 1}, d, ss, 1, hd, nullptr, 0);
        c.free_ss(ss, 32);
        c.release(d);
    }
    View p = c.pool(x2);
    c.release(x2);
    View x3 = conv_block(c, p, 128);                                                       // conv3
    c.release(p);
    View x4 = conv_block(c, x3, 256);                                                      // conv4
    c.release(x3);
    c.stage("conv4", x4);
    View hg = hourglass(c, 4, x4);                                                         // m0 (releases x4)
    c.stage("m0", hg);
    View top = conv_block(c, hg, 256);                                                     // top_m_0
    c.release(hg);
    c.stage("top_m_0", top);
    View ll = c.alloc(top.H, top.W, 256);
    c.conv(ConvSpec{256, 256, 1, 1, 1, 0, 0, 0, 1}, top, -1, 0, ll, nullptr, 0);           // conv_last0
    c.release(top);
    c.stage("conv_last0", ll);
    ss = c.stats(ll, 32, 1);                                                               // bn_end0 + ReLU in the loads of l0
    View out{0, feat, ll.H, ll.W, out_ch, out_ch};
    c.conv(ConvSpec{256, out_ch, 1, 1, 1, 0, 0, 0, 1}, ll, ss, 1, out, nullptr, 0);
    c.free_ss(ss, 256);
    c.release(ll);
}

bool tex_shape_ok(int V, int H, int W, int ds, int ngf, int n_down, int n_blocks, int n_up, int out_ch) {
    if (V < 1 || ds < 0 || ds > 1 || out_ch < 1 || out_ch > 512 || n_down < 0 || n_down > 5 || n_blocks < 0 || n_blocks > 64) return false;
    if (n_up < 1 || n_up > n_down) return false;                       // n_upsample = 0 drops the last convolution: not implemented
    if (ngf < 8 || (ngf & (ngf - 1)) || (ngf << n_down) > 1024) return false;
    const int h = H >> ds, w = W >> ds;
    return h >= 1 && w >= 1 && (int64_t)V * h * w * ngf < (1ll << 30);
}
// ResBlkEncoder.forward (src/utils.py:216-247) with norm = "instance"
void tex_walk(Ctx& c, int ngf, int n_down, int n_blocks, int n_up, int out_ch, float* feat) {
    const int h = c.Hraw >> c.ds, w = c.Wraw >> c.ds;
    View im{0, nullptr, h, w, 3, 3};
    View t = c.alloc(h, w, ngf);
    c.conv(ConvSpec{3, ngf, 7, 7, 1, 3, 1, 0, 1}, im, -1, 0, t, nullptr, 0, 1);
    c.stage("stem", t);
    int64_t ss = c.stats(t, t.C, 0);
    for (int i = 0; i < n_down; ++i) {
        View t2 = c.alloc((t.H - 1) / 2 + 1, (t.W - 1) / 2 + 1, t.C * 2);
        c.conv(ConvSpec{t.C, t.C * 2, 3, 3, 2, 1, 0, 0, 1}, t, ss, 1, t2, nullptr, 0);
        c.free_ss(ss, t.C);
        c.release(t);
        t = t2;
        char nm[16]; snprintf(nm, sizeof nm, "down%d", i + 1); c.stage(nm, t);
        ss = c.stats(t, t.C, 0);
    }
    View x = c.alloc(t.H, t.W, t.C);
    c.affine(t, ss, 1, nullptr, x);
    c.free_ss(ss, t.C);
    c.release(t);
    const int C = x.C;
    for (int b = 0; b < n_blocks; ++b) {                                // ResBlk: x + layers(x)
        View y1 = c.alloc(x.H, x.W, C);
        c.conv(ConvSpec{C, C, 3, 3, 1, 1, 1, 0, 1}, x, -1, 0, y1, nullptr, 0);
        ss = c.stats(y1, C, 0);
        View y2 = c.alloc(x.H, x.W, C);
        c.conv(ConvSpec{C, C, 3, 3, 1, 1, 1, 0, 1}, y1, ss, 1, y2, nullptr, 0);
        c.free_ss(ss, C);
        c.release(y1);
        ss = c.stats(y2, C, 0);
        c.affine(y2, ss, 0, &x, y2);
        c.free_ss(ss, C);
        c.release(x);
        x = y2;
        char nm[16]; snprintf(nm, sizeof nm, "res%d", b + 1); c.stage(nm, x);
    }
    t = x;
    ss = -1;
    for (int i = 0; i < n_up; ++i) {
        View t2 = c.alloc(t.H * 2, t.W * 2, t.C / 2);
        c.conv(ConvSpec{t.C, t.C / 2, 3, 3, 2, 1, 0, 1, 1}, t, ss, ss >= 0, t2, nullptr, 0);
        if (ss >= 0) c.free_ss(ss, t.C);
        c.release(t);
        t = t2;
        char nm[16]; snprintf(nm, sizeof nm, "up%d", i + 1); c.stage(nm, t);
        ss = c.stats(t, t.C, 0);
    }
    View out{0, feat, t.H, t.W, out_ch, out_ch};
    c.conv(ConvSpec{t.C, out_ch, 7, 7, 1, 3, 1, 0, 1}, t, ss, 1, out, nullptr, 0);
    c.free_ss(ss, t.C);
    c.release(t);
}
Ctx geo_count(int V, int H, int W, int ds, int out_ch, int out_ch_hd) {
    Ctx c; c.nimg = V; c.Hraw = H; c.Wraw = W; c.ds = ds;
    geo_walk(c, out_ch, out_ch_hd, nullptr, nullptr);
    return c;
}
Ctx tex_count(int V, int H, int W, int ds, int ngf, int n_down, int n_blocks, int n_up, int out_ch) {
    Ctx c; c.nimg = V; c.Hraw = H; c.Wraw = W; c.ds = ds;
    tex_walk(c, ngf, n_down, n_blocks, n_up, out_ch, nullptr);
    return c;
}
int stage_info(const Ctx& c, int index, char* name, int cap, int64_t* offset, int32_t* dims) {
    if (index < 0 || index >= (int)c.stage_list.size() || !name || cap < 1 || !offset || !dims) return KPN_EINVAL;
    const StageInfo& s = c.stage_list[index];
    snprintf(name, (size_t)cap, "%s", s.name.c_str());
    *offset = s.off;
    dims[0] = c.nimg; dims[1] = s.H; dims[2] = s.W; dims[3] = s.C;
    return KPN_OK;
}
}  // namespace enc

extern "C" size_t kpn_geo_encoder_plain_floats(int32_t out_ch, int32_t out_ch_hd) {
    return enc::geo_shape_ok(1, 64, 64, 0, out_ch, out_ch_hd) ? (size_t)enc::geo_count(1, 64, 64, 0, out_ch, out_ch_hd).plain_off : 0;
}
extern "C" size_t kpn_geo_encoder_packed_floats(int32_t out_ch, int32_t out_ch_hd) {
    return enc::geo_shape_ok(1, 64, 64, 0, out_ch, out_ch_hd) ? (size_t)enc::geo_count(1, 64, 64, 0, out_ch, out_ch_hd).packed_off : 0;
}
extern "C" int kpn_geo_encoder_pack_device(const float* plain, float* packed, int32_t out_ch, int32_t out_ch_hd, void* stream) {
    KPN_REQUIRE(plain && packed, "null pointer");
    KPN_REQUIRE(((uintptr_t)packed & 15) == 0, "packed must be 16-byte aligned");
    KPN_REQUIRE(enc::geo_shape_ok(1, 64, 64, 0, out_ch, out_ch_hd), "out_ch / out_ch_hd must be in 1 .. 512");
    enc::Ctx c; c.mode = enc::PACK; c.nimg = 1; c.Hraw = 64; c.Wraw = 64; c.plain = plain; c.packed = packed; c.stream = stream;
    enc::geo_walk(c, out_ch, out_ch_hd, nullptr, nullptr);
    if (c.copy_err != hipSuccess) return fail(KPN_ELAUNCH, std::string("encoder: device copy failed: ") + hipGetErrorString(c.copy_err));
    return check_launch("kpn_geo_encoder_pack_device");
}
extern "C" size_t kpn_geo_encoder_workspace_bytes(int32_t V, int32_t H, int32_t W, int32_t ds, int32_t out_ch, int32_t out_ch_hd) {
    return enc::geo_shape_ok(V, H, W, ds, out_ch, out_ch_hd) ? (size_t)enc::geo_count(V, H, W, ds, out_ch, out_ch_hd).high * sizeof(float) : 0;
}
extern "C" size_t kpn_geo_encoder_stage_floats(int32_t V, int32_t H, int32_t W, int32_t ds, int32_t out_ch, int32_t out_ch_hd) {
    return enc::geo_shape_ok(V, H, W, ds, out_ch, out_ch_hd) ? (size_t)enc::geo_count(V, H, W, ds, out_ch, out_ch_hd).stage_off : 0;
}
extern "C" int kpn_geo_encoder_stage_info(int32_t V, int32_t H, int32_t W, int32_t ds, int32_t out_ch, int32_t out_ch_hd, int32_t index,
                                          char* name, int32_t name_cap, int64_t* offset, int32_t* dims) {
    KPN_REQUIRE(enc::geo_shape_ok(V, H, W, ds, out_ch, out_ch_hd), "geometry encoder: (H >> ds) and (W >> ds) must be multiples of 64");
    return enc::stage_info(enc::geo_count(V, H, W, ds, out_ch, out_ch_hd), index, name, name_cap, offset, dims);
}
extern "C" int kpn_geo_encode(const float* img, int32_t V, int32_t H, int32_t W, int32_t ds, int32_t out_ch, int32_t out_ch_hd,
                              const float* packed, float eps, float* feat, float* feat_hd, float* stages, void* workspace,
                              size_t workspace_bytes, void* stream) {
    KPN_REQUIRE(img && packed && feat && feat_hd && workspace, "null pointer");
    KPN_REQUIRE(enc::geo_shape_ok(V, H, W, ds, out_ch, out_ch_hd),
                "geometry encoder: (H >> ds) and (W >> ds) must be multiples of 64 (stem stride 2, avg-pool 2, four hourglass levels)");
    KPN_REQUIRE(((uintptr_t)packed & 15) == 0 && ((uintptr_t)workspace & 15) == 0, "packed / workspace must be 16-byte aligned");
    KPN_REQUIRE(workspace_bytes >= (size_t)enc::geo_count(V, H, W, ds, out_ch, out_ch_hd).high * sizeof(float),
                "workspace too small (kpn_geo_encoder_workspace_bytes)");
    enc::Ctx c; c.mode = enc::RUN; c.nimg = V; c.Hraw = H; c.Wraw = W; c.ds = ds; c.eps = eps; c.img = img;
    c.packed = const_cast<float*>(packed); c.ws = static_cast<float*>(workspace); c.stages = stages; c.stream = stream;
    enc::geo_walk(c, out_ch, out_ch_hd, feat, feat_hd);
    if (c.copy_err != hipSuccess) return fail(KPN_ELAUNCH, std::string("encoder: device copy failed: ") + hipGetErrorString(c.copy_err));
    return check_launch("kpn_geo_encode");
}

extern "C" size_t kpn_tex_encoder_plain_floats(int32_t ngf, int32_t n_down, int32_t n_blocks, int32_t n_up, int32_t out_ch) {
    return enc::tex_shape_ok(1, 8, 8, 0, ngf, n_down, n_blocks, n_up, out_ch) ? (size_t)enc::tex_count(1, 8, 8, 0, ngf, n_down, n_blocks, n_up, out_ch).plain_off : 0;
}
extern "C" size_t kpn_tex_encoder_packed_floats(int32_t ngf, int32_t n_down, int32_t n_blocks, int32_t n_up, int32_t out_ch) {
    return enc::tex_shape_ok(1, 8, 8, 0, ngf, n_down, n_blocks, n_up, out_ch) ? (size_t)enc::tex_count(1, 8, 8, 0, ngf, n_down, n_blocks, n_up, out_ch).packed_off : 0;
}
extern "C" int kpn_tex_encoder_pack_device(const float* plain, float* packed, int32_t ngf, int32_t n_down, int32_t n_blocks, int32_t n_up,
                                           int32_t out_ch, void* stream) {
    KPN_REQUIRE(plain && packed, "null pointer");
    KPN_REQUIRE(((uintptr_t)packed & 15) == 0, "packed must be 16-byte aligned");
    KPN_REQUIRE(enc::tex_shape_ok(1, 8, 8, 0, ngf, n_down, n_blocks, n_up, out_ch), "texture encoder: ngf a power of two >= 8, 1 <= n_upsample <= n_downsample <= 5");
    enc::Ctx c; c.mode = enc::PACK; c.nimg = 1; c.Hraw = 8; c.Wraw = 8; c.plain = plain; c.packed = packed; c.stream = stream;
    enc::tex_walk(c, ngf, n_down, n_blocks, n_up, out_ch, nullptr);
    if (c.copy_err != hipSuccess) return fail(KPN_ELAUNCH, std::string("encoder: device copy failed: ") + hipGetErrorString(c.copy_err));
    return check_launch("kpn_tex_encoder_pack_device");
}
extern "C" size_t kpn_tex_encoder_workspace_bytes(int32_t V, int32_t H, int32_t W, int32_t ds, int32_t ngf, int32_t n_down, int32_t n_blocks,
                                                  int32_t n_up, int32_t out_ch) {
    return enc::tex_shape_ok(V, H, W, ds, ngf, n_down, n_blocks, n_up, out_ch)
               ? (size_t)enc::tex_count(V, H, W, ds, ngf, n_down, n_blocks, n_up, out_ch).high * sizeof(float) : 0;
}
extern "C" size_t kpn_tex_encoder_stage_floats(int32_t V, int32_t H, int32_t W, int32_t ds, int32_t ngf, int32_t n_down, int32_t n_blocks,
                                               int32_t n_up, int32_t out_ch) {
    return enc::tex_shape_ok(V, H, W, ds, ngf, n_down, n_blocks, n_up, out_ch)
               ? (size_t)enc::tex_count(V, H, W, ds, ngf, n_down, n_blocks, n_up, out_ch).stage_off : 0;
}
extern "C" int kpn_tex_encoder_stage_info(int32_t V, int32_t H, int32_t W, int32_t ds, int32_t ngf, int32_t n_down, int32_t n_blocks, int32_t n_up,
                                          int32_t out_ch, int32_t index, char* name, int32_t name_cap, int64_t* offset, int32_t* dims) {
    KPN_REQUIRE(enc::tex_shape_ok(V, H, W, ds, ngf, n_down, n_blocks, n_up, out_ch), "texture encoder: unsupported size or arguments");
    return enc::stage_info(enc::tex_count(V, H, W, ds, ngf, n_down, n_blocks, n_up, out_ch), index, name, name_cap, offset, dims);
}
extern "C" int kpn_tex_encode(const float* img, int32_t V, int32_t H, int32_t W, int32_t ds, int32_t ngf, int32_t n_down, int32_t n_blocks,
                              int32_t n_up, int32_t out_ch, const float* packed, float eps, float* feat, float* stages, void* workspace,
                              size_t workspace_bytes, void* stream) {
    KPN_REQUIRE(img && packed && feat && workspace, "null pointer");
    KPN_REQUIRE(enc::tex_shape_ok(V, H, W, ds, ngf, n_down, n_blocks, n_up, out_ch),
                "texture encoder: ngf a power of two >= 8, 1 <= n_upsample <= n_downsample <= 5, (H >> ds) and (W >> ds) >= 1");
    KPN_REQUIRE(((uintptr_t)packed & 15) == 0 && ((uintptr_t)workspace & 15) == 0, "packed / workspace must be 16-byte aligned");
    KPN_REQUIRE(workspace_bytes >= (size_t)enc::tex_count(V, H, W, ds, ngf, n_down, n_blocks, n_up, out_ch).high * sizeof(float),
                "workspace too small (kpn_tex_encoder_workspace_bytes)");
    enc::Ctx c; c.mode = enc::RUN; c.nimg = V; c.Hraw = H; c.Wraw = W; c.ds = ds; c.eps = eps; c.img = img;
    c.packed = const_cast<float*>(packed); c.ws = static_cast<float*>(workspace); c.stages = stages; c.stream = stream;
    enc::tex_walk(c, ngf, n_down, n_blocks, n_up, out_ch, feat);
    if (c.copy_err != hipSuccess) return fail(KPN_ELAUNCH, std::string("encoder: device copy failed: ") + hipGetErrorString(c.copy_err));
    return check_launch("kpn_tex_encode");
}

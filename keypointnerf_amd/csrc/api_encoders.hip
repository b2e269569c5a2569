// ---------------------------------------------------------------------------------------------
// The image encoders, HGFilterV2 and ResBlkEncoder (reference src/utils.py:199-474), forward.  Kernels: encoder_kernels.hip.
// Each network is written once, as a walk over its layers (enc::geo_walk / enc::tex_walk) that a context runs in one of
// three modes: COUNT (sizes of the plain and packed parameter vectors, the workspace and the stage buffer), PACK (launch the
// packers) and RUN (launch the forward).  The order in which a walk asks for parameters defines the plain layout
// (keypointnerf_amd/encoders.py builds it from the caller's module in the same order).
namespace enc {
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

    static int tile_n(int cout) { return cout > 32 ? 64 : 32; }
    // split K by the per-image geometry only: an image's result must not depend on how many images are encoded with it
    // (api_conv.hip splits its single layers by the same rule)
    static int ksplit_of(int Ho, int Wo, int bm, int bn, int cout_p, int ncls, int nkmin) {
        const int64_t tiles_img = ((int64_t)Ho * Wo + bm - 1) / bm * (cout_p / bn) * ncls;
        int ksplit = 1;
        if (tiles_img < 128) ksplit = (int)std::min<int64_t>(std::min(nkmin, 16), (256 + tiles_img - 1) / tiles_img);
        return ksplit < 1 ? 1 : ksplit;
    }
    static int taps_of(const ConvSpec& s, int cls) { return s.deconv ? (1 + (cls >> 1)) * (1 + (cls & 1)) : s.kh * s.kw; }

    // src: the stem reads `img` instead (stem != 0).  ss: offset of scale / shift in the workspace or -1
    void conv(const ConvSpec& s, const View& src, int64_t ss, int relu_in, const View& dst, const View* res, int relu_out, int stem = 0) {
        const int bn = tile_n(s.cout), bm = bn == 64 ? 64 : 128;
        kpn_enc_conv_args a{};
        a.cin = s.cin; a.cin_p = (s.cin + 3) / 4 * 4;
        a.cout = s.cout; a.cout_p = (s.cout + bn - 1) / bn * bn;
        const int ncls = s.deconv ? 4 : 1;
        int64_t wtotal = 0;
        int nkmin = 1 << 30;
        for (int c = 0; c < ncls; ++c) {
            a.nk[c] = (taps_of(s, c) * a.cin_p + 15) / 16;
            a.wofs[c] = wtotal;
            wtotal += (int64_t)a.nk[c] * a.cout_p * 16;
            if (a.nk[c] < nkmin) nkmin = a.nk[c];
        }
        // parameters: weight, then bias
        const float* wp = packed ? packed + packed_off : nullptr;
        if (mode == PACK)
            for (int c = 0; c < ncls; ++c) {
                kpn_enc_pack_args pa{plain + plain_off, packed + packed_off + a.wofs[c], s.cin, a.cin_p, s.cout, a.cout_p, s.kh, s.kw, a.nk[c], s.deconv, c};
                const int64_t n = (int64_t)a.nk[c] * a.cout_p * 16;
                KPN_LAUNCH(k_enc_pack, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 4096)), dim3(256), stream, pa);
            }
        plain_off += (int64_t)s.cout * s.cin * s.kh * s.kw;
        packed_off += wtotal;
        const float* bias = s.bias ? vec(s.cout) : nullptr;
        // geometry
        a.nimg = nimg;
        a.Hs = src.H; a.Ws = src.W;
        if (s.deconv) { a.Ho = src.H; a.Wo = src.W; }
        else { a.Ho = dst.H; a.Wo = dst.W; }
        a.kh = s.kh; a.kw = s.kw; a.stride = s.stride; a.pad = s.pad; a.replicate = s.replicate;
        const int ksplit = ksplit_of(a.Ho, a.Wo, bm, bn, a.cout_p, ncls, nkmin);
        a.ksplit = ksplit;
        const int64_t M = (int64_t)nimg * a.Ho * a.Wo;
        const int64_t part = ksplit > 1 ? (int64_t)ncls * ksplit * M * a.cout_p : 0;
        const int64_t poff = part ? alloc_raw(part) : 0;
        if (mode == RUN) {
            a.src = stem ? img : ptr(src);
            a.src_cs = src.cs; a.Hraw = Hraw; a.Wraw = Wraw; a.ds = ds;
            a.ss = ss >= 0 ? ws + ss : nullptr;
            a.relu_in = relu_in;
            a.wp = wp; a.bias = bias;
            a.dst = ptr(dst); a.dst_cs = dst.cs;
            a.res = res ? ptr(*res) : nullptr; a.res_cs = res ? res->cs : 0;
            a.relu_out = relu_out;
            a.partial = part ? ws + poff : nullptr;
            const dim3 grid((unsigned)((M + bm - 1) / bm * (a.cout_p / bn)), (unsigned)ksplit, (unsigned)ncls);
            if (stem) {
                if (bn == 64) KPN_LAUNCH((k_enc_conv<64, 64, true, false>), grid, dim3(256), stream, a);
                else KPN_LAUNCH((k_enc_conv<128, 32, true, false>), grid, dim3(256), stream, a);
            } else if (s.deconv) {
                if (bn == 64) KPN_LAUNCH((k_enc_conv<64, 64, false, true>), grid, dim3(256), stream, a);
                else KPN_LAUNCH((k_enc_conv<128, 32, false, true>), grid, dim3(256), stream, a);
            } else {
                if (bn == 64) KPN_LAUNCH((k_enc_conv<64, 64, false, false>), grid, dim3(256), stream, a);
                else KPN_LAUNCH((k_enc_conv<128, 32, false, false>), grid, dim3(256), stream, a);
            }
            if (ksplit > 1) {
                const int64_t n = (int64_t)ncls * M * a.cout;
                KPN_LAUNCH(k_enc_combine, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 8192)), dim3(256), stream, a, (int)s.deconv);
            }
        }
        if (part) release_raw(poff, part);
    }
    // GroupNorm(G, C) (affine) or InstanceNorm2d (G = C, no affine) statistics of x -> offset of scale / shift
    int64_t stats(const View& x, int G, int affine) {
        const float* gamma = affine ? vec(x.C) : nullptr;
        const float* beta = affine ? vec(x.C) : nullptr;
        const int HW = x.H * x.W;
        const int nchunks = std::max(1, std::min(64, HW / 256));
        const int64_t ss = alloc_raw((int64_t)2 * nimg * x.C);
        const int64_t pn = (int64_t)nimg * nchunks * x.C * 2 * 2;        // doubles, counted in floats
        const int64_t po = alloc_raw(pn);
        if (mode == RUN) {
            kpn_enc_stats_args a{};
            a.src = ptr(x); a.cs = x.cs; a.C = x.C; a.HW = HW; a.nchunks = nchunks; a.nimg = nimg;
            a.partial = reinterpret_cast<double*>(ws + po);
            a.G = G; a.gamma = gamma; a.beta = beta; a.eps = eps; a.ss = ws + ss;
            KPN_LAUNCH(k_enc_stats_partial, dim3((unsigned)nchunks, (unsigned)nimg), dim3(256), stream, a);
            KPN_LAUNCH(k_enc_stats_final, dim3((unsigned)((nimg * G + 63) / 64)), dim3(64), stream, a);
        }
        release_raw(po, pn);
        return ss;
    }
    void free_ss(int64_t ss, int C) { release_raw(ss, (int64_t)2 * nimg * C); }
    void affine(const View& src, int64_t ss, int relu, const View* res, const View& dst) {
        if (mode != RUN) return;
        const int64_t n = (int64_t)nimg * src.H * src.W * src.C / 4;
        KPN_LAUNCH(k_enc_affine, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 8192)), dim3(256), stream, (const float*)ptr(src),
                   (const float*)(ss >= 0 ? ws + ss : nullptr), relu, (const float*)(res ? ptr(*res) : nullptr), ptr(dst), nimg, src.H * src.W, src.C);
    }
    View pool(const View& x) {
        View o = alloc(x.H / 2, x.W / 2, x.C);
        if (mode == RUN) {
            const int64_t n = (int64_t)nimg * o.H * o.W * o.C / 4;
            KPN_LAUNCH(k_enc_pool2, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 8192)), dim3(256), stream, (const float*)ptr(x), ptr(o), nimg, o.H, o.W, o.C);
        }
        return o;
    }
    void upadd(const View& low, const View& up) {
        if (mode != RUN) return;
        const int64_t n = (int64_t)nimg * up.H * up.W * up.C / 4;
        KPN_LAUNCH(k_enc_upadd, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 8192)), dim3(256), stream, (const float*)ptr(low), (const float*)ptr(up), ptr(up), nimg,
                   low.H, low.W, low.C);
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

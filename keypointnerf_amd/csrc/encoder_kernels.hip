// encoder_kernels.hip — forward of the two image encoders in front of the ray march, HGFilterV2 (geometry) and ResBlkEncoder
// (texture) of the reference (src/utils.py:199-474, called from attach_geo_feat / attach_tex_feat, src/model.py:653-680), on the
// fp32 MFMA (v_mfma_f32_32x32x2_f32: exact fp32 products, fp32 accumulation).
//
// One convolution family, k_enc_conv: implicit GEMM  out[pixel][co] = sum_k A[pixel][k] * Wp[k][co]  over NHWC activations with
// k = tap * cin_p + ci (cin_p = cin rounded up to 4, so the 3-channel stems pack four taps into one 16-wide K chunk).  A
// workgroup of four wavefronts computes BM x BN outputs (64 x 64, or 128 x 32 for layers with at most 32 output channels), one
// 32 x 32 accumulator per wavefront.  Per K chunk of 16 every thread loads one or two float4s of A and one of the packed
// weights, the workgroup stages them in LDS (k-major: the lanes of an MFMA operand read consecutive floats of one row) and issues
// eight MFMAs; the loads of chunk s + 1 are in flight while chunk s is multiplied.
//   loads    : zero padding or replication padding (a clamp of the source coordinate), stride 1 / 2; per (image, channel)
//              scale * x + shift with optional ReLU (GroupNorm / InstanceNorm + ReLU in front of the convolution); the stems read
//              the NCHW images, average 2 x 2 blocks when ds = 1 (the avg_pool2d of attach_*_feat; the host admits ds <= 1) and apply
//              2 * im - 1 (stem_plain = 0, the walks) or nothing (stem_plain = 1, a module's own stem layer);
//   RPADJ    : the input gradient of a replication-padded stride-1 convolution: the adjoint of the clamped load, the sum of dy over
//              the positions that the clamp maps onto the pixel (kpn_enc_load_a_rp_adjoint) - a gather, no scatter;
//   DECONV   : ConvTranspose2d(k = 3, stride = 2, padding = 1, output_padding = 1) as four gathers, one per output parity
//              (py, px) with (1 + py) * (1 + px) valid taps each (blockIdx.z) — no scatter;
//   epilogue : bias, residual add from a second tensor, ReLU, store into a channel slice of a wider NHWC tensor;
//   split K  : layers with few pixels split the K chunks over blockIdx.y; the partial tiles go to scratch and k_enc_combine adds
//              them in split order and runs the epilogue.  The split depends on the per-image geometry only.
// Beside it: k_enc_stats_partial / k_enc_stats_final (GroupNorm / InstanceNorm statistics in fp64 partial sums, reduced in a
// fixed order and folded with gamma / beta into the scale / shift the next loads use), k_enc_affine (normalise [+ ReLU]
// [+ residual] where the value is needed as a tensor), k_enc_add_cs (the sum of two channel slices), k_enc_norm_bwd_partial / _final / _dx (the gradient of statistics +
// affine, api_norm.hip), k_enc_pool2 / k_enc_pool2_bwd (avg_pool2d(x, 2, 2) and its gradient; k_enc_pool2_bwd_acc adds that gradient onto a
// finished one: the fan-in sums of api_geo_train.hip), k_enc_upadd (bicubic x2,
// align_corners = True, ATen's coefficients with A = -0.75 and clamped taps, fused with the up1 + up2 add of HourGlass._forward;
// out of place or in place, with or without the added tensor), k_enc_up2_bwd (its gradient with respect to the low tensor, a gather
// with the forward's own weights; api_resample.hip) and k_enc_pack.  No float
// atomics; every reduction has a fixed order, so results are bit-reproducible and independent of the position of an image in
// the batch.

struct kpn_enc_conv_args {
    int nimg, Ho, Wo;          // GEMM rows = nimg * Ho * Wo.  DECONV: (Ho, Wo) is the source grid, row (y, x) of class (py, px)
                               // writes output pixel (2y + py, 2x + px) of the (2 Ho, 2 Wo) result
    int Hs, Ws;                // source size (STEM: after the 2^ds average)
    int cin, cin_p;            // source channels; cin_p = cin rounded up to 4
    int kh, kw, stride, pad, replicate;
    int nk[4];                 // K chunks of 16 (DECONV: per parity class, else nk[0])
    int64_t wofs[4];           // DECONV: offset (floats) of the class's packed weights
    int ksplit;                // number of K ranges (gridDim.y)
    const float* src;          // NHWC, pointer at the first channel of the slice; STEM: NCHW (nimg, cin, Hraw, Wraw)
    int src_cs;                // channel stride of a source pixel
    int Hraw, Wraw, ds;        // STEM
    int stem_plain;            // STEM: 0 = the walks' raw images in [0, 1], loaded as 2 * im - 1; 1 = an already normalised tensor,
                               // loaded as it is (a module's own stem layer, api_strided.hip)
    const float* ss;           // scale [nimg][cin] then shift [nimg][cin], or NULL
    int relu_in;
    const float* wp;           // packed [chunk][cout_p][16]
    int cout, cout_p;
    const float* bias;         // or NULL
    float* dst;                // NHWC, pointer at the first channel of the slice
    int dst_cs;
    const float* res;          // or NULL; same pixel grid as dst
    int res_cs;
    int relu_out;
    float* partial;            // ksplit > 1: [class][split][row][cout_p]
};

__device__ __forceinline__ void kpn_enc_epilogue(const kpn_enc_conv_args& a, int cls, int64_t q, int co, float v, bool deconv) {
    int64_t dq = q;
    if (deconv) {
        const int hw = a.Ho * a.Wo;
        const int n = (int)(q / hw), r = (int)(q % hw);
        const int y = r / a.Wo, x = r % a.Wo;
        dq = ((int64_t)n * 2 * a.Ho + 2 * y + (cls >> 1)) * (2 * a.Wo) + 2 * x + (cls & 1);
    }
    if (a.bias) v = KADD(v, a.bias[co]);
    if (a.res) v = KADD(v, a.res[dq * a.res_cs + co]);
    if (a.relu_out) v = v > 0.0f ? v : 0.0f;
    a.dst[dq * a.dst_cs + co] = v;
}

// four consecutive K entries (one tap, channels [c, c + 4)) of GEMM row (n, oy, ox)
template <bool STEM, bool DECONV>
__device__ __forceinline__ kpn_f32x4 kpn_enc_load_a(const kpn_enc_conv_args& a, int cls, bool valid, int n, int oy, int ox, int kk) {
    kpn_f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    const int tap = kk / a.cin_p, c = kk - tap * a.cin_p;
    int sy, sx;
    if constexpr (DECONV) {
        const int py = cls >> 1, px = cls & 1;
        const int ntx = 1 + px;
        const int ty = tap / ntx, tx = tap - ty * ntx;
        if (ty > py) valid = false;                     // K padding behind the last tap
        sy = oy + (py ? 1 - ty : 0);
        sx = ox + (px ? 1 - tx : 0);
    } else {
        const int ky = tap / a.kw, kx = tap - ky * a.kw;
        if (ky >= a.kh) valid = false;
        sy = oy * a.stride - a.pad + ky;
        sx = ox * a.stride - a.pad + kx;
        if (a.replicate) {
            sy = sy < 0 ? 0 : (sy >= a.Hs ? a.Hs - 1 : sy);
            sx = sx < 0 ? 0 : (sx >= a.Ws ? a.Ws - 1 : sx);
        }
    }
    if (!valid || sy < 0 || sy >= a.Hs || sx < 0 || sx >= a.Ws) return v;
    if constexpr (STEM) {
        const int f = 1 << a.ds;
        const float inv = 1.0f / (float)(f * f);
        for (int e = 0; e < 4; ++e) {
            if (c + e >= a.cin) break;
            const float* p = a.src + (((size_t)n * a.cin + c + e) * a.Hraw + (size_t)sy * f) * a.Wraw + (size_t)sx * f;
            float s = 0.0f;
            for (int j = 0; j < f; ++j)
                for (int i = 0; i < f; ++i) s = KADD(s, p[(size_t)j * a.Wraw + i]);
            const float m = KMUL(s, inv);
            v[e] = a.stem_plain ? m : KSUB(KMUL(2.0f, m), 1.0f);
        }
    } else {
        v = *KPN_GLOBAL4(a.src + (((size_t)n * a.Hs + sy) * a.Ws + sx) * a.src_cs + c);
        if (a.ss) {
            const kpn_f32x4 sc = *KPN_GLOBAL4(a.ss + (size_t)n * a.cin + c);
            const kpn_f32x4 sh = *KPN_GLOBAL4(a.ss + ((size_t)a.nimg + n) * a.cin + c);
            for (int e = 0; e < 4; ++e) v[e] = fmaf(v[e], sc[e], sh[e]);
        }
        if (a.relu_in)
            for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.0f ? v[e] : 0.0f;
    }
    return v;
}

// The adjoint of the clamped load: the A entry of the input gradient of a replication-padded stride-1 convolution with an odd
// kernel and pad = k / 2 (api_reppad.hip).  GEMM row (n, y, x) is an input pixel, K entry (tap', co) with tap' = (ky', kx') counted as
// the flipped packed copy counts it (ky = kh - 1 - ky'), the source is dy on the same (Hs, Ws) grid.  The forward read
// x[clamp(o + ky - pad)], so dx[y] collects every dy[oy] with clamp(oy + ky - pad, 0, Hs - 1) == y: for an interior y the one position
// y + ky' - pad (the zero-padded gradient's), for y = 0 everything up to it, for y = Hs - 1 everything from it on - one contiguous range
// per axis, at most pad + 1 long, and only on the outermost ring.  The rectangle is added oy outer, ox inner: a gather in a fixed order.
__device__ __forceinline__ void kpn_enc_rp_range(int y, int base, int n, int& lo, int& hi) {
    lo = y == 0 ? 0 : base;
    hi = y == n - 1 ? n - 1 : base;
    lo = lo < 0 ? 0 : lo;
    hi = hi > n - 1 ? n - 1 : hi;
}
__device__ __forceinline__ kpn_f32x4 kpn_enc_load_a_rp_adjoint(const kpn_enc_conv_args& a, bool valid, int n, int y, int x, int kk) {
    kpn_f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    const int tap = kk / a.cin_p, c = kk - tap * a.cin_p;
    const int ky = tap / a.kw, kx = tap - ky * a.kw;
    if (!valid || ky >= a.kh) return v;
    int y0, y1, x0, x1;
    kpn_enc_rp_range(y, y + ky - a.pad, a.Hs, y0, y1);
    kpn_enc_rp_range(x, x + kx - a.pad, a.Ws, x0, x1);
    if (y0 > y1 || x0 > x1) return v;
    // the first value is loaded as the plain load loads it, with nothing consuming it before the next chunk's LDS store: an interior
    // pixel, and a wavefront without a ring pixel, pays nothing for the mode.  Only a ring pixel with more values enters the loop, whose
    // adds wait for their loads
    v = *KPN_GLOBAL4(a.src + (((size_t)n * a.Hs + y0) * a.Ws + x0) * a.src_cs + c);
    if (y1 > y0 || x1 > x0)
        for (int sy = y0; sy <= y1; ++sy)
            for (int sx = sy == y0 ? x0 + 1 : x0; sx <= x1; ++sx) {
                const kpn_f32x4 d = *KPN_GLOBAL4(a.src + (((size_t)n * a.Hs + sy) * a.Ws + sx) * a.src_cs + c);
                for (int e = 0; e < 4; ++e) v[e] = KADD(v[e], d[e]);
            }
    return v;
}

// RPADJ: the A loads are kpn_enc_load_a_rp_adjoint (STEM and DECONV off); everything else is the same GEMM
template <int BM, int BN, bool STEM, bool DECONV, bool RPADJ = false>
__global__ __launch_bounds__(256) void k_enc_conv(kpn_enc_conv_args a) {
    static_assert(!RPADJ || (!STEM && !DECONV), "the adjoint load is a mode of the plain NHWC GEMM");
    static_assert((BM / 32) * (BN / 32) == 4, "four wavefronts, one 32 x 32 accumulator each");
    constexpr int NA = BM * 4 / 256;        // float4s of A per thread and K chunk
    constexpr int KQ = 256 / BM;            // K quarter step between the float4s of one thread
    __shared__ float As[16][BM];
    __shared__ float Bs[16][BN];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cls = DECONV ? (int)blockIdx.z : 0;
    const int ctiles = a.cout_p / BN;
    const int ct = (int)(blockIdx.x % ctiles);
    const int64_t pt = blockIdx.x / ctiles;
    const int64_t M = (int64_t)a.nimg * a.Ho * a.Wo;
    const int hw = a.Ho * a.Wo;
    // A loads: one GEMM row per thread
    const int arow = tid % BM, akq = tid / BM;
    const int64_t p = pt * BM + arow;
    const bool valid = p < M;
    const int n = valid ? (int)(p / hw) : 0;
    const int rem = valid ? (int)(p % hw) : 0;
    const int oy = rem / a.Wo, ox = rem % a.Wo;
    // B loads
    const bool bload = tid < BN * 4;
    const int bco = tid % BN, bkq = tid / BN;
    const float* wbase = a.wp + (DECONV ? a.wofs[cls] : 0) + ((size_t)ct * BN + bco) * 16 + bkq * 4;
    const int nk = a.nk[cls];
    const int ks = (int)blockIdx.y;
    const int s0 = (int)((int64_t)ks * nk / a.ksplit), s1 = (int)((int64_t)(ks + 1) * nk / a.ksplit);
    kpn_f32x4 ra[NA], rb = {0.0f, 0.0f, 0.0f, 0.0f};
    auto load = [&](int s) {
        for (int j = 0; j < NA; ++j) {
            if constexpr (RPADJ) ra[j] = kpn_enc_load_a_rp_adjoint(a, valid, n, oy, ox, s * 16 + (akq + j * KQ) * 4);
            else ra[j] = kpn_enc_load_a<STEM, DECONV>(a, cls, valid, n, oy, ox, s * 16 + (akq + j * KQ) * 4);
        }
        if (bload) rb = *KPN_GLOBAL4(wbase + (size_t)s * a.cout_p * 16);
    };
    const int wn = wave % (BN / 32), wm = wave / (BN / 32);
    const int ai = wm * 32 + (lane & 31), bj = wn * 32 + (lane & 31), kh2 = lane >> 5;
    kpn_f32x16 acc;
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    if (s0 < s1) load(s0);
    for (int s = s0; s < s1; ++s) {
        for (int j = 0; j < NA; ++j)
            for (int e = 0; e < 4; ++e) As[(akq + j * KQ) * 4 + e][arow] = ra[j][e];
        if (bload)
            for (int e = 0; e < 4; ++e) Bs[bkq * 4 + e][bco] = rb[e];
        __syncthreads();
        if (s + 1 < s1) load(s + 1);
        for (int m = 0; m < 8; ++m)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[2 * m + kh2][ai], Bs[2 * m + kh2][bj], acc, 0, 0, 0);
        __syncthreads();
    }
    // D[row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)][col = lane & 31]: rows are pixels, columns output channels
    const int co = ct * BN + bj;
    if (co >= a.cout) return;
    for (int r = 0; r < 16; ++r) {
        const int64_t q = pt * BM + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh2;
        if (q >= M) continue;
        if (a.ksplit > 1) a.partial[(((int64_t)cls * a.ksplit + ks) * M + q) * a.cout_p + co] = acc[r];
        else kpn_enc_epilogue(a, cls, q, co, acc[r], DECONV);
    }
}

// split-K combine: the partial tiles of one output element are added in split order, then the epilogue
__global__ __launch_bounds__(256) void k_enc_combine(kpn_enc_conv_args a, int deconv) {
    const int64_t M = (int64_t)a.nimg * a.Ho * a.Wo;
    const int ncls = deconv ? 4 : 1;
    const int64_t total = (int64_t)ncls * M * a.cout;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int co = (int)(i % a.cout);
        const int64_t q = (i / a.cout) % M;
        const int cls = (int)(i / a.cout / M);
        float v = 0.0f;
        for (int ks = 0; ks < a.ksplit; ++ks) v = KADD(v, a.partial[(((int64_t)cls * a.ksplit + ks) * M + q) * a.cout_p + co]);
        kpn_enc_epilogue(a, cls, q, co, v, deconv != 0);
    }
}

// statistics, step 1: block (chunk, image) adds x and x^2 of its pixel range per channel in fp64; the threads of one channel
// quad are added in thread order.  partial [image][chunk][channel][2]
struct kpn_enc_stats_args {
    const float* src;      // NHWC slice
    int cs, C, HW, nchunks, nimg;
    double* partial;
    // step 2
    int G;                 // groups (InstanceNorm: G = C)
    const float* gamma;    // or NULL
    const float* beta;
    float eps;
    float* ss;             // scale [nimg][C] then shift [nimg][C]
    float* mr;             // or NULL: mean [nimg][G] then rstd [nimg][G], the fp64 values rounded once (kept for a backward)
};
__global__ __launch_bounds__(256) void k_enc_stats_partial(kpn_enc_stats_args a) {
    __shared__ double red[256][8];
    const int L = a.C / 4;                       // threads per pixel (a power of two, at most 256)
    const int PP = 256 / L;
    const int cl = threadIdx.x % L, pl = threadIdx.x / L;
    const int chunk = blockIdx.x, n = blockIdx.y;
    const int p0 = (int)((int64_t)chunk * a.HW / a.nchunks), p1 = (int)((int64_t)(chunk + 1) * a.HW / a.nchunks);
    double s[4] = {0.0, 0.0, 0.0, 0.0}, q[4] = {0.0, 0.0, 0.0, 0.0};
    for (int p = p0 + pl; p < p1; p += PP) {
        const kpn_f32x4 v = *KPN_GLOBAL4(a.src + ((size_t)n * a.HW + p) * a.cs + cl * 4);
        for (int e = 0; e < 4; ++e) { s[e] += (double)v[e]; q[e] += (double)v[e] * (double)v[e]; }
    }
    for (int e = 0; e < 4; ++e) { red[threadIdx.x][e] = s[e]; red[threadIdx.x][4 + e] = q[e]; }
    __syncthreads();
    if (pl == 0) {
        for (int k = 1; k < PP; ++k)
            for (int e = 0; e < 4; ++e) { s[e] += red[k * L + cl][e]; q[e] += red[k * L + cl][4 + e]; }
        double* o = a.partial + (((size_t)n * a.nchunks + chunk) * a.C + cl * 4) * 2;
        for (int e = 0; e < 4; ++e) { o[2 * e] = s[e]; o[2 * e + 1] = q[e]; }
    }
}
// s0 += p[k C][0], s1 += p[k C][1] for the chunks k = 0 .. nchunks - 1 of one (image, channel), added in chunk order.  The loads of
// sixteen chunks are issued before their adds: one thread walks up to 64 chunks, and a load per add is a latency chain
typedef double kpn_f64x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void kpn_enc_add_chunks(const double* p, int C, int nchunks, double& s0, double& s1) {
    for (int k0 = 0; k0 < nchunks; k0 += 16) {
        kpn_f64x2 v[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = *reinterpret_cast<const kpn_f64x2*>(p + (size_t)(k0 + j < nchunks ? k0 + j : k0) * C * 2);
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (k0 + j < nchunks) { s0 += v[j][0]; s1 += v[j][1]; }
    }
}
// step 2: one thread per (image, group): chunks then channels in order; biased variance; scale = gamma * rstd,
// shift = beta - mean * scale
__global__ __launch_bounds__(64) void k_enc_stats_final(kpn_enc_stats_args a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.nimg * a.G) return;
    const int n = i / a.G, g = i % a.G, cpg = a.C / a.G;
    double S = 0.0, Q = 0.0;
    for (int c = g * cpg; c < (g + 1) * cpg; ++c)
        kpn_enc_add_chunks(a.partial + ((size_t)n * a.nchunks * a.C + c) * 2, a.C, a.nchunks, S, Q);
    const double cnt = (double)a.HW * cpg;
    const double mean = S / cnt;
    double var = Q / cnt - mean * mean;
    if (var < 0.0) var = 0.0;
    const double rstd = 1.0 / sqrt(var + (double)a.eps);
    if (a.mr) { a.mr[(size_t)n * a.G + g] = (float)mean; a.mr[((size_t)a.nimg + n) * a.G + g] = (float)rstd; }
    for (int c = g * cpg; c < (g + 1) * cpg; ++c) {
        const double sc = a.gamma ? (double)a.gamma[c] * rstd : rstd;
        const double sh = (a.beta ? (double)a.beta[c] : 0.0) - mean * sc;
        a.ss[(size_t)n * a.C + c] = (float)sc;
        a.ss[((size_t)a.nimg + n) * a.C + c] = (float)sh;
    }
}

// dst = [relu](src * scale + shift) [+ res], whole NHWC tensors (n, HW, C); ss may be NULL (plain add / copy)
__global__ __launch_bounds__(256) void k_enc_affine(const float* src, const float* ss, int relu, const float* res, float* dst,
                                                    int nimg, int HW, int C) {
    const int c4 = C / 4;
    const int64_t total = (int64_t)nimg * HW * c4;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % c4) * 4;
        const int n = (int)(i / c4 / HW);
        kpn_f32x4 v = *KPN_GLOBAL4(src + i * 4);
        if (ss) {
            const kpn_f32x4 sc = *KPN_GLOBAL4(ss + (size_t)n * C + c), sh = *KPN_GLOBAL4(ss + ((size_t)nimg + n) * C + c);
            for (int e = 0; e < 4; ++e) v[e] = fmaf(v[e], sc[e], sh[e]);
        }
        if (relu)
            for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.0f ? v[e] : 0.0f;
        if (res) {
            const kpn_f32x4 r = *KPN_GLOBAL4(res + i * 4);
            for (int e = 0; e < 4; ++e) v[e] = KADD(v[e], r[e]);
        }
        *reinterpret_cast<kpn_f32x4*>(dst + i * 4) = v;
    }
}

// dst[p][c] = a[p][c] + b[p][c] over M pixels of C channels, each tensor with its own channel stride: the residual add of the
// single-operator ConvBlock over the channel slices it keeps (api_block.hip).  dst may be b itself: a thread reads its float4 of b
// before it writes the same float4 of dst, and no other thread touches it
__global__ __launch_bounds__(256) void k_enc_add_cs(const float* a, int a_cs, const float* b, int b_cs, float* dst, int dst_cs, int64_t M, int C) {
    const int c4 = C / 4;
    const int64_t total = M * c4;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % c4) * 4;
        const size_t p = (size_t)(i / c4);
        const kpn_f32x4 u = *KPN_GLOBAL4(a + p * a_cs + c), r = *KPN_GLOBAL4(b + p * b_cs + c);
        kpn_f32x4 v;
        for (int e = 0; e < 4; ++e) v[e] = KADD(u[e], r[e]);
        *reinterpret_cast<kpn_f32x4*>(dst + p * dst_cs + c) = v;
    }
}

// ---- gradient of y = [relu](x * scale + shift), scale / shift / mean / rstd as k_enc_stats_final left them (api_norm.hip).
// With g = the gradient behind the ReLU (the mask is recomputed from fmaf(x, scale, shift): the forward's own bits),
// A_c = sum g and B_c = sum g x per (image, channel), ds = sum_c gamma_c B_c, db = sum_c gamma_c A_c over a group, cnt = cpg HW:
//   dx = gamma_c rstd g + c2 x + c3,   c2 = (db mean - ds) rstd^3 / cnt,   c3 = -c2 mean - db rstd / cnt
//   dgamma_c = sum_n (B_nc - mean A_nc) rstd,   dbeta_c = sum_n A_nc
// Every sum is fp64 in a fixed order (no atomics); each result is rounded once.
struct kpn_enc_norm_bwd_args {
    const float* x;        // NHWC (nimg, HW, C) with channel stride x_cs (C for a dense tensor; wider for a channel slice)
    int x_cs;
    const float* dy;       // dense, like dx
    const float* ss;       // scale [nimg][C] then shift [nimg][C]
    const float* mr;       // mean [nimg][G] then rstd [nimg][G]
    const float* gamma;    // or NULL
    int relu, C, HW, nchunks, nimg, G;
    double* partial;       // [image][chunk][channel][2]: A, B
    float* coef;           // a [nimg][C], then c2 [nimg][C], then c3 [nimg][C]; NULL: dx is not wanted
    float* dx;
    float* dgamma;         // or NULL
    float* dbeta;          // or NULL
    const float* add;      // or NULL; pass 3: dx = add + (g a + (x c2 + c3)), one fp32 add behind the expression.  (nimg, HW, C) with
    int add_cs;            // channel stride add_cs; add may be dx itself (a thread reads its float4 before it writes the same one)
};
__device__ __forceinline__ kpn_f32x4 kpn_enc_norm_g(kpn_f32x4 x, kpn_f32x4 dy, kpn_f32x4 sc, kpn_f32x4 sh, int relu) {
    kpn_f32x4 g = dy;
    if (relu)
        for (int e = 0; e < 4; ++e) g[e] = fmaf(x[e], sc[e], sh[e]) > 0.0f ? dy[e] : 0.0f;
    return g;
}
// pass 1: grid and thread mapping of k_enc_stats_partial; products in fp64
__global__ __launch_bounds__(256) void k_enc_norm_bwd_partial(kpn_enc_norm_bwd_args a) {
    __shared__ double red[256][8];
    const int L = a.C / 4;                       // threads per pixel (a power of two, at most 256)
    const int PP = 256 / L;
    const int cl = threadIdx.x % L, pl = threadIdx.x / L;
    const int chunk = blockIdx.x, n = blockIdx.y;
    const int p0 = (int)((int64_t)chunk * a.HW / a.nchunks), p1 = (int)((int64_t)(chunk + 1) * a.HW / a.nchunks);
    const kpn_f32x4 sc = *KPN_GLOBAL4(a.ss + (size_t)n * a.C + cl * 4), sh = *KPN_GLOBAL4(a.ss + ((size_t)a.nimg + n) * a.C + cl * 4);
    double s[4] = {0.0, 0.0, 0.0, 0.0}, q[4] = {0.0, 0.0, 0.0, 0.0};
    for (int p = p0 + pl; p < p1; p += 4 * PP) {          // four pixels' loads in flight, their adds in pixel order
        kpn_f32x4 v[4], d[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const size_t q = (size_t)n * a.HW + (p + j * PP < p1 ? p + j * PP : p);
            v[j] = *KPN_GLOBAL4(a.x + q * a.x_cs + cl * 4); d[j] = *KPN_GLOBAL4(a.dy + q * a.C + cl * 4);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (p + j * PP >= p1) break;
            const kpn_f32x4 g = kpn_enc_norm_g(v[j], d[j], sc, sh, a.relu);
            for (int e = 0; e < 4; ++e) { s[e] += (double)g[e]; q[e] += (double)g[e] * (double)v[j][e]; }
        }
    }
    for (int e = 0; e < 4; ++e) { red[threadIdx.x][e] = s[e]; red[threadIdx.x][4 + e] = q[e]; }
    __syncthreads();
    if (pl == 0) {
        for (int k = 1; k < PP; ++k)
            for (int e = 0; e < 4; ++e) { s[e] += red[k * L + cl][e]; q[e] += red[k * L + cl][4 + e]; }
        double* o = a.partial + (((size_t)n * a.nchunks + chunk) * a.C + cl * 4) * 2;
        for (int e = 0; e < 4; ++e) { o[2 * e] = s[e]; o[2 * e + 1] = q[e]; }
    }
}
// pass 2: thread i < nimg G serves one (image, group) - chunks then channels in order -> the coefficients of pass 3; thread
// nimg G + c serves channel c - chunks then images in order -> dgamma, dbeta.  B - mean A cancels: fp64 throughout
__global__ __launch_bounds__(64) void k_enc_norm_bwd_final(kpn_enc_norm_bwd_args a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int ng = a.nimg * a.G, cpg = a.C / a.G;
    if (i < ng) {
        if (!a.coef) return;
        const int n = i / a.G, g = i % a.G;
        const double mean = (double)a.mr[(size_t)n * a.G + g], rstd = (double)a.mr[((size_t)a.nimg + n) * a.G + g];
        double ds = 0.0, db = 0.0;
        for (int c = g * cpg; c < (g + 1) * cpg; ++c) {
            double A = 0.0, B = 0.0;
            kpn_enc_add_chunks(a.partial + ((size_t)n * a.nchunks * a.C + c) * 2, a.C, a.nchunks, A, B);
            const double gm = a.gamma ? (double)a.gamma[c] : 1.0;
            ds += gm * B; db += gm * A;
        }
        const double cnt = (double)a.HW * cpg;
        const double c2 = (db * mean - ds) * rstd * rstd * rstd / cnt;
        const double c3 = -c2 * mean - db * rstd / cnt;
        const size_t nc = (size_t)a.nimg * a.C;
        for (int c = g * cpg; c < (g + 1) * cpg; ++c) {
            a.coef[(size_t)n * a.C + c] = (float)((a.gamma ? (double)a.gamma[c] : 1.0) * rstd);
            a.coef[nc + (size_t)n * a.C + c] = (float)c2;
            a.coef[2 * nc + (size_t)n * a.C + c] = (float)c3;
        }
        return;
    }
    const int c = i - ng;
    if (c >= a.C || (!a.dgamma && !a.dbeta)) return;
    const int g = c / cpg;
    double dg = 0.0, dbt = 0.0;
    for (int n = 0; n < a.nimg; ++n) {
        double A = 0.0, B = 0.0;
        kpn_enc_add_chunks(a.partial + ((size_t)n * a.nchunks * a.C + c) * 2, a.C, a.nchunks, A, B);
        const double mean = (double)a.mr[(size_t)n * a.G + g], rstd = (double)a.mr[((size_t)a.nimg + n) * a.G + g];
        dg += (B - mean * A) * rstd;
        dbt += A;
    }
    if (a.dgamma) a.dgamma[c] = (float)dg;
    if (a.dbeta) a.dbeta[c] = (float)dbt;
}
// pass 3: dx = [add +] (g a + (x c2 + c3)), elementwise over float4s like k_enc_affine
__global__ __launch_bounds__(256) void k_enc_norm_bwd_dx(kpn_enc_norm_bwd_args a) {
    const int c4 = a.C / 4;
    const int64_t total = (int64_t)a.nimg * a.HW * c4;
    const size_t nc = (size_t)a.nimg * a.C;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % c4) * 4;
        const int n = (int)(i / c4 / a.HW);
        const size_t k = (size_t)n * a.C + c;
        const kpn_f32x4 v = *KPN_GLOBAL4(a.x + (size_t)(i / c4) * a.x_cs + c);
        kpn_f32x4 sc = {0.0f, 0.0f, 0.0f, 0.0f}, sh = sc;
        if (a.relu) { sc = *KPN_GLOBAL4(a.ss + k); sh = *KPN_GLOBAL4(a.ss + nc + k); }
        const kpn_f32x4 g = kpn_enc_norm_g(v, *KPN_GLOBAL4(a.dy + i * 4), sc, sh, a.relu);
        const kpn_f32x4 ca = *KPN_GLOBAL4(a.coef + k), c2 = *KPN_GLOBAL4(a.coef + nc + k), c3 = *KPN_GLOBAL4(a.coef + 2 * nc + k);
        kpn_f32x4 o;
        for (int e = 0; e < 4; ++e) o[e] = fmaf(g[e], ca[e], fmaf(v[e], c2[e], c3[e]));
        if (a.add) {
            const kpn_f32x4 r = *KPN_GLOBAL4(a.add + (size_t)(i / c4) * a.add_cs + c);
            for (int e = 0; e < 4; ++e) o[e] = KADD(r[e], o[e]);
        }
        *reinterpret_cast<kpn_f32x4*>(a.dx + i * 4) = o;
    }
}

// avg_pool2d(x, 2, stride = 2): (n, 2 Ho, 2 Wo, C) -> (n, Ho, Wo, C), rows added in window order
__global__ __launch_bounds__(256) void k_enc_pool2(const float* src, float* dst, int nimg, int Ho, int Wo, int C) {
    const int c4 = C / 4;
    const int64_t total = (int64_t)nimg * Ho * Wo * c4;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % c4) * 4;
        const int x = (int)((i / c4) % Wo), y = (int)((i / c4 / Wo) % Ho), n = (int)(i / c4 / Wo / Ho);
        const float* p = src + (((size_t)n * 2 * Ho + 2 * y) * (2 * Wo) + 2 * x) * C + c;
        const kpn_f32x4 p00 = *KPN_GLOBAL4(p), p01 = *KPN_GLOBAL4(p + C);
        const kpn_f32x4 p10 = *KPN_GLOBAL4(p + (size_t)2 * Wo * C), p11 = *KPN_GLOBAL4(p + (size_t)2 * Wo * C + C);
        kpn_f32x4 v;
        for (int e = 0; e < 4; ++e) v[e] = KMUL(KADD(KADD(KADD(p00[e], p01[e]), p10[e]), p11[e]), 0.25f);
        *reinterpret_cast<kpn_f32x4*>(dst + i * 4) = v;
    }
}

// ATen's cubic convolution coefficients (A = -0.75) for the taps at floor(s) - 1 .. floor(s) + 2
__device__ __forceinline__ void kpn_enc_cubic(float t, float (&w)[4]) {
    const float A = -0.75f;
    const float x0 = t + 1.0f, x1 = t, x2 = 1.0f - t, x3 = 2.0f - t;
    w[0] = ((A * x0 - 5.0f * A) * x0 + 8.0f * A) * x0 - 4.0f * A;
    w[1] = ((A + 2.0f) * x1 - (A + 3.0f)) * x1 * x1 + 1.0f;
    w[2] = ((A + 2.0f) * x2 - (A + 3.0f)) * x2 * x2 + 1.0f;
    w[3] = ((A * x3 - 5.0f * A) * x3 + 8.0f * A) * x3 - 4.0f * A;
}
// out (n, 2h, 2w, C) = skip + interpolate(low (n, h, w, C), scale_factor = 2, mode = 'bicubic', align_corners = True); skip = NULL:
// the interpolation alone.  out may be skip itself (the encoder walk's in-place up1 + up2): a thread reads its float4 of skip before
// it writes the same float4 of out, and no other thread touches it
__global__ __launch_bounds__(256) void k_enc_upadd(const float* low, const float* skip, float* out, int nimg, int h, int w, int C) {
    const int c4 = C / 4, Ho = 2 * h, Wo = 2 * w;
    const float sy = Ho > 1 ? (float)(h - 1) / (float)(Ho - 1) : 0.0f, sx = Wo > 1 ? (float)(w - 1) / (float)(Wo - 1) : 0.0f;
    const int64_t total = (int64_t)nimg * Ho * Wo * c4;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % c4) * 4;
        const int x = (int)((i / c4) % Wo), y = (int)((i / c4 / Wo) % Ho), n = (int)(i / c4 / Wo / Ho);
        const float fy = KMUL(sy, (float)y), fx = KMUL(sx, (float)x);
        const int iy = (int)floorf(fy), ix = (int)floorf(fx);
        float wy[4], wx[4];
        kpn_enc_cubic(KSUB(fy, (float)iy), wy);
        kpn_enc_cubic(KSUB(fx, (float)ix), wx);
        kpn_f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int j = 0; j < 4; ++j) {
            int yy = iy - 1 + j;
            yy = yy < 0 ? 0 : (yy >= h ? h - 1 : yy);
            kpn_f32x4 row = {0.0f, 0.0f, 0.0f, 0.0f};
            for (int k = 0; k < 4; ++k) {
                int xx = ix - 1 + k;
                xx = xx < 0 ? 0 : (xx >= w ? w - 1 : xx);
                const kpn_f32x4 v = *KPN_GLOBAL4(low + (((size_t)n * h + yy) * w + xx) * C + c);
                for (int e = 0; e < 4; ++e) row[e] = fmaf(v[e], wx[k], row[e]);
            }
            for (int e = 0; e < 4; ++e) acc[e] = fmaf(row[e], wy[j], acc[e]);
        }
        if (skip) {
            kpn_f32x4 u = *KPN_GLOBAL4(skip + i * 4);
            for (int e = 0; e < 4; ++e) u[e] = KADD(u[e], acc[e]);
            acc = u;
        }
        *reinterpret_cast<kpn_f32x4*>(out + i * 4) = acc;
    }
}

// gradient of k_enc_pool2: dx[n][y][x][c] = 0.25 dy[n][y / 2][x / 2][c], indexed over the high tensor (one float4 in, one out)
__global__ __launch_bounds__(256) void k_enc_pool2_bwd(const float* dy, float* dx, int nimg, int Ho, int Wo, int C) {
    const int c4 = C / 4, H = 2 * Ho, W = 2 * Wo;
    const int64_t total = (int64_t)nimg * H * W * c4;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % c4) * 4;
        const int x = (int)((i / c4) % W), y = (int)((i / c4 / W) % H), n = (int)(i / c4 / W / H);
        const kpn_f32x4 g = *KPN_GLOBAL4(dy + (((size_t)n * Ho + (y >> 1)) * Wo + (x >> 1)) * C + c);
        kpn_f32x4 v;
        for (int e = 0; e < 4; ++e) v[e] = KMUL(0.25f, g[e]);
        *reinterpret_cast<kpn_f32x4*>(dx + i * 4) = v;
    }
}

// k_enc_pool2_bwd added onto a finished gradient of the same high tensor: dst[n][y][x][c] += 0.25 dy[n][y / 2][x / 2][c].  Where a
// tensor feeds a pool and one other consumer (the input of an HourGlass level, the conv2 output of HGFilterV2) this is the fan-in sum:
// one fp32 add of two complete values, the product having the bits k_enc_pool2_bwd writes.  One float4 per thread, no atomics.
__global__ __launch_bounds__(256) void k_enc_pool2_bwd_acc(const float* dy, float* dst, int nimg, int Ho, int Wo, int C) {
    const int c4 = C / 4, H = 2 * Ho, W = 2 * Wo;
    const int64_t total = (int64_t)nimg * H * W * c4;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % c4) * 4;
        const int x = (int)((i / c4) % W), y = (int)((i / c4 / W) % H), n = (int)(i / c4 / W / H);
        const kpn_f32x4 g = *KPN_GLOBAL4(dy + (((size_t)n * Ho + (y >> 1)) * Wo + (x >> 1)) * C + c);
        kpn_f32x4 v = *KPN_GLOBAL4(dst + i * 4);
        for (int e = 0; e < 4; ++e) v[e] = KADD(v[e], KMUL(0.25f, g[e]));
        *reinterpret_cast<kpn_f32x4*>(dst + i * 4) = v;
    }
}

// The weight with which output coordinate o of k_enc_upadd reads source coordinate r along one axis (scale s, source size n): the
// forward's own fy / iy / weights, the taps that clamp onto r added in tap order.  false: o does not read r.
__device__ __forceinline__ bool kpn_enc_up2_weight(float s, int o, int r, int n, float& a) {
    const float f = KMUL(s, (float)o);
    const int i = (int)floorf(f);
    if (i < r - 2 || i > r + 1) return false;
    float wt[4];
    kpn_enc_cubic(KSUB(f, (float)i), wt);
    bool hit = false;
    a = 0.0f;
    for (int j = 0; j < 4; ++j) {
        int q = i - 1 + j;
        q = q < 0 ? 0 : (q >= n ? n - 1 : q);
        if (q == r) { a = hit ? KADD(a, wt[j]) : wt[j]; hit = true; }
    }
    return hit;
}
// The outputs that can read source coordinate r: floor(s o) in [r - 2, r + 1] with s = (n - 1) / (no - 1), i.e. o in
// [(r - 2) / s, (r + 2) / s), in integers and one coordinate wider on both sides (the rounding of s o moves floor(s o) only where
// s o is within ~1e-6 relative of an integer; one step of o moves s o by about 0.5).  n = 1: every output.  At most
// 4 (no - 1) / (n - 1) + 5 < 14 coordinates for n >= 5, and no <= 8 below that: KPN_ENC_UP2_SPAN covers every size.
#define KPN_ENC_UP2_SPAN 16
__device__ __forceinline__ void kpn_enc_up2_range(int r, int n, int no, int& lo, int& hi) {
    lo = 0; hi = no - 1;
    if (n > 1) {
        if (r > 2) lo = (int)(((int64_t)(r - 2) * (no - 1)) / (n - 1)) - 1;
        const int64_t t = ((int64_t)(r + 2) * (no - 1) + (n - 2)) / (n - 1) + 1;
        if (t < hi) hi = (int)t;
        if (lo < 0) lo = 0;
    }
}
// gradient of k_enc_upadd with respect to low, in gather form: d_low = U^T dy, one thread per float4 of the LOW tensor.  Which high
// pixels read a low pixel, and with which weight, is decided by the forward's own arithmetic (kpn_enc_up2_weight) over a widened
// range - never by an inverse formula - so no contribution is lost or doubled and the weights are the forward's bits.  The adds run
// in a fixed order: x ascending in an fmaf chain per high row, the rows ascending in a second chain.  No atomics, no LDS, no workspace.
__global__ __launch_bounds__(256) void k_enc_up2_bwd(const float* dy, float* dlow, int nimg, int h, int w, int C) {
    const int c4 = C / 4, Ho = 2 * h, Wo = 2 * w;
    const float sy = Ho > 1 ? (float)(h - 1) / (float)(Ho - 1) : 0.0f, sx = Wo > 1 ? (float)(w - 1) / (float)(Wo - 1) : 0.0f;
    const int64_t total = (int64_t)nimg * h * w * c4;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % c4) * 4;
        const int cx = (int)((i / c4) % w), r = (int)((i / c4 / w) % h), n = (int)(i / c4 / w / h);
        int x0, x1, y0, y1;
        kpn_enc_up2_range(cx, w, Wo, x0, x1);
        kpn_enc_up2_range(r, h, Ho, y0, y1);
        // the column weights do not depend on the row: once per thread, in registers (every index below is a compile-time constant)
        float ax[KPN_ENC_UP2_SPAN];
        bool on[KPN_ENC_UP2_SPAN];
#pragma unroll
        for (int k = 0; k < KPN_ENC_UP2_SPAN; ++k) {
            ax[k] = 0.0f;
            on[k] = x0 + k <= x1 && kpn_enc_up2_weight(sx, x0 + k, cx, w, ax[k]);
        }
        kpn_f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int y = y0; y <= y1; ++y) {
            float ay;
            if (!kpn_enc_up2_weight(sy, y, r, h, ay)) continue;
            const float* p = dy + (((size_t)n * Ho + y) * Wo + x0) * C + c;
            kpn_f32x4 row = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int k = 0; k < KPN_ENC_UP2_SPAN; ++k) {
                if (!on[k]) continue;
                const kpn_f32x4 v = *KPN_GLOBAL4(p + (size_t)k * C);
                for (int e = 0; e < 4; ++e) row[e] = fmaf(v[e], ax[k], row[e]);
            }
            for (int e = 0; e < 4; ++e) acc[e] = fmaf(row[e], ay, acc[e]);
        }
        *reinterpret_cast<kpn_f32x4*>(dlow + i * 4) = acc;
    }
}

// packer of one convolution: OIHW (Conv2d) or IOHW (ConvTranspose2d, parity class cls) -> [chunk][cout_p][16] with
// k = tap * cin_p + ci; everything beyond the real taps / channels is zero.  tflip: the operand of the input gradient of a
// stride-1 Conv2d, w'[ci][co][kh - 1 - ky][kw - 1 - kx] read from the same OIHW tensor (cin / cout are those of the gradient's
// GEMM: cin = the layer's output channels, cout = its input channels)
struct kpn_enc_pack_args {
    const float* w;
    float* out;
    int cin, cin_p, cout, cout_p, kh, kw, nk, deconv, cls, tflip;
};
__global__ __launch_bounds__(256) void k_enc_pack(kpn_enc_pack_args a) {
    const int64_t total = (int64_t)a.nk * a.cout_p * 16;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int e = (int)(i % 16), co = (int)((i / 16) % a.cout_p), s = (int)(i / 16 / a.cout_p);
        const int kk = s * 16 + e, tap = kk / a.cin_p, c = kk % a.cin_p;
        float v = 0.0f;
        if (co < a.cout && c < a.cin) {
            if (a.deconv) {
                const int py = a.cls >> 1, px = a.cls & 1, ntx = 1 + px;
                const int ty = tap / ntx, tx = tap % ntx;
                if (ty <= py) {
                    const int ky = py ? 2 * ty : 1, kx = px ? 2 * tx : 1;
                    v = a.w[(((size_t)c * a.cout + co) * 3 + ky) * 3 + kx];
                }
            } else if (tap < a.kh * a.kw) {
                v = a.tflip ? a.w[((size_t)c * a.cout + co) * a.kh * a.kw + (a.kh * a.kw - 1 - tap)]
                            : a.w[((size_t)co * a.cin + c) * a.kh * a.kw + tap];
            }
        }
        a.out[i] = v;
    }
}

// ---- gradients of one convolution (api_conv.hip: stride 1; api_strided.hip: stride 2, the 7 x 7 stem, ConvTranspose2d).  The input
// gradient is k_enc_conv over another packed copy of the weight.
//
// Weight gradient: dW[(tap, ci)][co] = sum over GEMM pixels of A[pixel][(tap, ci)] * R[pixel][co], A the implicit im2col row of a
// convolution (kpn_enc_load_a: the padding, stride and stem logic exists once) and R the dense tensor on that convolution's output
// grid.  A Conv2d: A from x, R = dY.  A ConvTranspose2d(k 3, s 2, p 1, op 1) is the adjoint of the stride-2 convolution that reads
// its (cin, cout, 3, 3) weight as OIHW, so the roles swap: A from dY (2H, 2W), R = x over the N H W source pixels, and the OIHW
// result is the layer's own layout.  The MFMA K dimension is the pixel index.  A workgroup of four
// wavefronts owns BM K-rows x BN output channels (64 x 64, or 128 x 32 for at most 32 output channels), one 32 x 32 accumulator per
// wavefront, and walks the 16-pixel chunks [range * cpr, (range + 1) * cpr) of blockIdx.y: both operands are staged in LDS per
// chunk (pixel-major: the lanes of an MFMA operand read consecutive floats of one pixel) with the next chunk's loads in flight.
// After every chunk the accumulator is added to an fp64 sum and cleared: no fp32 chain is longer than 16 pixels (activations behind
// a ReLU times a gradient with a mean give sums of like-signed terms, whose fp32 chains lose a digit per 100 terms).  The tile of a
// range goes, rounded to fp32, to partial[range][tap * cin + ci][co] - padded K rows and channels are never stored - and
// k_enc_wgrad_combine adds the ranges in order in fp64, rounds once and writes OIHW.  No atomics.
// The GEMM's K-rows are tap * cin_p + ci (cin_p > cin for the stems only: STEM loads the NCHW tensor through
// kpn_enc_load_a<true, false>); kpn_enc_wgrad_row maps one to its real row in `partial`, for the store and the combine alike.
struct kpn_enc_wgrad_args {
    kpn_enc_conv_args c;       // the geometry and source of A; wp, dst, partial unused.  ss with relu_in = 1: A is relu(fmaf(x, scale,
                               // shift)) computed in the loads from the un-normalised source (the legs of api_block.hip); else ss = NULL
    const float* rhs;          // R: NHWC (nimg, Ho, Wo, cout) with channel stride rhs_cs (cout for a dense tensor)
    int rhs_cs;
    const float* rhs_ss;       // scale [nimg][cout] then shift [nimg][cout] of R, or NULL: R is [relu](fmaf(rhs, scale, shift)) computed in
    int rhs_relu;              // its loads (the transposed layers of api_tex_train.hip, whose swapped roles make R the layer's lazily
                               // normalised input); NULL: rhs is loaded as it is
    int krows;                 // kh * kw * cin: the real rows
    int nchunks, cpr, nranges; // 16-pixel chunks in all / per range; ranges (gridDim.y)
    float* partial;            // [range][krows][cout]
    float* dw;                 // OIHW
};
// GEMM K-row kp = tap * cin_p + ci -> tap and the row tap * cin + ci of `partial`, or -1 for a padded tap or channel
__device__ __forceinline__ int kpn_enc_wgrad_row(const kpn_enc_conv_args& c, int kp, int& tap, int& ci) {
    tap = kp / c.cin_p; ci = kp - tap * c.cin_p;
    return tap < c.kh * c.kw && ci < c.cin ? tap * c.cin + ci : -1;
}
template <int BM, int BN, bool STEM>
__global__ __launch_bounds__(256) void k_enc_wgrad(kpn_enc_wgrad_args a) {
    static_assert((BM / 32) * (BN / 32) == 4, "four wavefronts, one 32 x 32 accumulator each");
    constexpr int QA = BM / 4, PA = 256 / QA, NA = 16 / PA;     // K-row quads per chunk row; pixels per pass; passes
    constexpr int QB = BN / 4;
    __shared__ __attribute__((aligned(16))) float As[16][BM];
    __shared__ __attribute__((aligned(16))) float Bs[16][BN];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ctiles = a.c.cout_p / BN;
    const int ct = (int)(blockIdx.x % ctiles), kt = (int)(blockIdx.x / ctiles);
    const int64_t M = (int64_t)a.c.nimg * a.c.Ho * a.c.Wo;
    const int hw = a.c.Ho * a.c.Wo;
    const int aq = tid % QA, ap = tid / QA;                     // A loads: K-row quad, pixel of the chunk (+ j * PA)
    const int bq = tid % QB, bp = tid / QB;                     // dY loads: channel quad, pixel of the chunk
    const bool bload = bp < 16;
    const int bco = ct * BN + bq * 4;
    const int s0 = (int)blockIdx.y * a.cpr, s1 = min(s0 + a.cpr, a.nchunks);
    kpn_f32x4 ra[NA], rb = {0.0f, 0.0f, 0.0f, 0.0f};
    auto load = [&](int s) {
        for (int j = 0; j < NA; ++j) {
            const int64_t p = (int64_t)s * 16 + ap + j * PA;
            const bool valid = p < M;
            const int n = valid ? (int)(p / hw) : 0, rem = valid ? (int)(p % hw) : 0;
            ra[j] = kpn_enc_load_a<STEM, false>(a.c, 0, valid, n, rem / a.c.Wo, rem % a.c.Wo, kt * BM + aq * 4);
        }
        if (bload) {
            const int64_t p = (int64_t)s * 16 + bp;
            rb = kpn_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            if (p < M && bco < a.c.cout) {
                rb = *KPN_GLOBAL4(a.rhs + (size_t)p * a.rhs_cs + bco);
                if (a.rhs_ss) {
                    const size_t n = (size_t)(p / hw);          // the image of the pixel
                    const kpn_f32x4 sc = *KPN_GLOBAL4(a.rhs_ss + n * a.c.cout + bco);
                    const kpn_f32x4 sh = *KPN_GLOBAL4(a.rhs_ss + ((size_t)a.c.nimg + n) * a.c.cout + bco);
                    for (int e = 0; e < 4; ++e) rb[e] = fmaf(rb[e], sc[e], sh[e]);
                    if (a.rhs_relu)
                        for (int e = 0; e < 4; ++e) rb[e] = rb[e] > 0.0f ? rb[e] : 0.0f;
                }
            }
        }
    };
    const int wn = wave % (BN / 32), wm = wave / (BN / 32);
    const int ai = wm * 32 + (lane & 31), bj = wn * 32 + (lane & 31), kh2 = lane >> 5;
    kpn_f32x16 acc;
    double sum[16];
    for (int r = 0; r < 16; ++r) { acc[r] = 0.0f; sum[r] = 0.0; }
    if (s0 < s1) load(s0);
    for (int s = s0; s < s1; ++s) {
        for (int j = 0; j < NA; ++j) *reinterpret_cast<kpn_f32x4*>(&As[ap + j * PA][aq * 4]) = ra[j];
        if (bload) *reinterpret_cast<kpn_f32x4*>(&Bs[bp][bq * 4]) = rb;
        __syncthreads();
        if (s + 1 < s1) load(s + 1);
        for (int m = 0; m < 8; ++m)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[2 * m + kh2][ai], Bs[2 * m + kh2][bj], acc, 0, 0, 0);
        for (int r = 0; r < 16; ++r) { sum[r] += (double)acc[r]; acc[r] = 0.0f; }   // an fp32 chain is one chunk long; above it, fp64
        __syncthreads();
    }
    // D[row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)][col = lane & 31]: rows are K-rows, columns output channels
    const int co = ct * BN + bj;
    if (co >= a.c.cout) return;
    float* out = a.partial + (size_t)blockIdx.y * a.krows * a.c.cout;
    for (int r = 0; r < 16; ++r) {
        int tap, ci;
        const int krow = kpn_enc_wgrad_row(a.c, kt * BM + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh2, tap, ci);
        if (krow >= 0) out[(size_t)krow * a.c.cout + co] = (float)sum[r];
    }
}
// the ranges of one dW element, added in range order in fp64 and rounded once; one thread per (GEMM K-row, co), the padded ones
// idle; partial[range][tap * cin + ci][co] -> OIHW
__global__ __launch_bounds__(256) void k_enc_wgrad_combine(kpn_enc_wgrad_args a) {
    const int taps = a.c.kh * a.c.kw;
    const int64_t total = (int64_t)taps * a.c.cin_p * a.c.cout, real = (int64_t)a.krows * a.c.cout;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int co = (int)(i % a.c.cout);
        int tap, ci;
        const int krow = kpn_enc_wgrad_row(a.c, (int)(i / a.c.cout), tap, ci);
        if (krow < 0) continue;
        double v = 0.0;
        for (int r = 0; r < a.nranges; ++r) v += (double)a.partial[(size_t)r * real + (size_t)krow * a.c.cout + co];
        a.dw[((size_t)co * a.c.cin + ci) * taps + tap] = (float)v;
    }
}

// Bias gradient db[co] = sum over pixels of dY[pixel][co]: block `chunk` adds its pixel range per channel in fp64 (the threads
// of one channel quad in thread order), k_enc_dbias_final adds the chunks in order and rounds once.  partial [chunk][C]
struct kpn_enc_dbias_args {
    const float* dy;       // (M, C) dense
    int64_t M;
    int C, nchunks;
    double* partial;
    float* db;
};
__global__ __launch_bounds__(256) void k_enc_dbias_partial(kpn_enc_dbias_args a) {
    __shared__ double red[256][4];
    const int L = a.C / 4;                       // threads per pixel (at most 256)
    const int PP = 256 / L;
    const int cl = threadIdx.x % L, pl = threadIdx.x / L;
    const int chunk = blockIdx.x;
    const int64_t p0 = chunk * a.M / a.nchunks, p1 = (chunk + 1) * a.M / a.nchunks;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    if (pl < PP)
        for (int64_t p = p0 + pl; p < p1; p += PP) {
            const kpn_f32x4 v = *KPN_GLOBAL4(a.dy + (size_t)p * a.C + cl * 4);
            for (int e = 0; e < 4; ++e) s[e] += (double)v[e];
        }
    for (int e = 0; e < 4; ++e) red[threadIdx.x][e] = s[e];
    __syncthreads();
    if (pl == 0) {
        for (int k = 1; k < PP; ++k)
            for (int e = 0; e < 4; ++e) s[e] += red[k * L + cl][e];
        for (int e = 0; e < 4; ++e) a.partial[(size_t)chunk * a.C + cl * 4 + e] = s[e];
    }
}
__global__ __launch_bounds__(64) void k_enc_dbias_final(kpn_enc_dbias_args a) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.C) return;
    double S = 0.0;
    for (int k = 0; k < a.nchunks; ++k) S += a.partial[(size_t)k * a.C + c];
    a.db[c] = (float)S;
}

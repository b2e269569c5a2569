// vgg_kernels.hip — the perceptual term of the training loss, VGGLoss (reference src/utils.py:750-805), forward and the
// gradient to its first argument, on the fp32 MFMA (v_mfma_f32_16x16x4_f32).
//
// VGGLoss(x, y) = sum_i w_i * mean|phi_i(norm(x)) - phi_i(norm(y))| with norm(v) = (v - mean) / std per channel and phi_i the
// outputs of vgg19.features[0:2], [2:7], [7:12], [12:21] (relu1_1, relu2_1, relu3_1, relu4_1): nine 3x3 / stride 1 / pad 1
// convolutions with bias and ReLU, a 2x2 / stride 2 floor-mode max-pool in front of conv 3, 5 and 9.
//
// Layout: activations NHWC, x and y as one batch of 2B images (x first), so that both go through the same arithmetic
// whatever their position.  Each convolution is an implicit GEMM  out[pixel][co] = sum_{tap, ci} in[pixel + tap][ci] *
// W[co][ci][tap]: one workgroup computes 16 pixels x 32 output channels (two 16x16 accumulators), its four wavefronts split
// the K loop over the nine taps and groups of 16 input channels; each lane loads four consecutive channels of one pixel (A operand) and four
// weights of one output channel (B operand) as float4s and feeds them to four MFMAs.  Normalisation is folded into the
// first convolution's loads, each max-pool into the next convolution's loads; bias and ReLU are the epilogue.
//
// Backward (x only, the y features are detached and the weights frozen, src/utils.py:772-774,804): for l = 9 .. 1
//   dIn_l = conv(G_l, W_l transposed and flipped),   G_l = [A_l > 0] * (seed_l + unpool(dIn_{l+1}))
// as the same GEMM over a second packed copy of the weights.  G_l is formed in the loads: the ReLU mask and the pool
// arg-maxes (first maximum of each window in row-major order, as PyTorch) come from the stored activations of x, the L1
// seed sign(phi_x - phi_y) * lambda * w_i / n_i (sign(0) = 0) from those of x and y.  The last step writes d x / std.
//
// Every output element is four MFMA chains over fixed K ranges, added in a fixed order; the loss is reduced from fixed per-block fp64
// partials in block order: results are bit-reproducible and independent of the position of an image in the batch.

#define KPN_VGG_LAYERS 9

// geometry of one convolution launch (forward or backward)
struct kpn_vgg_conv_args {
    int nimg, H, W;          // images and resolution of the output (= of the GEMM rows)
    int groups;              // K = 9 taps x groups x 16 channels
    int cout, cout_p;        // output channels, padded to a multiple of 32 (weight rows)
    const float* wp;         // packed weights [tap][group][cout_p][16]
    const float* bias;       // forward only
    float* out;              // NHWC (nimg, H, W, cout); the backward of layer 1 writes NCHW d x instead (final != 0)
    // sources
    const float* src;        // mode 1: NHWC (H, W, csrc); mode 2: NHWC (Hs, Ws, csrc) pooled 2x2; mode 3: A_l (2B images)
    int Hs, Ws, csrc;
    const float* x;          // mode 0: NCHW inputs, images [0, B) from x, [B, 2B) from y
    const float* y;
    int B;
    float mean[3], stdv[3];
    // backward loads (mode 3)
    const float* up;         // dIn_{l+1} (B, Hu, Wu, csrc) or NULL (layer 9)
    int up_pool, Hu, Wu;     // up is at the pooled resolution (conv l+1 reads a max-pool of A_l)
    float seed;              // lambda * w_i / n_i if layer l is a tap, else 0
    int tap;
    int final_;              // backward of layer 1: out is d x (NCHW), divided by std
};

__device__ __forceinline__ kpn_f32x4 kpn_vgg_ld4(const float* p) { return *KPN_GLOBAL4(p); }

// A operand: channels [c, c+4) of pixel (n, sy, sx) of the GEMM input; zero outside the image (padding)
template <int MODE>
__device__ __forceinline__ kpn_f32x4 kpn_vgg_load_a(const kpn_vgg_conv_args& a, int n, int sy, int sx, int c) {
    kpn_f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if constexpr (MODE == 0) {
        // normalize(x) (torchvision Normalize: (v - mean) / std), channels >= 3 are the zero padding of K
        const float* img = n < a.B ? a.x + (size_t)n * 3 * a.H * a.W : a.y + (size_t)(n - a.B) * 3 * a.H * a.W;
        for (int e = 0; e < 4; ++e) {
            const int ch = c + e;
            if (ch < 3) v[e] = KSUB(img[((size_t)ch * a.H + sy) * a.W + sx], a.mean[ch]) / a.stdv[ch];
        }
    } else if constexpr (MODE == 1) {
        v = kpn_vgg_ld4(a.src + (((size_t)n * a.H + sy) * a.W + sx) * a.csrc + c);
    } else if constexpr (MODE == 2) {
        const float* p = a.src + (((size_t)n * a.Hs + 2 * sy) * a.Ws + 2 * sx) * a.csrc + c;
        const kpn_f32x4 p00 = kpn_vgg_ld4(p), p01 = kpn_vgg_ld4(p + a.csrc);
        const kpn_f32x4 p10 = kpn_vgg_ld4(p + (size_t)a.Ws * a.csrc), p11 = kpn_vgg_ld4(p + (size_t)a.Ws * a.csrc + a.csrc);
        for (int e = 0; e < 4; ++e) v[e] = fmaxf(fmaxf(p00[e], p01[e]), fmaxf(p10[e], p11[e]));
    } else {
        // G_l = [A_l > 0] * (seed + unpool(up)) at pixel (n, sy, sx) of layer l (n < B: the x images)
        const size_t pix = ((size_t)n * a.H + sy) * a.W + sx;
        const kpn_f32x4 ax = kpn_vgg_ld4(a.src + pix * a.csrc + c);
        float g[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (a.tap) {
            const kpn_f32x4 ay = kpn_vgg_ld4(a.src + (pix + (size_t)a.B * a.H * a.W) * a.csrc + c);
            for (int e = 0; e < 4; ++e) {
                const float d = KSUB(ax[e], ay[e]);
                g[e] = d > 0.0f ? a.seed : (d < 0.0f ? -a.seed : 0.0f);
            }
        }
        if (a.up) {
            if (!a.up_pool) {
                const kpn_f32x4 u = kpn_vgg_ld4(a.up + pix * a.csrc + c);
                for (int e = 0; e < 4; ++e) g[e] = KADD(g[e], u[e]);
            } else {
                const int qy = sy >> 1, qx = sx >> 1;
                if (qy < a.Hu && qx < a.Wu) {           // floor mode: the last odd row / column is in no window
                    const float* p = a.src + (((size_t)n * a.H + 2 * qy) * a.W + 2 * qx) * a.csrc + c;
                    const kpn_f32x4 w0 = kpn_vgg_ld4(p), w1 = kpn_vgg_ld4(p + a.csrc);
                    const kpn_f32x4 w2 = kpn_vgg_ld4(p + (size_t)a.W * a.csrc), w3 = kpn_vgg_ld4(p + (size_t)a.W * a.csrc + a.csrc);
                    const kpn_f32x4 u = kpn_vgg_ld4(a.up + (((size_t)n * a.Hu + qy) * a.Wu + qx) * a.csrc + c);
                    const int mine = 2 * (sy & 1) + (sx & 1);
                    for (int e = 0; e < 4; ++e) {
                        // first maximum in row-major scan order (PyTorch: update only on a strictly greater value)
                        float m = w0[e];
                        int arg = 0;
                        if (w1[e] > m) { m = w1[e]; arg = 1; }
                        if (w2[e] > m) { m = w2[e]; arg = 2; }
                        if (w3[e] > m) { m = w3[e]; arg = 3; }
                        if (arg == mine) g[e] = KADD(g[e], u[e]);
                    }
                }
            }
        }
        for (int e = 0; e < 4; ++e) v[e] = ax[e] > 0.0f ? g[e] : 0.0f;
    }
    return v;
}

// one workgroup = 16 pixels x 32 output channels; its 4 wavefronts split K (taps x channel groups) into four consecutive
// ranges, and wavefront 0 adds their accumulators in wavefront order (fixed, the same for every tile)
template <int MODE>
__global__ __launch_bounds__(256) void k_vgg_conv(kpn_vgg_conv_args a) {
    __shared__ kpn_f32x4 red[3][2][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t tile = blockIdx.x;
    const int64_t npx = (int64_t)a.nimg * a.H * a.W;
    const int64_t ptiles = (npx + 15) / 16;
    const int ctiles = a.cout_p / 32;
    if (tile >= ptiles * ctiles) return;                 // whole workgroups only
    const int ct = (int)(tile % ctiles);                 // neighbouring workgroups share the pixels (their loads hit L2)
    const int64_t pt = tile / ctiles;
    const int i = lane & 15, kk = lane >> 4;
    const int64_t p = pt * 16 + i;
    const bool valid = p < npx;
    const int n = valid ? (int)(p / ((int64_t)a.H * a.W)) : 0;
    const int rem = valid ? (int)(p % ((int64_t)a.H * a.W)) : 0;
    const int yy = rem / a.W, xx = rem % a.W;
    const float* w0 = a.wp + ((size_t)ct * 32 + i) * 16 + kk * 4;     // + ((tap * groups + g) * cout_p) * 16
    kpn_f32x4 acc0 = {0.0f, 0.0f, 0.0f, 0.0f}, acc1 = {0.0f, 0.0f, 0.0f, 0.0f};
    // K step s = (tap t, channel group g); the operands of step s + 1 are loaded before the MFMAs of step s
    const int nk = 9 * a.groups;
    const int s0 = wave * nk / 4, s1 = (wave + 1) * nk / 4;
    auto load = [&](int s, kpn_f32x4& av, kpn_f32x4& b0, kpn_f32x4& b1) {
        const int t = s / a.groups, g = s % a.groups;
        const int sy = yy + t / 3 - 1, sx = xx + t % 3 - 1;
        av = kpn_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        if (valid && sy >= 0 && sy < a.H && sx >= 0 && sx < a.W) av = kpn_vgg_load_a<MODE>(a, n, sy, sx, g * 16 + kk * 4);
        const float* wr = w0 + (size_t)s * a.cout_p * 16;
        b0 = kpn_vgg_ld4(wr);
        b1 = kpn_vgg_ld4(wr + 16 * 16);
    };
    kpn_f32x4 av = {0.0f, 0.0f, 0.0f, 0.0f}, b0 = av, b1 = av;
    if (s0 < s1) load(s0, av, b0, b1);
    for (int s = s0; s < s1; ++s) {
        kpn_f32x4 avn = av, b0n = b0, b1n = b1;
        if (s + 1 < s1) load(s + 1, avn, b0n, b1n);
        for (int m = 0; m < 4; ++m) {
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m], b0[m], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m], b1[m], acc1, 0, 0, 0);
        }
        av = avn; b0 = b0n; b1 = b1n;
    }
    if (wave > 0) {
        red[wave - 1][0][lane] = acc0;
        red[wave - 1][1][lane] = acc1;
    }
    __syncthreads();
    if (wave > 0) return;
    for (int w = 0; w < 3; ++w) {
        const kpn_f32x4 r0 = red[w][0][lane], r1 = red[w][1][lane];
        for (int e = 0; e < 4; ++e) { acc0[e] = KADD(acc0[e], r0[e]); acc1[e] = KADD(acc1[e], r1[e]); }
    }
    // D[row = 4 (lane >> 4) + r][col = lane & 15]: rows are pixels, columns output channels
    for (int b = 0; b < 2; ++b) {
        const int co = ct * 32 + b * 16 + (lane & 15);
        if (co >= a.cout) continue;
        kpn_f32x4 acc = acc0;
        if (b) acc = acc1;
        for (int r = 0; r < 4; ++r) {
            const int64_t q = pt * 16 + 4 * (lane >> 4) + r;
            if (q >= npx) continue;
            if constexpr (MODE != 3) {
                const float z = KADD(acc[r], a.bias[co]);
                a.out[q * a.cout + co] = z > 0.0f ? z : 0.0f;
            } else if (a.final_) {
                const int qn = (int)(q / ((int64_t)a.H * a.W)), qr = (int)(q % ((int64_t)a.H * a.W));
                a.out[((size_t)qn * 3 + co) * a.H * a.W + qr] = acc[r] / a.stdv[co];
            } else {
                a.out[q * a.cout + co] = acc[r];
            }
        }
    }
}

// the four L1 terms: block (k, t) sums |phi_x - phi_y| over its stride of tap t in fp64 (kpn_reduce.h); the last block to finish
// adds the partials in a fixed tree of its own and writes loss = lambda * sum_t w_t * S_t / n_t
#define KPN_VGG_L1_BLOCKS 64
struct kpn_vgg_l1_args {
    const float* act[4];
    int64_t n[4];            // elements of phi_t(x); those of phi_t(y) follow them
    double w[4];
    double lambda;
    double* partial;         // 4 x KPN_VGG_L1_BLOCKS
    int* ticket;
    float* loss;
};
__global__ __launch_bounds__(256) void k_vgg_l1(kpn_vgg_l1_args a) {
    __shared__ double red[1][256];
    const int t = blockIdx.y;
    const float* px = a.act[t];
    const int64_t n = a.n[t];
    double acc[1] = {0.0};
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)KPN_VGG_L1_BLOCKS * blockDim.x)
        acc[0] += (double)fabsf(KSUB(px[i], px[n + i]));
    // block-uniform: the whole last block adds the partials, fixed tree
    if (kpn_block_sums_last(acc, red, a.partial, a.ticket, t * KPN_VGG_L1_BLOCKS + blockIdx.x, 4 * KPN_VGG_L1_BLOCKS, true)) {
        double* const r = red[0];
        r[threadIdx.x] = ((volatile double*)a.partial)[threadIdx.x];   // 256 = 4 taps x KPN_VGG_L1_BLOCKS
        __syncthreads();
        for (int s = KPN_VGG_L1_BLOCKS / 2; s > 0; s >>= 1) {
            if ((int)(threadIdx.x % KPN_VGG_L1_BLOCKS) < s) r[threadIdx.x] += r[threadIdx.x + s];
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            double tot = 0.0;
            for (int u = 0; u < 4; ++u) tot += a.w[u] * (r[u * KPN_VGG_L1_BLOCKS] / (double)a.n[u]);
            a.loss[0] = (float)(a.lambda * tot);
        }
    }
}

// packer: plain (per conv, in features order: OIHW weight then bias) -> forward copy [tap][group][cout][16] + bias, and
// backward copy [tap][group of cout][cin_p][16] holding W[co][ci][8 - tap] (transposed, flipped)
struct kpn_vgg_pack_layer {
    int cin, cout, gf, gb, cin_p;   // forward groups = ceil(cin/16); backward groups = cout/16; cin_p = cin padded to 32
    int64_t plain, fwd, bias, bwd;  // offsets (floats)
};
struct kpn_vgg_pack_table {
    kpn_vgg_pack_layer l[KPN_VGG_LAYERS];
    int64_t total;
};
__global__ __launch_bounds__(256) void k_vgg_pack(kpn_vgg_pack_table tb, const float* __restrict__ plain, float* __restrict__ packed) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < tb.total; i += (int64_t)gridDim.x * blockDim.x) {
    int L = 0;
    while (L + 1 < KPN_VGG_LAYERS && i >= tb.l[L + 1].fwd) ++L;
    const kpn_vgg_pack_layer& s = tb.l[L];
    const float* W = plain + s.plain;                       // [cout][cin][9]
    float v = 0.0f;
    if (i < s.bias) {                                       // forward: ((t * gf + g) * cout + co) * 16 + e
        const int64_t r = i - s.fwd;
        const int e = (int)(r % 16), co = (int)((r / 16) % s.cout);
        const int64_t tg = r / 16 / s.cout;
        const int g = (int)(tg % s.gf), t = (int)(tg / s.gf);
        const int ci = g * 16 + e;
        if (ci < s.cin) v = W[((size_t)co * s.cin + ci) * 9 + t];
    } else if (i < s.bwd) {
        v = plain[s.plain + (int64_t)s.cout * s.cin * 9 + (i - s.bias)];
    } else {                                                // backward: ((t * gb + g) * cin_p + ci) * 16 + e, e over cout
        const int64_t r = i - s.bwd;
        const int e = (int)(r % 16), ci = (int)((r / 16) % s.cin_p);
        const int64_t tg = r / 16 / s.cin_p;
        const int g = (int)(tg % s.gb), t = (int)(tg / s.gb);
        const int co = g * 16 + e;
        if (ci < s.cin) v = W[((size_t)co * s.cin + ci) * 9 + (8 - t)];
    }
    packed[i] = v;
  }
}

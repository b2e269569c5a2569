// encoder_split_kernels.hip — the stride-1 convolution family of encoder_kernels.hip on v_mfma_f32_32x32x16_bf16 with every fp32
// operand carried as three bf16 pieces (KPN_CONV_BF16X3): x = h + m + l, h = bf16(x), m = bf16(x - h), l = bf16(x - h - m), the
// residuals exact in fp32 (kpn_split_bf16x8, kpn_common.h), so |x - (h + m + l)| <= 2^-24 |x| over fp32's whole exponent range - no range
// guard, no scales.  A product a * b is the six piece products above 2^-24 relative, accumulated in fp32 into TWO accumulators per
// 32 x 32 output block, in this fixed order per K slab of 16 (kpn_enc_mfma6):
//     hi += ah bh              (exact products of 16 bits: hi is the fp32 chain of the leading pieces, as long as that of the fp32 kernel)
//     lo += ah bm,  am bh,  am bm,  ah bl,  al bh          (2^-8 of the result and below: their roundings are 2^-8 of an ulp of it)
// and the result is hi + lo, one fp32 add behind the last slab (the weight gradient adds both to its fp64 sum).  One accumulator
// for all six would round every small product at the ulp of the whole sum: 6 K roundings instead of K, which the K = 8 case of
// tests/conv_cases.py shows (4.6 e_ref).  6 x 8 passes against the 8 x 16 passes of v_mfma_f32_32x32x2_f32 over the same 16 K entries.
// Operand maps (kpn_common.h): A lane l holds A[i = l & 31][k = 8 (l >> 5) + e], B lane l holds B[k = 8 (l >> 5) + e][j = l & 31],
// e = 0 .. 7 as the eight bf16 of one 16-byte register quad; D as the 32x32x2 form.
//
// k_enc_pack_b3    OIHW weights -> [chunk of 32 K][piece][K octet g = 0 .. 3][cout_p] units of 16 bytes, a unit = the eight K entries
//                  32 chunk + 8 g + e of one output channel and one piece: exactly a lane's B operand.  K = tap * cin_p + ci as in
//                  k_enc_pack; plain and tflip; padded taps and channels are zero in all three pieces.  6 bytes per weight.
// k_enc_conv_b3    the implicit GEMM of k_enc_conv<.., false, false> (zero padding, stride 1, NHWC) with kpn_enc_load_a<false, false> and
//                  kpn_enc_epilogue unchanged.  A workgroup of four wavefronts computes BM x BN outputs, 128 x 64 or (at most 32 output
//                  channels) 256 x 32; a wavefront owns 64 pixels x 32 channels as two accumulators that share their B operand.  K
//                  chunk 32: a thread loads whole K octets of its pixel (two float4s), splits them once and writes each piece as one
//                  16-byte unit.  LDS image: As[piece][octet][pixel], Bs[piece][octet][channel], 16-byte units - the lanes of an operand
//                  read (and the staging threads write) consecutive units: ds_read_b128 / ds_write_b128 without bank conflicts.  The
//                  loads of chunk s + 1 are in flight while chunk s is multiplied.  Split K over blockIdx.y by the per-image geometry,
//                  partial tiles to scratch, k_enc_combine adds them in split order.
// k_enc_wgrad_b3   the weight gradient of k_enc_wgrad with the pixel index as the MFMA's K: both operands are split in the kernel, by the
//                  staging threads, once per tile.  The A operand needs eight consecutive pixels of one K-row per lane, the loads give
//                  four consecutive K-rows of one pixel: it is STAGED TRANSPOSED (no transposing LDS read).  A thread loads the same
//                  K-row quad (resp. channel quad of R) of two consecutive pixels, splits the eight values so that a converted pair is
//                  (pixel 2w, pixel 2w + 1) of one row, and writes one dword per row and piece to As[piece][pixel pair w][position].
//                  The position of row 4 q + e of the tile is e * (BM / 4) + q: consecutive threads (q) write consecutive dwords, and
//                  the lanes of an operand read consecutive positions, four dwords (pairs 4 (l >> 5) .. + 3) each - no bank conflicts
//                  either way.  The MFMA's row i is therefore the row at position i; the store undoes the permutation.  After every
//                  16-pixel chunk the fp32 accumulators are added to fp64 sums and cleared; ranges, partials and k_enc_wgrad_combine as
//                  the fp32 kernel.  The LDS image is double-buffered, so a chunk costs one barrier.
// No atomics, every sum in a fixed order: equal bits from run to run, and an image's result does not depend on its batch.

__device__ __forceinline__ kpn_u32x4 kpn_enc_u4(kpn_bf16x8 v) { return __builtin_bit_cast(kpn_u32x4, v); }
__device__ __forceinline__ kpn_bf16x8 kpn_enc_b8(kpn_u32x4 v) { return __builtin_bit_cast(kpn_bf16x8, v); }
// the six products of one K slab, in the documented order; a / b: the pieces h, m, l
__device__ __forceinline__ void kpn_enc_mfma6(const kpn_bf16x8 (&a)[3], const kpn_bf16x8 (&b)[3], kpn_f32x16& hi, kpn_f32x16& lo) {
    hi = KPN_MFMA16(a[0], b[0], hi);
    lo = KPN_MFMA16(a[0], b[1], lo);
    lo = KPN_MFMA16(a[1], b[0], lo);
    lo = KPN_MFMA16(a[1], b[1], lo);
    lo = KPN_MFMA16(a[0], b[2], lo);
    lo = KPN_MFMA16(a[2], b[0], lo);
}

// a.nk: chunks of 32; a.out: 16-byte units [chunk][piece][octet][cout_p]
__global__ __launch_bounds__(256) void k_enc_pack_b3(kpn_enc_pack_args a) {
    const int64_t total = (int64_t)a.nk * 4 * a.cout_p;
    kpn_u32x4* out = reinterpret_cast<kpn_u32x4*>(a.out);
    const int taps = a.kh * a.kw;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int co = (int)(i % a.cout_p), g = (int)((i / a.cout_p) % 4), s = (int)(i / a.cout_p / 4);
        float v[8];
        for (int e = 0; e < 8; ++e) {
            const int kk = s * 32 + g * 8 + e, tap = kk / a.cin_p, c = kk % a.cin_p;
            v[e] = 0.0f;
            if (co < a.cout && c < a.cin && tap < taps)
                v[e] = a.tflip ? a.w[((size_t)c * a.cout + co) * taps + (taps - 1 - tap)] : a.w[((size_t)co * a.cin + c) * taps + tap];
        }
        kpn_bf16x8 p[3];
        kpn_split_bf16x8(v, p[0], p[1], p[2]);
        for (int q = 0; q < 3; ++q) out[(((size_t)s * 3 + q) * 4 + g) * a.cout_p + co] = kpn_enc_u4(p[q]);
    }
}

template <int BM, int BN>
__global__ __launch_bounds__(256) void k_enc_conv_b3(kpn_enc_conv_args a) {
    static_assert((BM / 64) * (BN / 32) == 4, "four wavefronts, 64 pixels x 32 channels (two accumulators) each");
    constexpr int GS = 256 / BM;                // octet step between the units of one thread
    constexpr int NA = 4 / GS;                  // K octets of A per thread and chunk
    constexpr int NB = (12 * BN + 255) / 256;   // 16-byte units of the packed weights per thread and chunk
    __shared__ kpn_u32x4 As[3][4][BM];
    __shared__ kpn_u32x4 Bs[12][BN];            // [piece * 4 + octet][channel]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ctiles = a.cout_p / BN;
    const int ct = (int)(blockIdx.x % ctiles);
    const int64_t pt = blockIdx.x / ctiles;
    const int64_t M = (int64_t)a.nimg * a.Ho * a.Wo;
    const int hw = a.Ho * a.Wo;
    // A loads: one GEMM row per thread
    const int arow = tid % BM, ag = tid / BM;
    const int64_t p = pt * BM + arow;
    const bool valid = p < M;
    const int n = valid ? (int)(p / hw) : 0;
    const int rem = valid ? (int)(p % hw) : 0;
    const int oy = rem / a.Wo, ox = rem % a.Wo;
    const int nk = a.nk[0];
    const int ks = (int)blockIdx.y;
    const int s0 = (int)((int64_t)ks * nk / a.ksplit), s1 = (int)((int64_t)(ks + 1) * nk / a.ksplit);
    kpn_f32x4 ra[NA][2], rb[NB];
    auto load = [&](int s) {
        _Pragma("unroll") for (int j = 0; j < NA; ++j) {
            const int kk = s * 32 + (ag + j * GS) * 8;
            ra[j][0] = kpn_enc_load_a<false, false>(a, 0, valid, n, oy, ox, kk);
            ra[j][1] = kpn_enc_load_a<false, false>(a, 0, valid, n, oy, ox, kk + 4);
        }
        _Pragma("unroll") for (int j = 0; j < NB; ++j) {
            const int u = tid + j * 256;
            if (u < 12 * BN) rb[j] = *KPN_GLOBAL4(a.wp + (((size_t)s * 12 + u / BN) * a.cout_p + (size_t)ct * BN + u % BN) * 4);
        }
    };
    const int wn = wave % (BN / 32), wm = wave / (BN / 32);
    const int l31 = lane & 31, kh2 = lane >> 5;
    kpn_f32x16 acc[2], lo[2];
    _Pragma("unroll") for (int t = 0; t < 2; ++t)
        _Pragma("unroll") for (int r = 0; r < 16; ++r) { acc[t][r] = 0.0f; lo[t][r] = 0.0f; }
    if (s0 < s1) load(s0);
    for (int s = s0; s < s1; ++s) {
        _Pragma("unroll") for (int j = 0; j < NA; ++j) {
            const float x[8] = {ra[j][0][0], ra[j][0][1], ra[j][0][2], ra[j][0][3], ra[j][1][0], ra[j][1][1], ra[j][1][2], ra[j][1][3]};
            kpn_bf16x8 pc[3];
            kpn_split_bf16x8(x, pc[0], pc[1], pc[2]);
            _Pragma("unroll") for (int q = 0; q < 3; ++q) As[q][ag + j * GS][arow] = kpn_enc_u4(pc[q]);
        }
        _Pragma("unroll") for (int j = 0; j < NB; ++j) {
            const int u = tid + j * 256;
            if (u < 12 * BN) Bs[u / BN][u % BN] = __builtin_bit_cast(kpn_u32x4, rb[j]);
        }
        __syncthreads();
        if (s + 1 < s1) load(s + 1);
        _Pragma("unroll") for (int slab = 0; slab < 2; ++slab) {
            const int g = 2 * slab + kh2;
            kpn_bf16x8 b[3];
            _Pragma("unroll") for (int q = 0; q < 3; ++q) b[q] = kpn_enc_b8(Bs[q * 4 + g][wn * 32 + l31]);
            _Pragma("unroll") for (int t = 0; t < 2; ++t) {
                kpn_bf16x8 av[3];
                _Pragma("unroll") for (int q = 0; q < 3; ++q) av[q] = kpn_enc_b8(As[q][g][wm * 64 + t * 32 + l31]);
                kpn_enc_mfma6(av, b, acc[t], lo[t]);
            }
        }
        __syncthreads();
    }
    // D[row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)][col = lane & 31]: rows are pixels, columns output channels
    const int co = ct * BN + wn * 32 + l31;
    if (co >= a.cout) return;
    _Pragma("unroll") for (int t = 0; t < 2; ++t)
        _Pragma("unroll") for (int r = 0; r < 16; ++r) {
            const int64_t q = pt * BM + wm * 64 + t * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh2;
            if (q >= M) continue;
            const float v = KADD(acc[t][r], lo[t][r]);
            if (a.ksplit > 1) a.partial[((int64_t)ks * M + q) * a.cout_p + co] = v;
            else kpn_enc_epilogue(a, 0, q, co, v, false);
        }
}

template <int BM, int BN>
__global__ __launch_bounds__(256) void k_enc_wgrad_b3(kpn_enc_wgrad_args a) {
    static_assert((BM / 64) * (BN / 32) == 4, "four wavefronts, 64 K-rows x 32 channels (two accumulators) each");
    constexpr int QA = BM / 4, UA = QA * 8 / 256;   // K-row quads of the tile; (quad, pixel pair) units of A per thread and chunk
    constexpr int QB = BN / 4, UB = QB * 8;         // channel quads; units of R per chunk (one per thread, the first UB threads)
    __shared__ uint32_t As[2][3][8][BM];            // [buffer][piece][pixel pair][position]
    __shared__ uint32_t Bs[2][3][8][BN];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ctiles = a.c.cout_p / BN;
    const int ct = (int)(blockIdx.x % ctiles), kt = (int)(blockIdx.x / ctiles);
    const int64_t M = (int64_t)a.c.nimg * a.c.Ho * a.c.Wo;
    const int hw = a.c.Ho * a.c.Wo;
    const int bq = tid % QB, bw = tid / QB;
    const bool bload = tid < UB;
    const int bco = ct * BN + bq * 4;
    const int s0 = (int)blockIdx.y * a.cpr, s1 = min(s0 + a.cpr, a.nchunks);
    kpn_f32x4 ra[UA][2], rb[2];
    auto load = [&](int s) {
        _Pragma("unroll") for (int j = 0; j < UA; ++j) {
            const int u = tid + j * 256;
            // the pair's first pixel is decomposed once, in 32 bits (M < 2^31: the descriptor check), the second follows it
            const int p = s * 16 + (u / QA) * 2;
            int n = p / hw;
            const int rem = p - n * hw;
            int oy = rem / a.c.Wo, ox = rem - oy * a.c.Wo;
            ra[j][0] = kpn_enc_load_a<false, false>(a.c, 0, p < M, n, oy, ox, kt * BM + (u % QA) * 4);
            if (++ox == a.c.Wo) { ox = 0; if (++oy == a.c.Ho) { oy = 0; ++n; } }
            ra[j][1] = kpn_enc_load_a<false, false>(a.c, 0, p + 1 < M, n, oy, ox, kt * BM + (u % QA) * 4);
        }
        if (bload)
            _Pragma("unroll") for (int t = 0; t < 2; ++t) {
                const int p = s * 16 + bw * 2 + t;
                kpn_f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
                if (p < M && bco < a.c.cout) {
                    v = *KPN_GLOBAL4(a.rhs + (size_t)p * a.rhs_cs + bco);
                    if (a.rhs_ss) {
                        const size_t n = (size_t)(p / hw);          // the image of the pixel
                        const kpn_f32x4 sc = *KPN_GLOBAL4(a.rhs_ss + n * a.c.cout + bco);
                        const kpn_f32x4 sh = *KPN_GLOBAL4(a.rhs_ss + ((size_t)a.c.nimg + n) * a.c.cout + bco);
                        _Pragma("unroll") for (int e = 0; e < 4; ++e) v[e] = fmaf(v[e], sc[e], sh[e]);
                        if (a.rhs_relu)
                            _Pragma("unroll") for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.0f ? v[e] : 0.0f;
                    }
                }
                rb[t] = v;
            }
    };
    // eight values (rows e = 0 .. 3 of pixels 2 w and 2 w + 1) -> one dword (the pixel pair) per row and piece
    auto split_pairs = [](const kpn_f32x4& v0, const kpn_f32x4& v1, kpn_u32x4 (&pc)[3]) {
        const float x[8] = {v0[0], v1[0], v0[1], v1[1], v0[2], v1[2], v0[3], v1[3]};
        kpn_bf16x8 h, m, l;
        kpn_split_bf16x8(x, h, m, l);
        pc[0] = kpn_enc_u4(h); pc[1] = kpn_enc_u4(m); pc[2] = kpn_enc_u4(l);
    };
    const int wn = wave % (BN / 32), wm = wave / (BN / 32);
    const int l31 = lane & 31, kh2 = lane >> 5;
    kpn_f32x16 zero;
    double sum[2][16];
    _Pragma("unroll") for (int r = 0; r < 16; ++r) { zero[r] = 0.0f; sum[0][r] = 0.0; sum[1][r] = 0.0; }
    if (s0 < s1) load(s0);
    // Two LDS buffers, one barrier per chunk: chunk s is written to buffer s & 1 and read behind the barrier; the writes of chunk s + 1 go
    // to the other buffer, whose last readers (chunk s - 1) all passed the barrier of chunk s before any thread can write it
    for (int s = s0; s < s1; ++s) {
        const int buf = (s - s0) & 1;
        _Pragma("unroll") for (int j = 0; j < UA; ++j) {
            const int u = tid + j * 256;
            kpn_u32x4 pc[3];
            split_pairs(ra[j][0], ra[j][1], pc);
            _Pragma("unroll") for (int q = 0; q < 3; ++q)
                _Pragma("unroll") for (int e = 0; e < 4; ++e) As[buf][q][u / QA][e * QA + u % QA] = pc[q][e];
        }
        if (bload) {
            kpn_u32x4 pc[3];
            split_pairs(rb[0], rb[1], pc);
            _Pragma("unroll") for (int q = 0; q < 3; ++q)
                _Pragma("unroll") for (int e = 0; e < 4; ++e) Bs[buf][q][bw][e * QB + bq] = pc[q][e];
        }
        __syncthreads();
        if (s + 1 < s1) load(s + 1);
        kpn_bf16x8 b[3];
        _Pragma("unroll") for (int q = 0; q < 3; ++q) {
            kpn_u32x4 w;
            _Pragma("unroll") for (int j = 0; j < 4; ++j) w[j] = Bs[buf][q][4 * kh2 + j][wn * 32 + l31];
            b[q] = kpn_enc_b8(w);
        }
        _Pragma("unroll") for (int t = 0; t < 2; ++t) {
            kpn_bf16x8 av[3];
            _Pragma("unroll") for (int q = 0; q < 3; ++q) {
                kpn_u32x4 w;
                _Pragma("unroll") for (int j = 0; j < 4; ++j) w[j] = As[buf][q][4 * kh2 + j][wm * 64 + t * 32 + l31];
                av[q] = kpn_enc_b8(w);
            }
            kpn_f32x16 hi = zero, lo = zero;
            kpn_enc_mfma6(av, b, hi, lo);
            _Pragma("unroll") for (int r = 0; r < 16; ++r) sum[t][r] += (double)hi[r] + (double)lo[r];   // an fp32 chain is one chunk long; above it, fp64
        }
    }
    // D[row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)][col = lane & 31] in positions: position P holds row (P % Q) * 4 + P / Q of the tile
    const int pc = wn * 32 + l31;
    const int co = ct * BN + (pc % QB) * 4 + pc / QB;
    if (co >= a.c.cout) return;
    float* out = a.partial + (size_t)blockIdx.y * a.krows * a.c.cout;
    _Pragma("unroll") for (int t = 0; t < 2; ++t)
        _Pragma("unroll") for (int r = 0; r < 16; ++r) {
            const int pr = wm * 64 + t * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh2;
            int tap, ci;
            const int krow = kpn_enc_wgrad_row(a.c, kt * BM + (pr % QA) * 4 + pr / QA, tap, ci);
            if (krow >= 0) out[(size_t)krow * a.c.cout + co] = (float)sum[t][r];
        }
}

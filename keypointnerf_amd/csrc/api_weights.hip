// ---------------------------------------------------------------------------------------------
// weight packing
namespace {
enum { P_G1_0, P_G1_1, P_G1_2, P_G1_3, P_G2_0, P_G2_1, P_G2_2, P_CMP, P_RE_0, P_RE_1, P_BL_0, P_BL_1, P_V1_0, P_V1_1,
       P_V2_0, P_V2_1, P_O_0, P_O_1, P_O_2, P_COUNT };
const int plain_dims[P_COUNT][2] = {{128, 232}, {128, 128}, {120, 136}, {64, 120}, {64, 128}, {64, 64}, {2, 64},
                                    {24, 128},  {16, 4},    {35, 16},   {64, 105}, {32, 64},  {32, 32}, {33, 32},
                                    {32, 32},   {1, 32},    {16, 37},   {8, 16},   {1, 8}};
// offsets of a layer's W and b in the plain vector: [W0 | b0 | W1 | b1 | ... | ani_al]; plain_w_off(P_COUNT) = the offset of ani_al
size_t plain_w_off(int layer) {
    size_t o = 0;
    for (int l = 0; l < layer; ++l) o += (size_t)plain_dims[l][0] * plain_dims[l][1] + plain_dims[l][0];
    return o;
}
size_t plain_b_off(int layer) { return plain_w_off(layer) + (size_t)plain_dims[layer][0] * plain_dims[layer][1]; }
struct Plain { const float* w[P_COUNT]; const float* b[P_COUNT]; float ani_al; };
void bind_plain(const float* flat, Plain& pl) {
    for (int l = 0; l < P_COUNT; ++l) { pl.w[l] = flat + plain_w_off(l); pl.b[l] = flat + plain_b_off(l); }
    pl.ani_al = flat[plain_w_off(P_COUNT)];
}
// chained input: K-step s = 16*block + r is input feature 32*block + rowmap(r, h)
inline int chain_feature(int s, int h) { return 32 * (s / 16) + KPN_ROWMAP(s % 16, h); }
// x' order of the 35-vector: rows 0..23 = lat (orig 11..34), 24..26 = rgb (orig 0..2), 27..34 = tex (orig 3..10)
inline int xprime_to_orig(int q) { return q < 24 ? 11 + q : (q < 27 ? q - 24 : q - 24); }
// x' K-steps (20): s<16 -> row rowmap(s,h); s = 16..18 -> row 32 + rowmap(s-16, h); s = 19 -> pad
inline int xstep_row(int s, int h) { return s < 16 ? KPN_ROWMAP(s, h) : (s < 19 ? 32 + KPN_ROWMAP(s - 16, h) : 9999); }

template <class FMap, class OMap>
void pack_segment(float* packed, int seg, const float* W, const float* b, int out_dim, int in_dim, FMap fmap, OMap omap,
                  bool with_bias = true) {
    const int KS = kpn_seg_shapes[seg].ks, NOB = kpn_seg_shapes[seg].nob, G = kpn_seg_shapes[seg].g;
    const int NF = G * NOB;
    float* w = packed + kpn_seg_woff(seg);
    float* bb = packed + kpn_seg_boff(seg);
    for (int s = 0; s < KS; ++s)
        for (int ob = 0; ob < NOB; ++ob)
            for (int lane = 0; lane < 64; ++lane) {
                const int i = lane & 31, h = lane >> 5;
                const int orow = omap(ob * 32 + i);
                const int f = fmap(s, h);
                float val = 0.0f;
                if (orow >= 0 && orow < out_dim && f >= 0 && f < in_dim) val = W[(size_t)orow * in_dim + f];
                w[((size_t)(s / G) * 64 + lane) * NF + (s % G) * NOB + ob] = val;
            }
    for (int ob = 0; ob < NOB; ++ob)
        for (int h = 0; h < 2; ++h)
            for (int r = 0; r < 16; ++r) {
                const int orow = omap(ob * 32 + KPN_ROWMAP(r, h));
                bb[(ob * 2 + h) * 16 + r] = (with_bias && orow >= 0 && orow < out_dim) ? b[orow] : 0.0f;
            }
}
// a transposed (backward) segment: out row R of the stream is forward INPUT feature in_of_row(R), K-step (s,h) is
// forward OUTPUT feature chain_feature(s,h); value W[o][f]
template <class RowMap, class KMap>
void pack_segment_t(float* packed, int bseg, const float* W, int out_dim, int in_dim, RowMap in_of_row, KMap out_of_kstep) {
    const int KS = kpn_bseg_shapes[bseg].ks, NOB = kpn_bseg_shapes[bseg].nob, G = kpn_bseg_shapes[bseg].g;
    const int NF = G * NOB;
    float* w = packed + kpn_bseg_woff(bseg);
    for (int s = 0; s < KS; ++s)
        for (int ob = 0; ob < NOB; ++ob)
            for (int lane = 0; lane < 64; ++lane) {
                const int i = lane & 31, h = lane >> 5;
                const int f = in_of_row(ob * 32 + i);
                const int o = out_of_kstep(s, h);
                float val = 0.0f;
                if (f >= 0 && f < in_dim && o >= 0 && o < out_dim) val = W[(size_t)o * in_dim + f];
                w[((size_t)(s / G) * 64 + lane) * NF + (s % G) * NOB + ob] = val;
            }
}
template <class RowMap>
void pack_segment_t(float* packed, int bseg, const float* W, int out_dim, int in_dim, RowMap in_of_row) {
    pack_segment_t(packed, bseg, W, out_dim, in_dim, in_of_row, [](int s, int h) { return chain_feature(s, h); });
}
// split-bf16 stream of one layer (kpn_common.h HSEG_*): feat(step, h, e) = input feature of the e-th value the half-h
// lanes supply in 16-deep K-step `step`, or -1 (pad)
inline uint16_t host_f2bf(float f) {  // round to nearest even
    uint32_t u; memcpy(&u, &f, 4);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
inline float host_bf2f(uint16_t b) { uint32_t u = (uint32_t)b << 16; float f; memcpy(&f, &u, 4); return f; }
// enumerates the elements of one split-bf16 segment: emit(element index within the segment = ((s*NOB+ob)*64+lane)*8+e,
// plain-layout weight index or -1)
template <class FMap, class Emit>
void walk_hsegment(int hseg, size_t w_off, int out_dim, int in_dim, FMap feat, Emit emit) {
    const int KS = kpn_hseg_shapes[hseg].ks16, NOB = kpn_hseg_shapes[hseg].nob;
    for (int s = 0; s < KS; ++s)
        for (int ob = 0; ob < NOB; ++ob)
            for (int lane = 0; lane < 64; ++lane) {
                const int i = lane & 31, h = lane >> 5, orow = ob * 32 + i;
                for (int e = 0; e < 8; ++e) {
                    const int f = feat(s, h, e);
                    const bool real = orow < out_dim && f >= 0 && f < in_dim;
                    emit((((size_t)s * NOB + ob) * 64 + lane) * 8 + e, real ? (int64_t)(w_off + (size_t)orow * in_dim + f) : (int64_t)-1);
                }
            }
}
// the five layers1 segments with their K maps; w_off[layer] = offset of the layer's W in the plain layout
template <class Emit>
void walk_hsegments(const size_t (&w_off)[4], Emit emit) {
    auto chain16 = [](int s, int h, int e) { return 32 * (s / 2) + KPN_ROWMAP(8 * (s % 2) + e, h); };
    walk_hsegment(HSEG_G1_0A, w_off[0], 128, 232, [](int s, int h, int e) { return e < 7 ? e * 24 + s + 12 * h : -1; },
                  [&](size_t el, int64_t src) { emit(HSEG_G1_0A, el, src); });
    // geo0 channels of step s: 16 s + 8 h + e — the two halves of a point read the same 64-byte piece of one cache line (32
    // distinct lines per gather instruction instead of 64)
    walk_hsegment(HSEG_G1_0B, w_off[0], 128, 232, [](int s, int h, int e) { return 168 + 16 * s + 8 * h + e; },
                  [&](size_t el, int64_t src) { emit(HSEG_G1_0B, el, src); });
    walk_hsegment(HSEG_G1_1, w_off[1], 128, 128, chain16, [&](size_t el, int64_t src) { emit(HSEG_G1_1, el, src); });
    walk_hsegment(HSEG_G1_2, w_off[2], 120, 136,
                  [&](int s, int h, int e) { return s < 8 ? chain16(s, h, e) : (e < 4 ? 128 + 4 * h + e : -1); },
                  [&](size_t el, int64_t src) { emit(HSEG_G1_2, el, src); });
    walk_hsegment(HSEG_G1_3, w_off[3], 64, 120, chain16, [&](size_t el, int64_t src) { emit(HSEG_G1_3, el, src); });
}
// u16 slot of piece pc of element el of a segment, relative to the packed buffer viewed as uint16; np = pieces per value
// (3: the bf16 streams, 2: the fp16 streams behind them)
inline size_t hseg_slot(int hseg, size_t el, int pc, int np = 3) {
    const int NOB = kpn_hseg_shapes[hseg].nob;
    const size_t e = el % 8, lane = (el / 8) % 64, ob = (el / 512) % NOB, s = el / (512 * (size_t)NOB);
    return (size_t)kpn_xseg_off(hseg, np) * 2 + ((((s * NOB + ob) * np + pc) * 64 + lane) * 8 + e);   // [step][block][piece][lane][8]
}
inline uint16_t host_f2h(float f) { const _Float16 h = (_Float16)f; uint16_t u; memcpy(&u, &h, 2); return u; }   // round to nearest even
inline float host_h2f(uint16_t u) { _Float16 h; memcpy(&h, &u, 2); return (float)h; }
// factor folded into the weight at plain index `src` of segment `hseg` (log2-unit activations, kpn_common.h kpn_hseg_factor)
inline float hseg_weight_factor(int hseg, int64_t src, const size_t (&w_off)[4], int np = 3) {
    static const int layer_of[HSEG_COUNT] = {0, 0, 1, 2, 3}, in_dim[4] = {232, 128, 136, 120};
    if (src < 0) return 1.0f;
    const int l = layer_of[hseg];
    const int col = (int)((src - (int64_t)w_off[l]) % in_dim[l]);
    return np == 3 ? kpn_hseg_factor(hseg, col) : kpn_fseg_factor(hseg, col);
}
float softplus100_host(float x) { float t = x * 100.0f; return t > 20.0f ? x : log1pf(expf(t)) / 100.0f; }
// ---- the fp16 region of the per-point kernel (kpn_common.h kpn_cseg_*): every value is read from the ALREADY PACKED fp32
// stream of the same segment — K slot (chunk c, e) of the half-h lanes = fp32 K-step 8c + e — so host and device packer need
// no index maps of their own.  Element t of the region's stream part: ((c*NOB + ob)*64 + lane)*8 + e within its segment.
// flat element t of a region's concatenated segments -> its segment (returned) and the element within it (el)
template <int (*Elements)(int)>
__host__ __device__ inline int locate_segment(int first, int t, int& el) {
    int sg = first;
    for (el = t; el >= Elements(sg); ++sg) el -= Elements(sg);
    return sg;
}
__host__ __device__ inline int k2h_elements(int seg) { return kpn_cseg_chunks(seg) * kpn_seg_shapes[seg].nob * 64 * 8; }
inline int k2h_total_elements() { int n = 0; for (int sg = SEG_G2_0; sg < SEG_COUNT; ++sg) n += k2h_elements(sg); return n; }
// (segment, element) -> float index of the fp32 packed weight (or -1: pad), u16 slot of the h piece; the l piece is 64*8 slots on
__host__ __device__ inline void k2h_locate(int seg, int el, int& src, int& slot) {
    const int NOB = kpn_seg_shapes[seg].nob, G = kpn_seg_shapes[seg].g, KS = kpn_seg_shapes[seg].ks;
    const int e = el % 8, lane = (el / 8) % 64, ob = (el / 512) % NOB, c = el / (512 * NOB);
    const int s = 8 * c + e;
    src = s < KS ? kpn_seg_woff(seg) + ((s / G) * 64 + lane) * (G * NOB) + (s % G) * NOB + ob : -1;
    slot = kpn_cseg_woff(seg) * 2 + (((c * NOB + ob) * 2) * 64 + lane) * 8 + e;
}
// ---- the backward chains' bf16 region (kpn_common.h BH_*): same idea, three bf16 pieces, chunk width 7 or 8 ----
__host__ __device__ inline int bh_elements(int i) { return kpn_bh_chunks(i) * kpn_bh_shape(i).nob * 64 * 8; }
inline int bh_total_elements() { int n = 0; for (int i = 0; i < BH_COUNT; ++i) n += bh_elements(i); return n; }
// (stream, element) -> float index of the fp32 packed weight (or -1: pad), u16 slot of the h piece; the m and l pieces are 64*8 slots on each
__host__ __device__ inline void bh_locate(int i, int el, int& src, int& slot) {
    const int NOB = kpn_bh_shape(i).nob, G = kpn_bh_shape(i).g, KS = kpn_bh_shape(i).ks, CW = kpn_bh_cw(i);
    const int e = el % 8, lane = (el / 8) % 64, ob = (el / 512) % NOB, c = el / (512 * NOB);
    const int s = c * CW + e;
    src = (e < CW && s < KS) ? kpn_bh_src_woff(i) + ((s / G) * 64 + lane) * (G * NOB) + (s % G) * NOB + ob : -1;
    slot = kpn_bh_off(i) * 2 + (((c * NOB + ob) * 3) * 64 + lane) * 8 + e;
}
void pack_bh_host(float* P) {
    uint16_t* P16 = reinterpret_cast<uint16_t*>(P);
    for (int t = 0, n = bh_total_elements(); t < n; ++t) {
        int el, src, slot;
        const int i = locate_segment<bh_elements>(0, t, el);
        bh_locate(i, el, src, slot);
        const float w = src >= 0 ? P[src] : 0.0f;
        const uint16_t ph = host_f2bf(w);
        const float r1 = w - host_bf2f(ph);
        const uint16_t pm = host_f2bf(r1);
        P16[slot] = ph; P16[slot + 512] = pm; P16[slot + 1024] = host_f2bf(r1 - host_bf2f(pm));
    }
}
int pack_k2h_host(float* P) {   // returns the number of weights beyond fp16's range
    uint16_t* P16 = reinterpret_cast<uint16_t*>(P);
    int beyond = 0;
    for (int t = 0, n = k2h_total_elements(); t < n; ++t) {
        int el, src, slot;
        const int sg = locate_segment<k2h_elements>(SEG_G2_0, t, el);
        k2h_locate(sg, el, src, slot);
        const float w = (src >= 0 ? P[src] : 0.0f) * kpn_cseg_wfactor(sg);   // log2-unit activations of layers2 (kpn_common.h)
        if (!(fabsf(w) <= 65504.0f)) ++beyond;
        const uint16_t ph = host_f2h(w);
        P16[slot] = ph; P16[slot + 512] = host_f2h(w - host_h2f(ph));
    }
    for (int sg = SEG_G2_0; sg < SEG_COUNT; ++sg)
        for (int k = 0; k < kpn_seg_bfloats(sg); ++k) P[kpn_cseg_boff(sg) + k] = P[kpn_seg_boff(sg) + k] * kpn_cseg_bfactor(sg);
    return beyond;
}
}  // namespace
// device side of the same: one thread per stream element, then the bias blocks and the scalar / row-vector tail
__global__ void k_pack_k2h(float* __restrict__ packed, int n_elem, float* __restrict__ flags) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n_elem) {
        int el, src, slot;
        const int sg = locate_segment<k2h_elements>(SEG_G2_0, t, el);
        k2h_locate(sg, el, src, slot);
        const float w = (src >= 0 ? packed[src] : 0.0f) * kpn_cseg_wfactor(sg);
#ifndef KPN_SIMT_EMU
        const _Float16 h = (_Float16)w;
        const _Float16 l = (_Float16)(w - (float)h);
        uint16_t ph, pl; memcpy(&ph, &h, 2); memcpy(&pl, &l, 2);
#else
        const uint16_t ph = kpn_f2h(w), pl = kpn_f2h(w - kpn_h2f(ph));
#endif
        if (!(fabsf(w) <= 65504.0f)) kpn_atomic_add(flags, 1.0f);
        uint16_t* p16 = reinterpret_cast<uint16_t*>(packed);
        p16[slot] = ph; p16[slot + 512] = pl;
    }
    // bias blocks + tail: plain copies inside the packed buffer
    const int n_bias = kpn_k2h_tail_off() - kpn_cseg_boff(SEG_G2_0), n_tail = kpn_fwd_floats() - kpn_scalar_off();
    if (t < n_bias) {
        int sg = SEG_G2_0, k = t;
        while (k >= kpn_seg_bfloats(sg)) { k -= kpn_seg_bfloats(sg); ++sg; }
        packed[kpn_cseg_boff(sg) + k] = packed[kpn_seg_boff(sg) + k] * kpn_cseg_bfactor(sg);
    } else if (t < n_bias + n_tail) {
        packed[kpn_k2h_tail_off() + (t - n_bias)] = packed[kpn_scalar_off() + (t - n_bias)];
    }
}


extern "C" size_t kpn_plain_weight_floats(void) { return plain_w_off(P_COUNT) + 1; }
extern "C" size_t kpn_packed_weight_floats(void) { return (size_t)kpn_packed_floats(); }

extern "C" int kpn_pack_weights(const float* plain_host, float* packed_host) {
    KPN_REQUIRE(plain_host && packed_host, "null pointer");
    Plain pl;
    bind_plain(plain_host, pl);
    auto ident = [](int row) { return row; };
    auto chain = [](int s, int h) { return chain_feature(s, h); };
    float* P = packed_host;
    // layers1.0: part A, K-steps 0..83 keypoint encoding (j = s/7 -> keypoint j+12h, t = s%7 -> PE block t:
    // feature t*24 + kp, spatial.py:36-39,117); part B, 32 K-steps: geometry channel 32h + s (feature 168 + c)
    pack_segment(P, SEG_G1_0A, pl.w[P_G1_0], pl.b[P_G1_0], 128, 232,
                 [](int s, int h) { return (s % 7) * 24 + (s / 7) + 12 * h; }, ident);
    pack_segment(P, SEG_G1_0B, pl.w[P_G1_0], pl.b[P_G1_0], 128, 232, [](int s, int h) { return 168 + 32 * h + s; }, ident,
                 /*with_bias=*/false);
    pack_segment(P, SEG_G1_1, pl.w[P_G1_1], pl.b[P_G1_1], 128, 128, chain, ident);
    // layers1.2: [128 chained | hd channel 4h + (s-64)]
    pack_segment(P, SEG_G1_2, pl.w[P_G1_2], pl.b[P_G1_2], 120, 136,
                 [](int s, int h) { return s < 64 ? chain_feature(s, h) : 128 + 4 * h + (s - 64); }, ident);
    pack_segment(P, SEG_G1_3, pl.w[P_G1_3], pl.b[P_G1_3], 64, 120, chain, ident);
    // layers2.0: [mean64 | var64], each in chained order
    pack_segment(P, SEG_G2_0, pl.w[P_G2_0], pl.b[P_G2_0], 64, 128,
                 [](int s, int h) { return s < 32 ? chain_feature(s, h) : 64 + chain_feature(s - 32, h); }, ident);
    pack_segment(P, SEG_G2_1, pl.w[P_G2_1], pl.b[P_G2_1], 64, 64, chain, ident);
    pack_segment(P, SEG_G2_2, pl.w[P_G2_2], pl.b[P_G2_2], 2, 64, chain, ident);
    // ibr_compress_gfeat: same input as layers2.0; output rows already in x' order (row q<24 = lat q)
    pack_segment(P, SEG_CMP, pl.w[P_CMP], pl.b[P_CMP], 24, 128,
                 [](int s, int h) { return s < 32 ? chain_feature(s, h) : 64 + chain_feature(s - 32, h); }, ident);
    pack_segment(P, SEG_RE_0, pl.w[P_RE_0], pl.b[P_RE_0], 16, 4, [](int s, int h) { return s < 2 ? 2 * s + h : -1; }, ident);
    // ray_encoder.2: output rows permuted to x' order
    pack_segment(P, SEG_RE_1, pl.w[P_RE_1], pl.b[P_RE_1], 35, 16, chain,
                 [](int q) { return q < 35 ? xprime_to_orig(q) : -1; });
    // base_layer.0 columns: [mean35 | var35 | x35] (model.py:1292)
    pack_segment(P, SEG_BL_0A, pl.w[P_BL_0], pl.b[P_BL_0], 64, 105,
                 [](int s, int h) {
                     const int q = xstep_row(s % 20, h);
                     return q < 35 ? (s / 20) * 35 + xprime_to_orig(q) : -1;
                 }, ident);
    pack_segment(P, SEG_BL_0B, pl.w[P_BL_0], pl.b[P_BL_0], 64, 105,
                 [](int s, int h) { const int q = xstep_row(s, h); return q < 35 ? 70 + xprime_to_orig(q) : -1; }, ident,
                 /*with_bias=*/false);
    pack_segment(P, SEG_BL_1, pl.w[P_BL_1], pl.b[P_BL_1], 32, 64, chain, ident);
    pack_segment(P, SEG_V1_0, pl.w[P_V1_0], pl.b[P_V1_0], 32, 32, chain, ident);
    pack_segment(P, SEG_V1_1, pl.w[P_V1_1], pl.b[P_V1_1], 32, 32, chain, ident);  // rows 0..31 (res); row 32 (vis) below
    pack_segment(P, SEG_V2_0, pl.w[P_V2_0], pl.b[P_V2_0], 32, 32, chain, ident);
    // out_layer.0 columns: [x32 | vis | ray_diff4] (model.py:1300); extra K-steps 16,17,18
    pack_segment(P, SEG_O_0, pl.w[P_O_0], pl.b[P_O_0], 16, 37,
                 [](int s, int h) {
                     if (s < 16) return chain_feature(s, h);
                     const int f = 32 + 2 * (s - 16) + h;
                     return (s < 19 && f < 37) ? f : -1;
                 }, ident);
    pack_segment(P, SEG_O_1, pl.w[P_O_1], pl.b[P_O_1], 8, 16, chain, ident);
    // single-output layers as row vectors over the chained features of one 32-row block
    auto pack_row = [&](int row, const float* W, int in_dim, float bias) {
        float* r = P + kpn_row_off(row);
        for (int h = 0; h < 2; ++h)
            for (int k = 0; k < 16; ++k) { const int f = KPN_ROWMAP(k, h); r[h * 16 + k] = f < in_dim ? W[f] : 0.0f; }
        r[32] = bias; r[33] = r[34] = r[35] = 0.0f;
    };
    pack_row(ROW_V1_VIS, pl.w[P_V1_1] + 32 * 32, 32, pl.b[P_V1_1][32]);
    pack_row(ROW_V2_1, pl.w[P_V2_1], 32, pl.b[P_V2_1][0]);
    pack_row(ROW_O_2, pl.w[P_O_2], 8, pl.b[P_O_2][0]);
    // backward of layers1 (kpn_geo_rows_backward): the transposed matrices
    pack_segment_t(P, BSEG_G1_3T, pl.w[P_G1_3], 64, 120, ident);
    pack_segment_t(P, BSEG_G1_2T, pl.w[P_G1_2], 120, 136, [](int R) { return R < 128 ? R : (R < 136 ? R : -1); });
    pack_segment_t(P, BSEG_G1_1T, pl.w[P_G1_1], 128, 128, ident);
    pack_segment_t(P, BSEG_G1_0T, pl.w[P_G1_0], 128, 232, [](int R) { return R < 64 ? 168 + R : -1; });
    // backward of layers2 (kpn_query_backward)
    pack_segment_t(P, BSEG_G2_1T, pl.w[P_G2_1], 64, 64, ident);
    pack_segment_t(P, BSEG_G2_0T, pl.w[P_G2_0], 64, 128, ident);
    // backward of the colour head (k_color_bwd)
    pack_segment_t(P, BSEG_CMPT, pl.w[P_CMP], 24, 128, ident);
    pack_segment_t(P, BSEG_RE_1T, pl.w[P_RE_1], 35, 16, [](int R) { return R < 16 ? R : -1; },
                   [](int s, int h) { const int q = xstep_row(s, h); return q < 35 ? xprime_to_orig(q) : -1; });
    pack_segment_t(P, BSEG_BL_0AT, pl.w[P_BL_0], 64, 105, [](int R) {
        const int part = R / 64, q = R % 64;
        return q < 35 ? part * 35 + xprime_to_orig(q) : -1;
    });
    pack_segment_t(P, BSEG_BL_0BT, pl.w[P_BL_0], 64, 105, [](int R) { return R < 35 ? 70 + xprime_to_orig(R) : -1; });
    pack_segment_t(P, BSEG_BL_1T, pl.w[P_BL_1], 32, 64, ident);
    pack_segment_t(P, BSEG_V1_0T, pl.w[P_V1_0], 32, 32, ident);
    pack_segment_t(P, BSEG_V1_1T, pl.w[P_V1_1], 32, 32, ident);  // the vis row (32) is a rank-1 VALU update (ROW_V1_VIS)
    pack_segment_t(P, BSEG_V2_0T, pl.w[P_V2_0], 32, 32, ident);
    pack_segment_t(P, BSEG_O_0T, pl.w[P_O_0], 16, 37, [](int R) { return R <= 32 ? R : -1; });
    pack_segment_t(P, BSEG_O_1T, pl.w[P_O_1], 8, 16, [](int R) { return R < 16 ? R : -1; });
    for (int o = 0; o < 2; ++o)
        for (int b = 0; b < 2; ++b)
            for (int h = 0; h < 2; ++h)
                for (int r = 0; r < 16; ++r)
                    P[kpn_brow_off(BROW_G2_2_SDF + o) + (2 * b + h) * 16 + r] = pl.w[P_G2_2][o * 64 + 32 * b + KPN_ROWMAP(r, h)];
    // split-bf16 streams of layers1 (k_geo_rows_h)
    {
        size_t w_off[4];
        for (int l = 0; l < 4; ++l) w_off[l] = plain_w_off(P_G1_0 + l);
        uint16_t* P16 = reinterpret_cast<uint16_t*>(P);
        walk_hsegments(w_off, [&](int hseg, size_t el, int64_t src) {
            const float w = src >= 0 ? plain_host[src] * hseg_weight_factor(hseg, src, w_off) : 0.0f;
            const uint16_t ph = host_f2bf(w);
            const float r1 = w - host_bf2f(ph);
            const uint16_t pm = host_f2bf(r1);
            P16[hseg_slot(hseg, el, 0)] = ph; P16[hseg_slot(hseg, el, 1)] = pm; P16[hseg_slot(hseg, el, 2)] = host_f2bf(r1 - host_bf2f(pm));
        });
        // fp16 double-split streams of layers1 (k_geo_rows_f2) and the count of weights beyond fp16's range
        int beyond = 0;
        walk_hsegments(w_off, [&](int hseg, size_t el, int64_t src) {
            const float w = src >= 0 ? plain_host[src] * hseg_weight_factor(hseg, src, w_off, 2) : 0.0f;
            if (!(fabsf(w) <= 65504.0f)) ++beyond;
            const uint16_t ph = host_f2h(w);
            P16[hseg_slot(hseg, el, 0, 2)] = ph; P16[hseg_slot(hseg, el, 1, 2)] = host_f2h(w - host_h2f(ph));
        });
        // the per-point kernel's region with two fp16 pieces per value (k_fuse_color_h): derived from the fp32 streams packed above
        beyond += pack_k2h_host(P);
        pack_bh_host(P);
        float* fl = P + kpn_pack_flags_off();
        fl[0] = (float)beyond; fl[1] = fl[2] = fl[3] = 0.0f;
    }
    // scalars: |ani_al| (model.py:1287) and layers2(0), the query() result of a fully masked point
    float* sc = P + kpn_scalar_off();
    sc[0] = fabsf(pl.ani_al);
    {
        float a[64], b2[64], o2[2];
        for (int o = 0; o < 64; ++o) a[o] = softplus100_host(pl.b[P_G2_0][o]);
        for (int o = 0; o < 64; ++o) {
            float acc = 0.0f;
            for (int i = 0; i < 64; ++i) acc += pl.w[P_G2_1][o * 64 + i] * a[i];
            b2[o] = softplus100_host(acc + pl.b[P_G2_1][o]);
        }
        for (int o = 0; o < 2; ++o) {
            float acc = 0.0f;
            for (int i = 0; i < 64; ++i) acc += pl.w[P_G2_2][o * 64 + i] * b2[i];
            o2[o] = acc + pl.b[P_G2_2][o];
        }
        sc[1] = o2[0]; sc[2] = o2[1];
        sc[3] = pl.ani_al > 0.0f ? 1.0f : (pl.ani_al < 0.0f ? -1.0f : 0.0f);  // d|a|/da for the colour-head reverse
    }
    // k_fuse_color_h's copy of the scalars and row vectors (the tail of its LDS region)
    memcpy(P + kpn_k2h_tail_off(), P + kpn_scalar_off(), sizeof(float) * (size_t)(kpn_fwd_floats() - kpn_scalar_off()));
    return KPN_OK;
}

// ---------------------------------------------------------------------------------------------
// device-side packing: the host packer above is a pure gather apart from four derived scalars, so its index map is
// taken once (by packing a ramp) and applied on the device — a training loop re-packs after every optimizer step
// split-bf16 region: element t of the concatenated segments -> three bf16 pieces at their slots
__global__ void k_pack_hseg(const float* __restrict__ plain, const int32_t* __restrict__ src, const int32_t* __restrict__ slot0,
                            const int32_t* __restrict__ pstride, const float* __restrict__ factor, int n,
                            uint16_t* __restrict__ packed16) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const float w = src[t] >= 0 ? kpn_mul_nofma(plain[src[t]], factor[t]) : 0.0f;   // the host packer's product, bit for bit
    float one[8] = {w, 0, 0, 0, 0, 0, 0, 0};
    kpn_bf16x8 h, m, l;
    kpn_split3(one, h, m, l);
    uint16_t ph, pm, plo;
    { const auto hv = h[0]; const auto mv = m[0]; const auto lv = l[0]; memcpy(&ph, &hv, 2); memcpy(&pm, &mv, 2); memcpy(&plo, &lv, 2); }
    packed16[slot0[t]] = ph; packed16[slot0[t] + pstride[t]] = pm; packed16[slot0[t] + 2 * pstride[t]] = plo;
}
// fp16 region: two pieces; flag[0] counts the weights beyond fp16's range
__global__ void k_pack_fseg(const float* __restrict__ plain, const int32_t* __restrict__ src, const int32_t* __restrict__ slot0,
                            const int32_t* __restrict__ pstride, const float* __restrict__ factor, int n,
                            uint16_t* __restrict__ packed16, float* __restrict__ flags) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const float w = src[t] >= 0 ? kpn_mul_nofma(plain[src[t]], factor[t]) : 0.0f;
#ifndef KPN_SIMT_EMU
    const _Float16 h = (_Float16)w;
    const _Float16 l = (_Float16)(w - (float)h);
    uint16_t ph, pl; memcpy(&ph, &h, 2); memcpy(&pl, &l, 2);
#else
    const uint16_t ph = kpn_f2h(w), pl = kpn_f2h(w - kpn_h2f(ph));
#endif
    if (!(fabsf(w) <= 65504.0f)) kpn_atomic_add(flags, 1.0f);
    packed16[slot0[t]] = ph; packed16[slot0[t] + pstride[t]] = pl;
}
__global__ void k_pack_gather(const float* __restrict__ plain, const int32_t* __restrict__ map, int n, float* __restrict__ packed) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int m = map[i];
    packed[i] = m >= 0 ? plain[m] : 0.0f;
}
// scalars: |ani_al|, layers2(0) = query()'s [sdf_raw, rad] of a point masked in every view, sign(ani_al)
__global__ void k_pack_scalars(const float* __restrict__ plain, size_t w0, size_t b0, size_t w1, size_t b1, size_t w2, size_t b2,
                               size_t ani, float* __restrict__ sc) {
    __shared__ float a[64], b[64];
    const int o = threadIdx.x;  // 64 threads
    auto sp = [](float x) { const float t = x * 100.0f; return t > 20.0f ? x : log1pf(expf(t)) / 100.0f; };
    a[o] = sp(plain[b0 + o]);   // layers2.0 on pooled = 0
    __syncthreads();
    float acc = 0.0f;
    for (int i = 0; i < 64; ++i) acc += plain[w1 + (size_t)o * 64 + i] * a[i];
    b[o] = sp(acc + plain[b1 + o]);
    __syncthreads();
    if (o < 2) {
        float s = 0.0f;
        for (int i = 0; i < 64; ++i) s += plain[w2 + (size_t)o * 64 + i] * b[i];
        sc[1 + o] = s + plain[b2 + o];
    }
    if (o == 2) {
        const float al = plain[ani];
        sc[0] = fabsf(al);
        sc[3] = al > 0.0f ? 1.0f : (al < 0.0f ? -1.0f : 0.0f);
    }
    (void)w0;
}

// the backward chains' bf16 region from the fp32 streams (pack_bh_host): one thread per stream element
__global__ void k_pack_bh(float* __restrict__ packed, int n_elem) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_elem) return;
    int el, src, slot;
    const int i = locate_segment<bh_elements>(0, t, el);
    bh_locate(i, el, src, slot);
    const float w = src >= 0 ? packed[src] : 0.0f;
    float one[8] = {w, 0, 0, 0, 0, 0, 0, 0};
    kpn_bf16x8 h, m, l;
    kpn_split3(one, h, m, l);
    uint16_t ph, pm, plo;
    { const auto hv = h[0]; const auto mv = m[0]; const auto lv = l[0]; memcpy(&ph, &hv, 2); memcpy(&pm, &mv, 2); memcpy(&plo, &lv, 2); }
    uint16_t* p16 = reinterpret_cast<uint16_t*>(packed);
    p16[slot] = ph; p16[slot + 512] = pm; p16[slot + 1024] = plo;
}
// The gather maps of the device packer live in device memory, so they are kept PER DEVICE (a process that renders on two
// GPUs packs on both); built on first use for the device that is current at the call.
namespace {
struct DevicePackMaps {
    int32_t* map = nullptr;
    int32_t *hsrc = nullptr, *hslot = nullptr, *hstride = nullptr;
    float* hfactor = nullptr;
    int32_t *fslot = nullptr, *fstride = nullptr;   // the fp16 streams: same sources, their own slots and factors
    float* ffactor = nullptr;
    int n_helem = 0;
    int rc = KPN_OK;
};
DevicePackMaps* device_pack_maps() {
    static std::mutex mtx;
    static std::vector<DevicePackMaps*> per_device;   // index = HIP device ordinal
    int dev = 0;
#ifndef KPN_SIMT_EMU
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) return nullptr;
#endif
    std::lock_guard<std::mutex> lock(mtx);
    if ((size_t)dev >= per_device.size()) per_device.resize((size_t)dev + 1, nullptr);
    if (per_device[dev]) return per_device[dev];
    DevicePackMaps* M = per_device[dev] = new DevicePackMaps();
    const size_t np = kpn_plain_weight_floats(), nk = kpn_packed_weight_floats();
    std::vector<float> ramp(np), pk(nk, 0.0f);
    for (size_t i = 0; i < np; ++i) ramp[i] = (float)(i + 1);  // exact in fp32 (np < 2^24)
    if (kpn_pack_weights(ramp.data(), pk.data()) != KPN_OK) { M->rc = KPN_EINVAL; return M; }
    std::vector<int32_t> map(nk);
    // (the four derived scalars are not gathers: k_pack_scalars writes them; the split-bf16 region has its own maps)
    for (size_t i = 0; i < nk; ++i) map[i] = (pk[i] >= 1.0f && pk[i] <= (float)np) ? (int32_t)pk[i] - 1 : -1;
    for (int i = 0; i < 4; ++i) map[kpn_scalar_off() + i] = -1;
    auto up = [&](auto** d, const auto& h) {
        if (hipMalloc((void**)d, h.size() * sizeof(h[0])) != hipSuccess ||
            hipMemcpy(*d, h.data(), h.size() * sizeof(h[0]), hipMemcpyHostToDevice) != hipSuccess) M->rc = KPN_ELAUNCH;
    };
    up(&M->map, map);
    // split-bf16 region: per element its source weight, the folded factor, the u16 slot of its first piece and the piece stride
    std::vector<int32_t> hsrc, hslot, hstride;
    std::vector<float> hfactor;
    size_t w_off[4];
    for (int l = 0; l < 4; ++l) w_off[l] = plain_w_off(P_G1_0 + l);
    walk_hsegments(w_off, [&](int hseg, size_t el, int64_t src) {
        hsrc.push_back((int32_t)src);
        hfactor.push_back(hseg_weight_factor(hseg, src, w_off));
        hslot.push_back((int32_t)hseg_slot(hseg, el, 0));
        hstride.push_back((int32_t)(hseg_slot(hseg, el, 1) - hseg_slot(hseg, el, 0)));
    });
    M->n_helem = (int)hsrc.size();
    up(&M->hsrc, hsrc); up(&M->hslot, hslot); up(&M->hstride, hstride); up(&M->hfactor, hfactor);
    std::vector<int32_t> fslot, fstride;
    std::vector<float> ffactor;
    walk_hsegments(w_off, [&](int hseg, size_t el, int64_t src) {
        ffactor.push_back(hseg_weight_factor(hseg, src, w_off, 2));
        fslot.push_back((int32_t)hseg_slot(hseg, el, 0, 2));
        fstride.push_back((int32_t)(hseg_slot(hseg, el, 1, 2) - hseg_slot(hseg, el, 0, 2)));
    });
    up(&M->fslot, fslot); up(&M->fstride, fstride); up(&M->ffactor, ffactor);
    return M;
}
}  // namespace

extern "C" int kpn_pack_weights_device(const float* plain_dev, float* packed_dev, void* stream) {
    KPN_REQUIRE(plain_dev && packed_dev, "null pointer");
    const size_t np = kpn_plain_weight_floats();
    const DevicePackMaps* M = device_pack_maps();
    if (!M || M->rc != KPN_OK || !M->map) return fail(KPN_ELAUNCH, "could not build the device pack map");
    const int n_gather = kpn_bwd_end();  // everything before the split-bf16 region is a gather
    KPN_LAUNCH(k_pack_gather, grid1d((int64_t)n_gather, 256), dim3(256), stream, plain_dev, (const int32_t*)M->map, n_gather, packed_dev);
    KPN_LAUNCH(k_pack_hseg, grid1d((int64_t)M->n_helem, 256), dim3(256), stream, plain_dev, (const int32_t*)M->hsrc,
               (const int32_t*)M->hslot, (const int32_t*)M->hstride, (const float*)M->hfactor, M->n_helem,
               reinterpret_cast<uint16_t*>(packed_dev));
    (void)hipMemsetAsync(packed_dev + kpn_pack_flags_off(), 0, KPN_PACK_FLAG_FLOATS * sizeof(float), (hipStream_t)stream);
    KPN_LAUNCH(k_pack_fseg, grid1d((int64_t)M->n_helem, 256), dim3(256), stream, plain_dev, (const int32_t*)M->hsrc,
               (const int32_t*)M->fslot, (const int32_t*)M->fstride, (const float*)M->ffactor, M->n_helem,
               reinterpret_cast<uint16_t*>(packed_dev), packed_dev + kpn_pack_flags_off());
    KPN_LAUNCH(k_pack_scalars, dim3(1), dim3(64), stream, plain_dev, plain_w_off(P_G2_0), plain_b_off(P_G2_0), plain_w_off(P_G2_1), plain_b_off(P_G2_1),
               plain_w_off(P_G2_2), plain_b_off(P_G2_2), np - 1, packed_dev + kpn_scalar_off());
    // the per-point kernel's fp16 region from the fp32 streams, biases, scalars and row vectors written above (same stream: ordered)
    const int n_k2h = k2h_total_elements();
    KPN_LAUNCH(k_pack_k2h, grid1d((int64_t)n_k2h, 256), dim3(256), stream, packed_dev, n_k2h, packed_dev + kpn_pack_flags_off());
    const int n_bh = bh_total_elements();
    KPN_LAUNCH(k_pack_bh, grid1d((int64_t)n_bh, 256), dim3(256), stream, packed_dev, n_bh);
    return check_launch("kpn_pack_weights_device");
}

// Number of packed layers1 weights whose magnitude (after the folded activation scale) is beyond fp16's range, i.e. that rows
// mode 3 cannot represent (use mode 2 or 0 for such weights).  Reads four floats back from the device: synchronises `stream`.
extern "C" int kpn_packed_f16_range_check(const float* packed_dev, void* stream, int32_t* beyond) {
    KPN_REQUIRE(packed_dev && beyond, "null pointer");
    float fl[KPN_PACK_FLAG_FLOATS] = {0};
#ifndef KPN_SIMT_EMU
    if (hipMemcpyAsync(fl, packed_dev + kpn_pack_flags_off(), sizeof(fl), hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess ||
        hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return fail(KPN_ELAUNCH, "could not read the pack flags");
#else
    memcpy(fl, packed_dev + kpn_pack_flags_off(), sizeof(fl));
#endif
    *beyond = (int32_t)fl[0];
    return KPN_OK;
}

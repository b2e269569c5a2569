// ---------------------------------------------------------------------------------------------
// One differentiable convolution layer in terms of the launch layer (api_encoders.hip): which GEMMs it is, which packed copy each reads,
// how its source is loaded and which kernel is its input gradient.  Written once here; the single-layer families (api_conv.hip,
// api_strided.hip, api_reppad.hip) and the fused operators (api_block.hip, api_tex_train.hip) only say which layer they mean.
//   zero pad, stride 1     y = k_enc_conv            dx = k_enc_conv(dy, tflip copy, pad k - 1 - p)             dw = k_enc_wgrad, A from x
//   k 3, stride 2, pad 1   y = k_enc_conv(stride 2)  dx = k_enc_conv<DECONV>(dy) over the deconv copy of the same OIHW weight (H, W even:
//                          conv_transpose2d(dy, w, 2, 1, 1) is exactly the gradient)                            dw = A from x, stride 2
//   transposed k 3 (stride 2, pad 1, output_padding 1)
//                          y = k_enc_conv<DECONV>    dx = k_enc_conv(stride 2)(dy) over the plain copy of the (cin, cout, 3, 3) weight read
//                          as OIHW                                                      dw = A from dy with stride 2, rhs = x (swapped roles)
//   replicate, k 3 or 7    y = k_enc_conv(replicate) dx = k_enc_conv<RPADJ>(dy, tflip copy): the adjoint of the clamped load, a gather
//                                                                                       dw = A from x through the clamped load
//   stem (k 7; zero pad with stride 2, or replicate): reads an NCHW tensor as it is (stem_plain), K rows tap * 4 + ci, no dx
namespace enc {
struct LayerSpec {
    int cin, cout, k, stride, pad, replicate, transposed, stem;
    int arith = KPN_CONV_F32;  // KPN_CONV_BF16X3: the zero-padded stride-1 layer only (the first row of the table above)
};
struct Layer {
    LayerSpec s;
    int N, Hi, Wi, Ho, Wo;     // the grids of the layer's input and output
    ConvGeom fwd, dx, wg;      // fwd and dx are k_enc_conv launches; wg is the GEMM whose im2col rows and tile the weight gradient takes:
                               // the forward's, or the input gradient's for the transposed layer
    bool has_dx;               // not the stem
    int dx_tflip;              // the pack mode of the dx copy: transposed and flipped, or (stride 2, transposed) the other parity mode
    WgradPlan wgp;
    int64_t My;                // pixels of y: the rows of the bias gradient
    size_t packed_floats;      // the forward copy, then the dx copy
};
inline Layer layer(const LayerSpec& s, int N, int Hi, int Wi) {
    Layer l{};
    l.s = s; l.N = N; l.Hi = Hi; l.Wi = Wi;
    l.Ho = s.transposed ? 2 * Hi : (Hi + 2 * s.pad - s.k) / s.stride + 1;
    l.Wo = s.transposed ? 2 * Wi : (Wi + 2 * s.pad - s.k) / s.stride + 1;
    l.has_dx = !s.stem;
    l.dx_tflip = s.stride == 1 && !s.transposed;
    if (s.transposed) {
        l.fwd = conv_geom(N, Hi, Wi, s.cin, s.cout, s.k, s.k, 1);                      // x (H, W) -> y (2 H, 2 W)
        l.dx = conv_geom(N, Hi, Wi, s.cout, s.cin, s.k, s.k, 0);                       // dy (2 H, 2 W) -> dx (H, W), stride 2
    } else {
        l.fwd = conv_geom(N, l.Ho, l.Wo, s.cin, s.cout, s.k, s.k, 0, s.arith);
        if (l.has_dx) l.dx = s.stride == 2 ? conv_geom(N, l.Ho, l.Wo, s.cout, s.cin, s.k, s.k, 1)      // dy (Ho, Wo) -> dx (2 Ho, 2 Wo)
                                           : conv_geom(N, Hi, Wi, s.cout, s.cin, s.k, s.k, 0, s.arith);
    }
    l.wg = s.transposed ? l.dx : l.fwd;
    l.wgp = wgrad_plan(l.wg);
    l.My = (int64_t)N * l.Ho * l.Wo;
    l.packed_floats = (size_t)(l.fwd.packed + l.dx.packed);
    return l;
}
// the packed copies depend on cin, cout, k and the kind of the layer alone: the layer with a pad and on a grid that leave an output
inline Layer pack_layer(LayerSpec s) {
    if (!s.transposed) s.pad = s.k / 2;
    return layer(s, 1, s.k, s.k);
}
// Both copies read the weight as the layer holds it: OIHW through the plain mode is [GEMM cout][GEMM cin], (cin, cout, 3, 3) through the
// deconv mode is [GEMM cin][GEMM cout]; a stride-2 or transposed input gradient exchanges the counts and so takes the other mode
inline void layer_pack(const Layer& l, const float* w, float* packed, void* stream) {
    launch_pack(l.fwd, 0, w, packed, stream);
    if (l.has_dx) launch_pack(l.dx, l.dx_tflip, w, packed + l.fwd.packed, stream);
}
// the source side of the forward GEMM and (not transposed) of the weight gradient: src (N, Hi, Wi, cin) with channel stride src_cs -
// the stem's is NCHW, loaded as it is; ss: the scale / shift of a norm + ReLU fused into the loads, or NULL
inline void layer_source(kpn_enc_conv_args& a, const Layer& l, const float* src, int src_cs, const float* ss) {
    a.Hs = l.Hi; a.Ws = l.Wi; a.src = src; a.src_cs = src_cs;
    a.stride = l.s.transposed ? 1 : l.s.stride;
    a.pad = l.s.transposed ? 0 : l.s.pad;
    a.replicate = l.s.replicate;
    if (l.s.stem) { a.Hraw = l.Hi; a.Wraw = l.Wi; a.ds = 0; a.stem_plain = 1; }
    a.ss = ss; a.relu_in = ss != nullptr;
}
// dst (N, Ho, Wo, cout) = layer(src) [+ bias] [+ res]; wp: the layer's packed weight
inline void layer_forward(const Layer& l, const float* src, int src_cs, const float* ss, const float* wp, const float* bias, float* dst,
                          int dst_cs, const float* res, int res_cs, float* partial, void* stream) {
    kpn_enc_conv_args a = l.fwd.a;
    layer_source(a, l, src, src_cs, ss);
    a.wp = wp; a.bias = bias; a.dst = dst; a.dst_cs = dst_cs; a.res = res; a.res_cs = res_cs;
    a.partial = l.fwd.partial ? partial : nullptr;
    launch_conv(a, l.fwd, l.s.stem, stream);
}
// dn (N, Hi, Wi, cin) = the layer's input gradient of R (N, Ho, Wo, cout) [+ res], over the second packed copy
inline void layer_dgrad(const Layer& l, const float* R, int r_cs, const float* wp, float* dn, int dn_cs, const float* res, int res_cs,
                        float* partial, void* stream) {
    kpn_enc_conv_args a = l.dx.a;
    a.src = R; a.src_cs = r_cs;
    a.wp = wp + l.fwd.packed; a.dst = dn; a.dst_cs = dn_cs; a.res = res; a.res_cs = res_cs;
    a.partial = l.dx.partial ? partial : nullptr;
    if (l.s.replicate) { a.Hs = l.Hi; a.Ws = l.Wi; a.stride = 1; a.pad = l.s.pad; launch_conv_rp_adjoint(a, l.dx, stream); return; }
    a.Hs = l.Ho; a.Ws = l.Wo;
    if (l.s.transposed) { a.stride = 2; a.pad = 1; }                                  // the stride-2 GEMM
    else if (l.s.stride == 2) { a.stride = 1; a.pad = 0; }                            // the DECONV GEMM
    else { a.stride = 1; a.pad = l.s.k - 1 - l.s.pad; }                               // conv(R, w'[ci][co][k - 1 - ky][k - 1 - kx], pad k - 1 - p)
    launch_conv(a, l.dx, 0, stream);
}
// dw = the layer's weight gradient for R = dL/dy and its input src [normalised and rectified in the loads with ss]
inline void layer_wgrad(const Layer& l, const float* src, int src_cs, const float* ss, const float* R, int r_cs, float* partial, float* dw,
                        void* stream) {
    kpn_enc_conv_args c = l.wg.a;
    if (l.s.transposed) {               // the swapped roles: A from R with stride 2, rhs = the layer's input
        c.Hs = l.Ho; c.Ws = l.Wo; c.stride = 2; c.pad = 1; c.src = R; c.src_cs = r_cs;
        launch_wgrad(c, l.wg, l.wgp, 0, src, src_cs, partial, dw, stream, ss);
    } else {
        layer_source(c, l, src, src_cs, ss);
        launch_wgrad(c, l.wg, l.wgp, l.s.stem, R, r_cs, partial, dw, stream);
    }
}
inline bool aligned16(std::initializer_list<const void*> ps) {
    uintptr_t u = 0;
    for (const void* q : ps) u |= (uintptr_t)q;
    return (u & 15) == 0;
}

// ---- A single layer as six entry points: <name>_packed_floats / _pack_device / _workspace_bytes / _wgrad_ranges / _forward / _backward.
// A family F gives Desc, weight_error (what the packed copies depend on), desc_error, spec_of, and nchw_stem: whether one of its kinds is a
// stem, named stem_name, whose x is an NCHW tensor of any alignment.
// the workspace: the forward and the backward never run at once on it: the larger of the two
struct SingleLayerWorkspace { size_t o_fwd, o_dx, o_wg, o_db, bytes; };
inline SingleLayerWorkspace single_layer_workspace(const Layer& l) {
    SingleLayerWorkspace w{};
    Carver f, b;
    w.o_fwd = f.take((size_t)l.fwd.partial * sizeof(float));
    w.o_dx = b.take((size_t)l.dx.partial * sizeof(float));
    w.o_wg = b.take((size_t)l.wgp.partial * sizeof(float));
    w.o_db = b.take((size_t)dbias_chunks(l.My) * l.s.cout * sizeof(double));
    w.bytes = std::max<size_t>(std::max(f.o, b.o), 256);
    return w;
}
inline int single_fail(const char* name, const char* e) { return fail(KPN_EINVAL, std::string(name) + "_desc: " + e); }
// `arith`: the arithmetic of the layer's GEMMs, checked by the caller (the _ex entry points of api_conv.hip; every other family passes
// none and runs KPN_CONV_F32)
inline const char* arith_error(int32_t arith) {
    return arith == KPN_CONV_F32 || arith == KPN_CONV_BF16X3 ? nullptr : "arith must be KPN_CONV_F32 (0) or KPN_CONV_BF16X3 (1)";
}
template <class F> LayerSpec single_spec(const typename F::Desc* d, int arith) { LayerSpec s = F::spec_of(d); s.arith = arith; return s; }
template <class F> Layer single_layer(const typename F::Desc* d, int arith) { return layer(single_spec<F>(d, arith), d->N, d->H, d->W); }
template <class F> size_t single_packed_floats(const typename F::Desc* desc, int arith = KPN_CONV_F32) {
    return F::weight_error(desc) ? 0 : pack_layer(single_spec<F>(desc, arith)).packed_floats;
}
template <class F> int single_pack(const char* name, const char* what, const typename F::Desc* desc, const float* w, float* packed, void* stream,
                                   int arith = KPN_CONV_F32) {
    if (const char* e = F::weight_error(desc)) return single_fail(name, e);
    KPN_REQUIRE(w && packed, "null pointer");
    KPN_REQUIRE(((uintptr_t)packed & 15) == 0, "packed must be 16-byte aligned");
    layer_pack(pack_layer(single_spec<F>(desc, arith)), w, packed, stream);
    return check_launch(what);
}
template <class F> size_t single_workspace_bytes(const typename F::Desc* desc, int arith = KPN_CONV_F32) {
    return F::desc_error(desc) ? 0 : single_layer_workspace(single_layer<F>(desc, arith)).bytes;
}
template <class F> int32_t single_wgrad_ranges(const typename F::Desc* desc, int arith = KPN_CONV_F32) {
    return F::desc_error(desc) ? 0 : single_layer<F>(desc, arith).wgp.nranges;
}
// the alignment and workspace requirements of the forward (dy NULL, lead "") and the backward (lead "dy / ")
template <class F> int single_require(const char* name, const Layer& l, const SingleLayerWorkspace& w, const char* lead, const void* x,
                                      const void* dy, const void* packed, const void* workspace, size_t workspace_bytes) {
    if constexpr (F::nchw_stem) {
        KPN_REQUIRE(aligned16({dy, packed, workspace}), std::string(lead) + "packed / workspace must be 16-byte aligned");
        KPN_REQUIRE(l.s.stem || ((uintptr_t)x & 15) == 0, "x must be 16-byte aligned");
    } else {
        KPN_REQUIRE(aligned16({x, dy, packed, workspace}), std::string("x / ") + lead + "packed / workspace must be 16-byte aligned");
    }
    KPN_REQUIRE(workspace_bytes >= w.bytes, std::string("workspace too small (") + name + "_workspace_bytes)");
    return KPN_OK;
}
template <class F> int single_forward(const char* name, const char* what, const typename F::Desc* desc, const float* x, const float* packed,
                                      const float* bias, float* y, void* workspace, size_t workspace_bytes, void* stream,
                                      int arith = KPN_CONV_F32) {
    if (const char* e = F::desc_error(desc)) return single_fail(name, e);
    KPN_REQUIRE(x && packed && y && workspace, "null pointer");
    KPN_REQUIRE((bias != nullptr) == (desc->has_bias != 0), "bias must be given exactly when has_bias is set");
    const Layer l = single_layer<F>(desc, arith);
    const SingleLayerWorkspace w = single_layer_workspace(l);
    if (const int rc = single_require<F>(name, l, w, "", x, nullptr, packed, workspace, workspace_bytes)) return rc;
    float* partial = reinterpret_cast<float*>(static_cast<char*>(workspace) + w.o_fwd);
    layer_forward(l, x, l.s.cin, nullptr, packed, bias, y, l.s.cout, nullptr, 0, partial, stream);
    return check_launch(what);
}
template <class F> int single_backward(const char* name, const char* what, const typename F::Desc* desc, const float* x, const float* dy,
                                       const float* packed, float* dx, float* dw, float* db, void* workspace, size_t workspace_bytes,
                                       void* stream, int arith = KPN_CONV_F32) {
    if (const char* e = F::desc_error(desc)) return single_fail(name, e);
    KPN_REQUIRE(dy && workspace, "null pointer");
    const Layer l = single_layer<F>(desc, arith);
    if constexpr (F::nchw_stem) KPN_REQUIRE(!dx || l.has_dx, std::string("dx must be NULL for ") + F::stem_name + " (the stem has no input gradient)");
    KPN_REQUIRE(!dx || packed, "packed is null (the input gradient reads it)");
    KPN_REQUIRE(!dw || x, "x is null (the weight gradient reads it)");
    KPN_REQUIRE(!db || desc->has_bias, "db given for a convolution without bias (has_bias)");
    const SingleLayerWorkspace w = single_layer_workspace(l);
    if (const int rc = single_require<F>(name, l, w, "dy / ", x, dy, packed, workspace, workspace_bytes)) return rc;
    char* ws = static_cast<char*>(workspace);
    if (dx) layer_dgrad(l, dy, l.s.cout, packed, dx, l.s.cin, nullptr, 0, reinterpret_cast<float*>(ws + w.o_dx), stream);
    if (dw) layer_wgrad(l, x, l.s.cin, nullptr, dy, l.s.cout, reinterpret_cast<float*>(ws + w.o_wg), dw, stream);
    if (db) launch_dbias(dy, l.My, l.s.cout, reinterpret_cast<double*>(ws + w.o_db), db, stream);
    return check_launch(what);
}
}  // namespace enc

// the six entry points of the family F, under its name
#define KPN_SINGLE_LAYER(F, name) \
    extern "C" size_t name##_packed_floats(const F::Desc* desc) { return enc::single_packed_floats<F>(desc); } \
    extern "C" int name##_pack_device(const F::Desc* desc, const float* w, float* packed, void* stream) { \
        return enc::single_pack<F>(#name, #name "_pack_device", desc, w, packed, stream); \
    } \
    extern "C" size_t name##_workspace_bytes(const F::Desc* desc) { return enc::single_workspace_bytes<F>(desc); } \
    extern "C" int32_t name##_wgrad_ranges(const F::Desc* desc) { return enc::single_wgrad_ranges<F>(desc); } \
    extern "C" int name##_forward(const F::Desc* desc, const float* x, const float* packed, const float* bias, float* y, void* workspace, \
                                  size_t workspace_bytes, void* stream) { \
        return enc::single_forward<F>(#name, #name "_forward", desc, x, packed, bias, y, workspace, workspace_bytes, stream); \
    } \
    extern "C" int name##_backward(const F::Desc* desc, const float* x, const float* dy, const float* packed, float* dx, float* dw, float* db, \
                                   void* workspace, size_t workspace_bytes, void* stream) { \
        return enc::single_backward<F>(#name, #name "_backward", desc, x, dy, packed, dx, dw, db, workspace, workspace_bytes, stream); \
    }

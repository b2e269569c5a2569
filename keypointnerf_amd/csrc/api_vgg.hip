// ---------------------------------------------------------------------------------------------
// VGGLoss (reference src/utils.py:750-805): vgg19.features[0:21] on normalize(x) and normalize(y), the four relu taps' L1
// distances, and d loss / d x.  Kernels: vgg_kernels.hip.
namespace {
struct vgg_layer { int cin, cout, level, pooled_in; };
constexpr vgg_layer kVgg[KPN_VGG_LAYERS] = {{3, 64, 0, 0},    {64, 64, 0, 0},    {64, 128, 1, 1},   {128, 128, 1, 0}, {128, 256, 2, 1},
                                            {256, 256, 2, 0}, {256, 256, 2, 0}, {256, 256, 2, 0}, {256, 512, 3, 1}};
constexpr int kVggTap[4] = {0, 2, 4, 8};   // relu1_1, relu2_1, relu3_1, relu4_1
constexpr int kVggBlocks = 1024;           // packer grid (grid-stride)

kpn_vgg_pack_table vgg_table() {
    kpn_vgg_pack_table tb{};
    int64_t plain = 0, off = 0;
    for (int l = 0; l < KPN_VGG_LAYERS; ++l) {
        kpn_vgg_pack_layer& s = tb.l[l];
        s.cin = kVgg[l].cin; s.cout = kVgg[l].cout;
        s.gf = (s.cin + 15) / 16; s.gb = s.cout / 16; s.cin_p = (s.cin + 31) / 32 * 32;
        s.plain = plain; plain += (int64_t)s.cout * s.cin * 9 + s.cout;
        s.fwd = off; off += (int64_t)9 * s.gf * s.cout * 16;
        s.bias = off; off += s.cout;
        s.bwd = off; off += (int64_t)9 * s.gb * s.cin_p * 16;
    }
    tb.total = off;
    return tb;
}
int64_t vgg_plain_floats() {
    int64_t n = 0;
    for (const vgg_layer& l : kVgg) n += (int64_t)l.cout * l.cin * 9 + l.cout;
    return n;
}
struct vgg_plan {
    int64_t act[KPN_VGG_LAYERS];   // offsets (floats) of A_l, (2B, H_l, W_l, C_l) NHWC, contiguous = the `stages` layout
    int64_t act_total, grad_floats, grad0, grad1, partial, ticket, bytes;
};
vgg_plan vgg_make_plan(int B, int H, int W) {
    vgg_plan p{};
    int64_t off = 0;
    for (int l = 0; l < KPN_VGG_LAYERS; ++l) {
        p.act[l] = off;
        off += (int64_t)2 * B * (H >> kVgg[l].level) * (W >> kVgg[l].level) * kVgg[l].cout;
    }
    p.act_total = off;
    p.grad_floats = (int64_t)B * H * W * 64;   // the largest dIn_l (l = 2: A_1's resolution, 64 channels)
    p.grad0 = off; off += p.grad_floats;
    p.grad1 = off; off += p.grad_floats;
    p.partial = (int64_t)align_up((size_t)off * 4, 256);
    p.ticket = p.partial + 4 * KPN_VGG_L1_BLOCKS * 8;
    p.bytes = p.ticket + 256;
    return p;
}
bool vgg_shape_ok(int B, int H, int W) {
    return B >= 1 && H >= 8 && W >= 8 && (int64_t)2 * B * H * W * 64 < (1ll << 31);
}
dim3 vgg_conv_grid(int64_t npx, int cout_p) { return dim3((unsigned)((npx + 15) / 16 * (cout_p / 32))); }
}  // namespace

extern "C" size_t kpn_vgg_plain_floats(void) { return (size_t)vgg_plain_floats(); }
extern "C" size_t kpn_vgg_packed_floats(void) { return (size_t)vgg_table().total; }
extern "C" int kpn_vgg_pack_device(const float* plain, float* packed, void* stream) {
    KPN_REQUIRE(plain && packed, "null pointer");
    KPN_REQUIRE(((uintptr_t)packed & 15) == 0, "packed must be 16-byte aligned");
    KPN_LAUNCH(k_vgg_pack, dim3(kVggBlocks), dim3(256), stream, vgg_table(), plain, packed);
    return check_launch("kpn_vgg_pack_device");
}
extern "C" size_t kpn_vgg_workspace_bytes(int32_t B, int32_t H, int32_t W) {
    return vgg_shape_ok(B, H, W) ? (size_t)vgg_make_plan(B, H, W).bytes : 0;
}
extern "C" size_t kpn_vgg_stage_floats(int32_t B, int32_t H, int32_t W) {
    return vgg_shape_ok(B, H, W) ? (size_t)vgg_make_plan(B, H, W).act_total : 0;
}
extern "C" int kpn_vgg_loss(const float* x, const float* y, int32_t B, int32_t H, int32_t W, const float* packed,
                            const float* mean_host, const float* std_host, const float* tap_w_host, float lambda, float* loss,
                            float* d_x, float* stages, void* workspace, size_t workspace_bytes, void* stream) {
    KPN_REQUIRE(x && y && packed && mean_host && std_host && tap_w_host && loss && workspace, "null pointer");
    KPN_REQUIRE(vgg_shape_ok(B, H, W), "VGG loss needs B >= 1 and H, W >= 8 (three 2x2 pools)");
    KPN_REQUIRE(((uintptr_t)packed & 15) == 0 && ((uintptr_t)workspace & 15) == 0, "packed / workspace must be 16-byte aligned");
    const vgg_plan pl = vgg_make_plan(B, H, W);
    KPN_REQUIRE(workspace_bytes >= (size_t)pl.bytes, "workspace too small (kpn_vgg_workspace_bytes)");
    const kpn_vgg_pack_table tb = vgg_table();
    float* ws = static_cast<float*>(workspace);
    char* wsb = static_cast<char*>(workspace);
    (void)hipMemsetAsync(wsb + pl.ticket, 0, sizeof(int), (hipStream_t)stream);

    kpn_vgg_conv_args base{};
    base.x = x; base.y = y; base.B = B;
    for (int c = 0; c < 3; ++c) { base.mean[c] = mean_host[c]; base.stdv[c] = std_host[c]; }
    // forward over the 2B images
    for (int l = 0; l < KPN_VGG_LAYERS; ++l) {
        kpn_vgg_conv_args a = base;
        a.nimg = 2 * B; a.H = H >> kVgg[l].level; a.W = W >> kVgg[l].level;
        a.groups = tb.l[l].gf; a.cout = a.cout_p = kVgg[l].cout;
        a.wp = packed + tb.l[l].fwd; a.bias = packed + tb.l[l].bias;
        a.out = ws + pl.act[l];
        const dim3 grid = vgg_conv_grid((int64_t)a.nimg * a.H * a.W, a.cout_p);
        if (l == 0) {
            KPN_LAUNCH(k_vgg_conv<0>, grid, dim3(256), stream, a);
        } else {
            a.src = ws + pl.act[l - 1]; a.csrc = kVgg[l - 1].cout;
            a.Hs = H >> kVgg[l - 1].level; a.Ws = W >> kVgg[l - 1].level;
            if (kVgg[l].pooled_in) KPN_LAUNCH(k_vgg_conv<2>, grid, dim3(256), stream, a);
            else KPN_LAUNCH(k_vgg_conv<1>, grid, dim3(256), stream, a);
        }
    }
    kpn_vgg_l1_args la{};
    double seed[4];
    for (int t = 0; t < 4; ++t) {
        const int l = kVggTap[t];
        la.act[t] = ws + pl.act[l];
        la.n[t] = (int64_t)B * (H >> kVgg[l].level) * (W >> kVgg[l].level) * kVgg[l].cout;
        la.w[t] = (double)tap_w_host[t];
        seed[t] = (double)lambda * (double)tap_w_host[t] / (double)la.n[t];
    }
    la.lambda = (double)lambda;
    la.partial = reinterpret_cast<double*>(wsb + pl.partial);
    la.ticket = reinterpret_cast<int*>(wsb + pl.ticket);
    la.loss = loss;
    KPN_LAUNCH(k_vgg_l1, dim3(KPN_VGG_L1_BLOCKS, 4), dim3(256), stream, la);
    if (stages) (void)hipMemcpyAsync(stages, ws, (size_t)pl.act_total * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream);
    if (d_x) {
        // backward for the B x images, layer 9 down to 1; dIn_l alternates between the two gradient buffers
        const float* up = nullptr;
        for (int l = KPN_VGG_LAYERS - 1; l >= 0; --l) {
            kpn_vgg_conv_args a = base;
            a.nimg = B; a.H = H >> kVgg[l].level; a.W = W >> kVgg[l].level;
            a.groups = tb.l[l].gb; a.cout = kVgg[l].cin; a.cout_p = tb.l[l].cin_p;
            a.wp = packed + tb.l[l].bwd;
            a.src = ws + pl.act[l]; a.csrc = kVgg[l].cout;
            a.up = up;
            if (up) {
                a.up_pool = kVgg[l + 1].pooled_in;
                a.Hu = H >> kVgg[l + 1].level; a.Wu = W >> kVgg[l + 1].level;
            }
            for (int t = 0; t < 4; ++t)
                if (kVggTap[t] == l) { a.tap = 1; a.seed = (float)seed[t]; }
            a.final_ = l == 0;
            a.out = l == 0 ? d_x : ws + ((KPN_VGG_LAYERS - 1 - l) % 2 ? pl.grad1 : pl.grad0);
            KPN_LAUNCH(k_vgg_conv<3>, vgg_conv_grid((int64_t)a.nimg * a.H * a.W, a.cout_p), dim3(256), stream, a);
            up = a.out;
        }
    }
    return check_launch("kpn_vgg_loss");
}

// ---------------------------------------------------------------------------------------------
// GroupNorm / InstanceNorm2d [+ ReLU] of the image encoders, forward and backward (torch.nn.functional.group_norm [+ relu] and
// their autograd as the legs of ConvBlock and ResBlkEncoder call them: reference src/utils.py:416-474, 199-247).  Kernels:
// encoder_kernels.hip.  The forward is the encoder walk's own statistics and affine kernels, launched through the launch layer at
// the head of api_encoders.hip (enc::stats_chunks / enc::launch_stats / enc::launch_affine), with the statistics kept for the
// backward; the backward is k_enc_norm_bwd_partial / _final / _dx over the same chunks.
namespace gnorm {
const char* desc_error(const kpn_group_norm_desc* d) {
    if (!d) return "desc is null";
    if (d->C < 4 || d->C > 1024 || (d->C & (d->C - 1))) return "C must be a power of two in 4 .. 1024";
    if (d->G < 1 || d->C % d->G) return "G must divide C";
    if (d->N < 1 || d->H < 1 || d->W < 1) return "N, H, W must be positive";
    if (d->N > 65535) return "N must be at most 65535 (one grid row per image)";
    if ((int64_t)d->N * d->H * d->W * d->C >= (1ll << 31)) return "N * H * W * C must stay below 2^31";
    if (!(d->eps > 0.0f)) return "eps must be positive";
    if (d->affine != 0 && d->affine != 1) return "affine must be 0 or 1";
    if (d->relu != 0 && d->relu != 1) return "relu must be 0 or 1";
    return nullptr;
}
struct Plan {
    int HW, nchunks;
    size_t o_partial, o_coef, bytes;
};
Plan plan(const kpn_group_norm_desc* d) {
    Plan p{};
    p.HW = d->H * d->W;
    int64_t pd;
    p.nchunks = enc::stats_chunks(d->N, p.HW, d->C, &pd);
    // the forward's (sum, sum of squares) and the backward's (A, B) partials have one size and never live at once
    Carver c;
    p.o_partial = c.take((size_t)pd * sizeof(double));
    p.o_coef = c.take((size_t)3 * d->N * d->C * sizeof(float));
    p.bytes = c.o;
    return p;
}
}  // namespace gnorm

#define KPN_NORM_REQUIRE_DESC(desc) do { if (const char* e_ = gnorm::desc_error(desc)) return fail(KPN_EINVAL, std::string("kpn_group_norm_desc: ") + e_); } while (0)

extern "C" size_t kpn_group_norm_stats_floats(const kpn_group_norm_desc* desc) {
    return gnorm::desc_error(desc) ? 0 : (size_t)2 * desc->N * desc->C + (size_t)2 * desc->N * desc->G;
}
extern "C" size_t kpn_group_norm_workspace_bytes(const kpn_group_norm_desc* desc) {
    return gnorm::desc_error(desc) ? 0 : gnorm::plan(desc).bytes;
}
extern "C" int kpn_group_norm_forward(const kpn_group_norm_desc* desc, const float* x, const float* gamma, const float* beta, float* y,
                                      float* stats, void* workspace, size_t workspace_bytes, void* stream) {
    KPN_NORM_REQUIRE_DESC(desc);
    KPN_REQUIRE(x && y && stats && workspace, "null pointer");
    KPN_REQUIRE((gamma != nullptr) == (desc->affine != 0) && (beta != nullptr) == (desc->affine != 0),
                "gamma and beta must be given exactly when affine is set");
    KPN_REQUIRE((((uintptr_t)x | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)y | (uintptr_t)stats | (uintptr_t)workspace) & 15) == 0,
                "x / gamma / beta / y / stats / workspace must be 16-byte aligned");
    const gnorm::Plan p = gnorm::plan(desc);
    KPN_REQUIRE(workspace_bytes >= p.bytes, "workspace too small (kpn_group_norm_workspace_bytes)");
    kpn_enc_stats_args a{};
    a.src = x; a.cs = desc->C; a.C = desc->C; a.HW = p.HW; a.nchunks = p.nchunks; a.nimg = desc->N;
    a.partial = reinterpret_cast<double*>(static_cast<char*>(workspace) + p.o_partial);
    a.G = desc->G; a.gamma = gamma; a.beta = beta; a.eps = desc->eps;
    a.ss = stats; a.mr = stats + (size_t)2 * desc->N * desc->C;
    enc::launch_stats(a, stream);
    enc::launch_affine(x, stats, desc->relu, nullptr, y, desc->N, p.HW, desc->C, stream);
    return check_launch("kpn_group_norm_forward");
}
extern "C" int kpn_group_norm_backward(const kpn_group_norm_desc* desc, const float* x, const float* dy, const float* gamma, const float* stats,
                                       float* dx, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, void* stream) {
    KPN_NORM_REQUIRE_DESC(desc);
    KPN_REQUIRE(x && dy && stats && workspace, "null pointer");
    KPN_REQUIRE((gamma != nullptr) == (desc->affine != 0), "gamma must be given exactly when affine is set");
    KPN_REQUIRE((!dgamma && !dbeta) || desc->affine, "dgamma / dbeta given for a norm without affine parameters (affine)");
    KPN_REQUIRE((((uintptr_t)x | (uintptr_t)dy | (uintptr_t)gamma | (uintptr_t)stats | (uintptr_t)dx | (uintptr_t)dgamma | (uintptr_t)dbeta |
                  (uintptr_t)workspace) & 15) == 0, "x / dy / gamma / stats / dx / dgamma / dbeta / workspace must be 16-byte aligned");
    const gnorm::Plan p = gnorm::plan(desc);
    KPN_REQUIRE(workspace_bytes >= p.bytes, "workspace too small (kpn_group_norm_workspace_bytes)");
    if (!dx && !dgamma && !dbeta) return KPN_OK;
    char* ws = static_cast<char*>(workspace);
    kpn_enc_norm_bwd_args a{};
    a.x = x; a.x_cs = desc->C; a.dy = dy; a.ss = stats; a.mr = stats + (size_t)2 * desc->N * desc->C; a.gamma = gamma;
    a.relu = desc->relu; a.C = desc->C; a.HW = p.HW; a.nchunks = p.nchunks; a.nimg = desc->N; a.G = desc->G;
    a.partial = reinterpret_cast<double*>(ws + p.o_partial);
    a.coef = dx ? reinterpret_cast<float*>(ws + p.o_coef) : nullptr;
    a.dx = dx; a.dgamma = dgamma; a.dbeta = dbeta;
    enc::launch_norm_bwd(a, stream);
    return check_launch("kpn_group_norm_backward");
}

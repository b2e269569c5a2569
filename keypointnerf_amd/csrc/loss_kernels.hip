// loss_kernels.hip — the training loss: every pixel and mask term in one launch (kpn_train_loss, include/kpnerf.h), and the L1 term
// alone (kpn_pix_l1_loss).  Both kernels sum through the one reduction of kpn_reduce.h and take their L1 elements from the one
// kpn_l1_elem below.
//
// compute_error_nerf (reference src/utils.py:108-171) for the outputs the renderer produces: the coarse L1 term, the fine
// pix_loss terms l1 / l2 / lp (src/utils.py:173-183) and the two mask losses (:150-158), each with the gradient torch autograd
// derives for it for an upstream gradient of 1 — the seed gradients of kpn_render_rays_train_backward (d_tex_fg, d_tex_fg_fine,
// d_alpha, d_alpha_fine).  The work is latency, not bandwidth (a 64 x 64 patch is 12,288 + 4,096 floats per prediction): one
// launch instead of one per term, and nothing at all in the backward.
//
// Arithmetic.  The L1 terms call the same function as k_pix_l1 for every element (kpn_l1_elem), on the same grid (reduce_blocks,
// api_common.h) and through the same reduction, so their values and gradients are bit-identical to kpn_pix_l1_loss.
// l2, lp and the mask terms are evaluated per element in fp64 on the fp32 inputs and rounded once: the
// power goes through the fp64 libm pow, not through v_log_f32 / v_exp_f32 — those are ~1 ulp each on their RESULT, and the
// logarithm of |d| + 1e-4 reaches -13, so x^-0.6 = 2^(-0.6 log2 x) would carry ~8e-7 relative error (a dozen ulps) against the
// 1-2 ulps of torch's powf; at 12,288 elements the fp64 pow costs nothing that a launch does not cost many times over.
// Decisions (sign(d), the clamp's pass band) are taken on the fp32 values, as torch takes them.
struct kpn_loss_kargs {
    kpn_train_loss_args a;
    double* partial;   // [gridDim.x][6]
    int* ticket;       // 0 on entry; the last block leaves it at 0 again
};

// |src - tar| into the fp64 sum, and d |src - tar| / d src times gscale (sign(0) = 0, torch's abs backward)
__device__ __forceinline__ void kpn_l1_elem(float src, float tar, float gscale, double& acc, float* __restrict__ d_out) {
    const float d = KSUB(src, tar);
    acc += (double)fabsf(d);
    if (d_out) *d_out = d > 0.0f ? gscale : (d < 0.0f ? -gscale : 0.0f);
}
// clip(a, 1e-3, 1) as torch.clamp evaluates it in fp32 (a NaN stays a NaN) and its pass band (clamp backward: both ends inclusive)
__device__ __forceinline__ void kpn_mask_elem(float a, float t, double gscale, double& acc, float* __restrict__ d_out) {
    const float c = a < 1e-3f ? 1e-3f : (a > 1.0f ? 1.0f : a);
    const double e = (double)c - (double)t;
    acc += e * e;
    if (d_out) *d_out = (a >= 1e-3f && a <= 1.0f) ? (float)(gscale * e) : 0.0f;
}

// pix_loss's L1 term (reference src/utils.py:164-168): loss = lambda * mean|src - tar|, and what autograd derives for it,
// d loss / d src = lambda * sign(src - tar) / n (sign(0) = 0, torch's abs backward) — the seed gradient of
// kpn_render_rays_train_backward for tex_fg (lambda_l1_c, coarse) and tex_fg_fine (lambda_l1, fine), src/utils.py:128-145.
__global__ __launch_bounds__(256) void k_pix_l1(int64_t n, float lambda, const float* __restrict__ src, const float* __restrict__ tar,
                                                double* __restrict__ partial, int* __restrict__ ticket, float* __restrict__ loss,
                                                float* __restrict__ d_src) {
    __shared__ double red[1][256];
    double acc[1] = {0.0};
    const float gscale = lambda / (float)n;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        kpn_l1_elem(src[i], tar[i], gscale, acc[0], d_src ? d_src + i : nullptr);
    if (kpn_block_sums_last(acc, red, partial, ticket, blockIdx.x, gridDim.x, threadIdx.x == 0)) {
        const double tot = kpn_partials_in_order(partial, gridDim.x, 1, 0);
        loss[0] = lambda * (float)(tot / (double)n);
    }
}

__global__ __launch_bounds__(256) void k_train_loss(kpn_loss_kargs k) {
    __shared__ double red[6][256];
    const kpn_train_loss_args& a = k.a;
    const int64_t n = a.n, n3 = 3 * a.n;
    const bool on_c = a.tex && a.tar && a.l1_c > 0.0f;
    const bool on_l1 = a.tex_fine && a.tar && a.l1 > 0.0f, on_l2 = a.tex_fine && a.tar && a.l2 > 0.0f, on_lp = a.tex_fine && a.tar && a.lp > 0.0f;
    const bool on_mc = a.alpha && a.tar_alpha && a.mloss > 0.0f, on_mf = a.alpha_fine && a.tar_alpha && a.mloss > 0.0f;
    const float g_c = a.l1_c / (float)n3, g_l1 = a.l1 / (float)n3;                       // k_pix_l1's gscale, lambda / n
    const double g_l2 = 2.0 * (double)a.l2 / (double)n3, g_lp = 0.4 * (double)a.lp / (double)n3, g_m = 2.0 * (double)a.mloss / (double)n;
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n3; i += (int64_t)gridDim.x * blockDim.x) {
        if (on_c) kpn_l1_elem(a.tex[i], a.tar[i], g_c, acc[0], a.d_tex ? a.d_tex + i : nullptr);
        if (on_l1 | on_l2 | on_lp) {
            const float s = a.tex_fine[i], t = a.tar[i];
            const float d = KSUB(s, t);
            const double dd = (double)s - (double)t;                                     // exact; same sign as d
            float* g = a.d_tex_fine ? a.d_tex_fine + i : nullptr;
            if (on_l1) kpn_l1_elem(s, t, g_l1, acc[1], g);
            if (on_l2) {
                acc[2] += dd * dd;
                if (g) g[n3] = (float)(g_l2 * dd);
            }
            if (on_lp) {
                const double x = fabs(dd) + 1e-4;
                const double pw = pow(x, 0.4);
                acc[3] += pw;
                if (g) g[2 * n3] = d > 0.0f ? (float)(g_lp * pw / x) : (d < 0.0f ? -(float)(g_lp * pw / x) : 0.0f);   // sign(0) = 0
            }
        }
        if (i < n) {
            if (on_mc) kpn_mask_elem(a.alpha[i], a.tar_alpha[i], g_m, acc[4], a.d_alpha ? a.d_alpha + i : nullptr);
            if (on_mf) kpn_mask_elem(a.alpha_fine[i], a.tar_alpha[i], g_m, acc[5], a.d_alpha_fine ? a.d_alpha_fine + i : nullptr);
        }
    }
    if (kpn_block_sums_last(acc, red, k.partial, k.ticket, blockIdx.x, gridDim.x, threadIdx.x < 6)) {
        const int q = (int)threadIdx.x;
        const double tot = kpn_partials_in_order(k.partial, gridDim.x, 6, q);
        float v;
        if (q == 0) v = a.l1_c * (float)(tot / (double)n3);                               // k_pix_l1's last line
        else if (q == 1) v = a.l1 * (float)(tot / (double)n3);
        else if (q == 2) v = (float)((double)a.l2 * tot / (double)n3);
        else if (q == 3) v = (float)((double)a.lp * tot / (double)n3);
        else v = (float)((double)a.mloss * tot / (double)n);
        a.terms[q] = v;
        // every block has taken its ticket: nobody reads the word again in this launch, and the next launch on the
        // workspace is ordered after this one — the workspace is ready for it without a memset
        if (q == 0) *k.ticket = 0;
    }
}

// param_kernels.hip — the parameter leg of a training step, three launches (kpn_fold_params, kpn_fold_params_backward, kpn_adam_step;
// include/kpnerf.h): the live parameter tensors -> the flat effective-parameter vector (weight-norm fold + concatenation), the
// vector's gradient -> the gradients of the live tensors, and one multi-tensor Adam step.  They replace, per step, five
// torch._weight_norm calls, 38 reshapes and a cat (weights.plain_tensor_from_module), their autograd graph, and torch.optim.Adam's
// launches over 44 tensors of a few hundred elements each.
//
// Work: the layer table has 864 rows, 4 to 232 wide.  Fold and fold backward run one 64-thread block (one wave) per row: a lane
// takes columns lane, lane + 64, ...; a row's fp64 sum is added over the lanes by a fixed LDS tree (32, 16, ... 1), so the result
// does not depend on anything but the inputs.  Lane 0 of a row's block also moves the row's bias element, block 0 moves ani_al.
// Adam runs one thread per element; a block finds its segment in a table of first blocks.  No atomics, no inline assembly.
//
// Arithmetic.  Fold: n = sqrt(sum v^2) and g / n in fp64, s = (float)(g / n), W = v * s (one fp32 multiply): two roundings per
// element.  Backward: dot = sum dW v in fp64, dg = (float)(dot / n), dv = s dW - c v with c = (float)(g dot / n^3) formed in fp64;
// the two products and the difference are separate fp32 operations.  n is kept in fp64 for the backward (a rounded n would enter c
// three times).  Adam evaluates every element in fp64 on the fp32 state and rounds m, v and p once each.
// A row of zero norm divides by zero exactly as torch._weight_norm and its backward do (inf / NaN); it is not special-cased and
// not tested.
struct kpn_fold_layer { int row0, cols, w_off, b_off, norm0; };   // first row of the layer, its width, offsets in plain, first norm slot
struct kpn_fold_kargs {
    kpn_param_table p;                         // the live parameters (read)
    kpn_param_table d;                         // backward: where their gradients go (any entry may be null)
    kpn_fold_layer layer[KPN_PARAM_LAYERS];
    int ani_off, accumulate;
    float* plain;                              // forward: out
    const float* d_plain;                      // backward: in
    double* norm_n;                            // [normed rows]
    float* norm_s;                             // [normed rows]
    int n_kpt, sp_level;                       // the MAPPED kernels: layer 0's v_or_w (p and d) is the narrow (rows, D + 64) tensor
};
// Keypoint sets (include/kpnerf.h): canonical column c of layers1.0's input -> the column of an (n_kpt, sp_level) model's narrow
// weight, or -1 for a padded column (block t > 2 sp_level or keypoint k >= n_kpt)
__host__ __device__ inline int kpn_narrow_col(int c, int n_kpt, int sp_level) {
    if (c >= 7 * KPN_NKPT) return (1 + 2 * sp_level) * n_kpt + (c - 7 * KPN_NKPT);
    const int t = c / KPN_NKPT, k = c - KPN_NKPT * t;
    return (t <= 2 * sp_level && k < n_kpt) ? t * n_kpt + k : -1;
}
// and back: narrow column m -> its canonical column
__host__ __device__ inline int kpn_canonical_col(int m, int n_kpt, int sp_level) {
    const int D = (1 + 2 * sp_level) * n_kpt;
    if (m >= D) return 7 * KPN_NKPT + (m - D);
    const int t = m / n_kpt;
    return KPN_NKPT * t + (m - t * n_kpt);
}
struct kpn_adam_kargs {
    kpn_adam_segment seg[KPN_ADAM_MAX_SEGMENTS];
    int block0[KPN_ADAM_MAX_SEGMENTS + 1];     // first block of each segment; block0[n_seg] = the grid
    int n_seg;
    double one_minus_b1, b2, one_minus_b2, wd, step_size, bc2_sqrt, eps;
};

// the sum of x over the 64 threads of the block, in a fixed order; every thread calls it and gets the sum
__device__ __forceinline__ double kpn_row_sum(double x, double (&red)[64]) {
    red[threadIdx.x] = x;
    __syncthreads();
    for (int s = 32; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}
__device__ __forceinline__ int kpn_fold_layer_of(const kpn_fold_kargs& k, int row) {
    int l = 0;
    while (l + 1 < KPN_PARAM_LAYERS && row >= k.layer[l + 1].row0) ++l;
    return l;
}

// MAPPED (kpn_fold_params_shape): layer 0's rows are narrow; the thread that owns canonical column j loads the narrow column mapped
// to it, or 0 - everything behind the load is the unmapped kernel's, so the results are those of the widened tensor, bit for bit
template <bool MAPPED>
__global__ __launch_bounds__(64) void k_fold_params(kpn_fold_kargs k) {
    __shared__ double red[64];
    const int row = (int)blockIdx.x, lane = (int)threadIdx.x;
    const int l = kpn_fold_layer_of(k, row);
    const kpn_fold_layer L = k.layer[l];
    const int r = row - L.row0;
    const bool mapped = MAPPED && l == 0;                              // block-uniform
    const int pitch = mapped ? kpn_narrow_col(L.cols, k.n_kpt, k.sp_level) : L.cols;
    const float* __restrict__ src = k.p.v_or_w[l] + (size_t)r * pitch;
    auto ld = [&](const float* __restrict__ rowp, int j) {
        if (!mapped) return rowp[j];
        const int m = kpn_narrow_col(j, k.n_kpt, k.sp_level);
        return m >= 0 ? rowp[m] : 0.0f;
    };
    float* __restrict__ dst = k.plain + L.w_off + (size_t)r * L.cols;
    if (k.p.g[l]) {                                                    // block-uniform
        double acc = 0.0;
        for (int j = lane; j < L.cols; j += 64) { const double v = (double)ld(src, j); acc += v * v; }
        const double n = sqrt(kpn_row_sum(acc, red));
        const float s = (float)((double)k.p.g[l][r] / n);
        for (int j = lane; j < L.cols; j += 64) dst[j] = KMUL(ld(src, j), s);
        if (lane == 0) { k.norm_n[L.norm0 + r] = n; k.norm_s[L.norm0 + r] = s; }
    } else {
        for (int j = lane; j < L.cols; j += 64) dst[j] = ld(src, j);
    }
    if (lane == 0) k.plain[L.b_off + r] = k.p.b[l][r];
    if (row == 0 && lane == 1) k.plain[k.ani_off] = k.p.ani_al[0];
}

// MAPPED (kpn_fold_params_backward_shape): as above for the loads of v; the gradient of canonical column j goes to the narrow
// column mapped to it, a padded column's is dropped
template <bool MAPPED>
__global__ __launch_bounds__(64) void k_fold_params_backward(kpn_fold_kargs k) {
    __shared__ double red[64];
    const int row = (int)blockIdx.x, lane = (int)threadIdx.x;
    const int l = kpn_fold_layer_of(k, row);
    const kpn_fold_layer L = k.layer[l];
    const int r = row - L.row0;
    const bool acc_mode = k.accumulate != 0;
    const bool mapped = MAPPED && l == 0;                              // block-uniform
    const int pitch = mapped ? kpn_narrow_col(L.cols, k.n_kpt, k.sp_level) : L.cols;
    auto col = [&](int j) { return mapped ? kpn_narrow_col(j, k.n_kpt, k.sp_level) : j; };
    auto put = [acc_mode](float* dst, float val) { *dst = acc_mode ? KADD(*dst, val) : val; };
    const float* __restrict__ dW = k.d_plain + L.w_off + (size_t)r * L.cols;
    float* dvw = k.d.v_or_w[l] ? k.d.v_or_w[l] + (size_t)r * pitch : nullptr;
    if (k.p.g[l]) {                                                    // block-uniform
        const float* __restrict__ v = k.p.v_or_w[l] + (size_t)r * pitch;
        double acc = 0.0;
        for (int j = lane; j < L.cols; j += 64) { const int m = col(j); acc += (double)dW[j] * (double)(m >= 0 ? v[m] : 0.0f); }
        const double dot = kpn_row_sum(acc, red);
        const double n = k.norm_n[L.norm0 + r];
        if (dvw) {
            const float s = k.norm_s[L.norm0 + r];
            const float c = (float)((double)k.p.g[l][r] * dot / (n * n * n));
            for (int j = lane; j < L.cols; j += 64) { const int m = col(j); if (m >= 0) put(dvw + m, KSUB(KMUL(s, dW[j]), KMUL(c, v[m]))); }
        }
        if (k.d.g[l] && lane == 0) put(k.d.g[l] + r, (float)(dot / n));
    } else if (dvw) {
        for (int j = lane; j < L.cols; j += 64) { const int m = col(j); if (m >= 0) put(dvw + m, dW[j]); }
    }
    if (k.d.b[l] && lane == 0) put(k.d.b[l] + r, k.d_plain[L.b_off + r]);
    if (k.d.ani_al && row == 0 && lane == 1) put(k.d.ani_al, k.d_plain[k.ani_off]);
}

// Keypoint sets: narrow plain <-> plain, one thread per element of the vector that is written.  W of layers1.0 is the first block
// of both vectors (rows x 232 canonical, rows x pitch narrow); everything behind it is shifted by rows * (232 - pitch).
__global__ __launch_bounds__(256) void k_widen_plain(const float* __restrict__ narrow, float* __restrict__ plain, int n_plain, int rows,
                                                     int n_kpt, int sp_level) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= n_plain) return;
    const int cols = 7 * KPN_NKPT + 64, pitch = kpn_narrow_col(cols, n_kpt, sp_level);
    if (i < rows * cols) {
        const int r = i / cols, m = kpn_narrow_col(i - r * cols, n_kpt, sp_level);
        plain[i] = m >= 0 ? narrow[r * pitch + m] : 0.0f;
    } else {
        plain[i] = narrow[i - rows * (cols - pitch)];
    }
}
__global__ __launch_bounds__(256) void k_narrow_plain_grad(const float* __restrict__ d_plain, float* __restrict__ d_narrow, int n_narrow,
                                                           int rows, int n_kpt, int sp_level, int accumulate) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= n_narrow) return;
    const int cols = 7 * KPN_NKPT + 64, pitch = kpn_narrow_col(cols, n_kpt, sp_level);
    float g;
    if (i < rows * pitch) {
        const int r = i / pitch;
        g = d_plain[r * cols + kpn_canonical_col(i - r * pitch, n_kpt, sp_level)];
    } else {
        g = d_plain[i + rows * (cols - pitch)];
    }
    d_narrow[i] = accumulate ? KADD(d_narrow[i], g) : g;
}

// torch.optim.Adam's update (amsgrad = False, maximize = False) of one element; step_size = lr / (1 - beta1^t) and
// bc2_sqrt = sqrt(1 - beta2^t) come from the host in double, as torch computes them
__global__ __launch_bounds__(256) void k_adam_step(kpn_adam_kargs k) {
    int s = 0;
    while (s + 1 < k.n_seg && (int)blockIdx.x >= k.block0[s + 1]) ++s;
    const kpn_adam_segment sg = k.seg[s];
    const int64_t i = (int64_t)((int)blockIdx.x - k.block0[s]) * 256 + (int64_t)threadIdx.x;
    if (i >= sg.count) return;
    const double p = (double)sg.param[i];
    const double g = (double)sg.grad[i] + k.wd * p;
    const double m0 = (double)sg.exp_avg[i];
    const double m = m0 + k.one_minus_b1 * (g - m0);
    const double v = k.b2 * (double)sg.exp_avg_sq[i] + k.one_minus_b2 * g * g;
    const double denom = sqrt(v) / k.bc2_sqrt + k.eps;
    sg.exp_avg[i] = (float)m;
    sg.exp_avg_sq[i] = (float)v;
    sg.param[i] = (float)(p - k.step_size * (m / denom));
}

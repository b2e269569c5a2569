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
};
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

__global__ __launch_bounds__(64) void k_fold_params(kpn_fold_kargs k) {
    __shared__ double red[64];
    const int row = (int)blockIdx.x, lane = (int)threadIdx.x;
    const int l = kpn_fold_layer_of(k, row);
    const kpn_fold_layer L = k.layer[l];
    const int r = row - L.row0;
    const float* __restrict__ src = k.p.v_or_w[l] + (size_t)r * L.cols;
    float* __restrict__ dst = k.plain + L.w_off + (size_t)r * L.cols;
    if (k.p.g[l]) {                                                    // block-uniform
        double acc = 0.0;
        for (int j = lane; j < L.cols; j += 64) { const double v = (double)src[j]; acc += v * v; }
        const double n = sqrt(kpn_row_sum(acc, red));
        const float s = (float)((double)k.p.g[l][r] / n);
        for (int j = lane; j < L.cols; j += 64) dst[j] = KMUL(src[j], s);
        if (lane == 0) { k.norm_n[L.norm0 + r] = n; k.norm_s[L.norm0 + r] = s; }
    } else {
        for (int j = lane; j < L.cols; j += 64) dst[j] = src[j];
    }
    if (lane == 0) k.plain[L.b_off + r] = k.p.b[l][r];
    if (row == 0 && lane == 1) k.plain[k.ani_off] = k.p.ani_al[0];
}

__global__ __launch_bounds__(64) void k_fold_params_backward(kpn_fold_kargs k) {
    __shared__ double red[64];
    const int row = (int)blockIdx.x, lane = (int)threadIdx.x;
    const int l = kpn_fold_layer_of(k, row);
    const kpn_fold_layer L = k.layer[l];
    const int r = row - L.row0;
    const bool acc_mode = k.accumulate != 0;
    auto put = [acc_mode](float* dst, float val) { *dst = acc_mode ? KADD(*dst, val) : val; };
    const float* __restrict__ dW = k.d_plain + L.w_off + (size_t)r * L.cols;
    float* dvw = k.d.v_or_w[l] ? k.d.v_or_w[l] + (size_t)r * L.cols : nullptr;
    if (k.p.g[l]) {                                                    // block-uniform
        const float* __restrict__ v = k.p.v_or_w[l] + (size_t)r * L.cols;
        double acc = 0.0;
        for (int j = lane; j < L.cols; j += 64) acc += (double)dW[j] * (double)v[j];
        const double dot = kpn_row_sum(acc, red);
        const double n = k.norm_n[L.norm0 + r];
        if (dvw) {
            const float s = k.norm_s[L.norm0 + r];
            const float c = (float)((double)k.p.g[l][r] * dot / (n * n * n));
            for (int j = lane; j < L.cols; j += 64) put(dvw + j, KSUB(KMUL(s, dW[j]), KMUL(c, v[j])));
        }
        if (k.d.g[l] && lane == 0) put(k.d.g[l] + r, (float)(dot / n));
    } else if (dvw) {
        for (int j = lane; j < L.cols; j += 64) put(dvw + j, dW[j]);
    }
    if (k.d.b[l] && lane == 0) put(k.d.b[l] + r, k.d_plain[L.b_off + r]);
    if (k.d.ani_al && row == 0 && lane == 1) put(k.d.ani_al, k.d_plain[k.ani_off]);
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

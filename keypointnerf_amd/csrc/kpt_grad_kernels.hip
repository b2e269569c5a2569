// kpt_grad_kernels.hip — gradient of the loss with respect to the 3D keypoints (sp_data["kpt3d"]): the reverse of the keypoint
// encoding SpatialEncoder.forward builds for sp_type "rel_z_decay" (reference src/spatial.py:76-118), which the reference gets
// from autograd.  DESIGN.md 4.21 derives the formula; in short, for a (point, view) row with d = R_v (p - k_j) = c - kcam_j,
// dz = d_z, w = exp(-|d|^2 / 2 sigma^2) and the encoding values e_t (= dz w, sin / cos (pi 2^l dz) w):
//     g_t = sum_o W0[o][24 t + j] dA0[o]            (W0 = layers1.0, dA0 = the gradient at its output)
//     S_j = sum_t g_t e_t,   T_j = g_0 w + sum_l pi 2^l (g_{1+2l} e_{2+2l} - g_{2+2l} e_{1+2l})
//     dL/dk_j += R_v^T (S_j d / sigma^2 - T_j e_z)
// k_geo_rows_bwd has already dumped dA0 (D0 [rows][128]) and the finished e_t (X0 [rows][232], column 14 j' + 7 h + t for
// keypoint 12 h + j') for the weight gradient; only d and w are formed again, from the point and the scene table.
//
//   k_kpt_grad_pack   : the transposed encoding operand of layers1.0 from the fp32 forward stream SEG_G1_0A of the packed
//                       weights, in kpn_mfma_layer's stream layout (once per backward call, 96 KB of the workspace);
//   k_kpt_grad        : per 32-row tile of one view, G = dA0 (32 x 128) . W0enc (128 x 168 of 192) on the matrix cores, the chain
//                       above per (row, keypoint), fp64 sums per lane, one fixed-order sum per workgroup;
//   k_kpt_grad_finish : the workgroups' partials in a fixed order, the rotation back to world axes, 1 / sigma^2, += d_kpt3d.
//
// The GEMM runs on v_mfma_f32_32x32x2_f32 (kpn_mfma_layer), not on three bf16 pieces like the backward chains: its weight operand
// is then a plain permutation of a stream the packed buffer already holds (no per-call splitting of 21 k weights into pieces, no
// pieces of dA0 formed per tile), the products are exact fp32 and the kernel is an option whose cost is reported, not part of the
// default step.  K order: K-step s of half h is output feature o = 64 h + s of layers1.0, so a lane's B operands are 64 consecutive
// floats of its D0 row.  Output order: a lane (row p, half h) must hold all seven g_t of a keypoint, so output row
// 32 ob + rowmap(r, h) of the stream is (keypoint 12 h + (16 ob + r) / 8, t = (16 ob + r) % 8); t = 7 is a zero column.
#include "kpn_field_shared.h"

#define KPN_KG_NOB 6
#define KPN_KG_WT_FLOATS (16 * 64 * 4 * KPN_KG_NOB)   // 16 groups of 4 K-steps x 64 lanes x 6 output blocks
#define KPN_KG_Q (KPN_NKPT * 4)                       // per (workgroup, view): per keypoint sum S d (3, camera axes) and sum T

__global__ __launch_bounds__(256) void k_kpt_grad_pack(const float* __restrict__ wp, float* __restrict__ wt) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= KPN_KG_WT_FLOATS) return;
    const int g = e / (64 * 4 * KPN_KG_NOB), lane = (e / (4 * KPN_KG_NOB)) % 64, rem = e % (4 * KPN_KG_NOB);
    const int i = rem / KPN_KG_NOB, ob = rem % KPN_KG_NOB;
    const int o = 64 * (lane >> 5) + 4 * g + i;                       // K: output feature of layers1.0
    const int row = lane & 31, hh = (row >> 2) & 1, r = (row & 3) + 4 * (row >> 3);   // row = KPN_ROWMAP(r, hh)
    const int n = 16 * ob + r, jj = n >> 3, t = n & 7;
    // SEG_G1_0A (api_weights.hip): group jj = keypoints jj (h = 0) and jj + 12 (h = 1), K-step t, [64 lanes][7 x 4 output blocks]
    wt[e] = t < 7 ? wp[kpn_seg_woff(SEG_G1_0A) + ((size_t)jj * 64 + 32 * hh + (o & 31)) * 28 + t * 4 + (o >> 5)] : 0.0f;
}

struct kpn_kpt_grad_args {
    const float* D0;   // dA0 [rows][128]
    const float* X0;   // [rows][KPN_LDX0]
    const float* wt;   // k_kpt_grad_pack's stream
    double* partial;   // [gridDim.x][V][KPN_KG_Q], added to
    int n_kpt;         // keypoints of the model: table rows beyond repeat keypoint 0 and take no part
    uint32_t keep;     // bit v = 0: the rows of view v were never dumped (run_backward's wgrad_keep)
};

// grid (workers, V): a workgroup owns one view and every (4 x workers)-th tile of it per wave — a fixed assignment, so the sums are
// reproducible for a given valid list.  Rows of a dropped view and rows beyond the valid count are never read.
__global__ __launch_bounds__(256) void k_kpt_grad(kpn_scene_dev sc, kpn_points ps, const int* __restrict__ list,
                                                  const int* __restrict__ count_ptr, kpn_kpt_grad_args a) {
    const int v = blockIdx.y;
    if (!((a.keep >> v) & 1u)) return;   // (block-uniform; its partials stay zero)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int p = lane & 31, h = lane >> 5;
    const int count = *count_ptr;
    const int ntiles = (count + KPN_TILE - 1) / KPN_TILE;
    const float* tb = sc.table + (size_t)v * KPN_TBL_STRIDE;
    const float* E = tb + KPN_TBL_EXT;
    const float* kc = tb + KPN_TBL_KCAM + (12 * h) * 3;
    const float inv2s2 = 1.0f / sc.two_sigma2;
    const float pi = 3.14159265358979323846f;
    double acc[12][4];
#pragma unroll
    for (int j = 0; j < 12; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[j][q] = 0.0;

    for (int t = blockIdx.x * 4 + wave; t < ntiles; t += (int)gridDim.x * 4) {
        const int ci = t * KPN_TILE + p;
        const bool live = ci < count;
        const size_t row = ((size_t)t * sc.V + v) * KPN_TILE + p;
        float4 dy[16];
#pragma unroll
        for (int g = 0; g < 16; ++g) dy[g] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (live) {
            const float4* src = reinterpret_cast<const float4*>(a.D0 + row * 128 + 64 * h);
#pragma unroll
            for (int g = 0; g < 16; ++g) dy[g] = src[g];
        }
        kpn_f32x16 G[KPN_KG_NOB];
#pragma unroll
        for (int ob = 0; ob < KPN_KG_NOB; ++ob)
#pragma unroll
            for (int r = 0; r < 16; ++r) G[ob][r] = 0.0f;
        kpn_mfma_layer<64, KPN_KG_NOB, 4>(a.wt, lane, [&](auto gi, float (&x)[4]) {
            constexpr int g = decltype(gi)::value;
            x[0] = dy[g].x; x[1] = dy[g].y; x[2] = dy[g].z; x[3] = dy[g].w;
        }, G);
        if (!live) continue;
        float P[3], D[3];
        kpn_get_point(ps, (int64_t)list[ci], P, D);
        // the camera-frame point as k_geo_rows forms it
        const float cx = RADD(kpn_dot3(P[0], P[1], P[2], E[0], E[1], E[2]), E[3]);
        const float cy = RADD(kpn_dot3(P[0], P[1], P[2], E[4], E[5], E[6]), E[7]);
        const float cz = RADD(kpn_dot3(P[0], P[1], P[2], E[8], E[9], E[10]), E[11]);
        const float* xr = a.X0 + row * KPN_LDX0 + 7 * h;
        kpn_static_for<0, 12>([&](auto ji) {
            constexpr int jj = decltype(ji)::value;
            if (12 * h + jj >= a.n_kpt) return;
            const float dx = RSUB(cx, kc[jj * 3 + 0]), dy_ = RSUB(cy, kc[jj * 3 + 1]), dz = RSUB(cz, kc[jj * 3 + 2]);
            const float d2 = RADD(RADD(RMUL(dx, dx), RMUL(dy_, dy_)), RMUL(dz, dz));
            const float w = kpn_fast_exp(-d2 / sc.two_sigma2);
            float g[7], e[7];
#pragma unroll
            for (int i = 0; i < 7; ++i) { g[i] = G[jj >> 1][8 * (jj & 1) + i]; e[i] = xr[14 * jj + i]; }
            float S = g[0] * e[0];
#pragma unroll
            for (int i = 1; i < 7; ++i) S = fmaf(g[i], e[i], S);
            float T = g[0] * w;
            T = fmaf(pi, g[1] * e[2] - g[2] * e[1], T);
            T = fmaf(2.0f * pi, g[3] * e[4] - g[4] * e[3], T);
            T = fmaf(4.0f * pi, g[5] * e[6] - g[6] * e[5], T);
            // S (p - k_j) per row in fp32 (camera axes: d = R (p - k_j)), summed in fp64; 1 / (2 sigma^2) here, the 2 at the end
            const float Ss = S * inv2s2;
            acc[jj][0] += (double)(Ss * dx); acc[jj][1] += (double)(Ss * dy_); acc[jj][2] += (double)(Ss * dz);
            acc[jj][3] += (double)T;
        });
    }

    // the workgroup's sums: wave after wave through one LDS tile, the 32 rows of a half added in row order
    __shared__ double red_s[64][49];
    double tot = 0.0;
    const int q = threadIdx.x, qh = q / 48, qj = (q % 48) >> 2, qc = q & 3;
    for (int wv = 0; wv < 4; ++wv) {
        if (wave == wv) {
#pragma unroll
            for (int j = 0; j < 12; ++j)
#pragma unroll
                for (int c = 0; c < 4; ++c) red_s[lane][4 * j + c] = acc[j][c];
        }
        __syncthreads();
        if (q < KPN_KG_Q)
            for (int r = 0; r < 32; ++r) tot += red_s[32 * qh + r][4 * qj + qc];
        __syncthreads();
    }
    if (q < KPN_KG_Q) a.partial[((size_t)blockIdx.x * sc.V + v) * KPN_KG_Q + (12 * qh + qj) * 4 + qc] += tot;
}

// grid (n_kpt): the workers' partials of a keypoint in a fixed order per (view, quantity), then
// d_kpt[j] += sum_v R_v^T (2 A_v - T_v e_z),  A_v = sum S d / (2 sigma^2) (k_kpt_grad).  A zero sum leaves the bits of d_kpt alone.
__global__ __launch_bounds__(256) void k_kpt_grad_finish(kpn_scene_dev sc, const double* __restrict__ partial, int nworkers,
                                                         float* __restrict__ d_kpt) {
    const int kp = blockIdx.x;
    const int part = threadIdx.x >> 6, vq = threadIdx.x & 63, v = vq >> 2, q = vq & 3;
    __shared__ double red[4][64];
    __shared__ double tot[64];
    double s = 0.0;
    if (v < sc.V)
        for (int w = part; w < nworkers; w += 4) s += partial[((size_t)w * sc.V + v) * KPN_KG_Q + kp * 4 + q];
    red[part][vq] = s;
    __syncthreads();
    if (threadIdx.x < 64) tot[threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
    __syncthreads();
    if (threadIdx.x >= 3) return;
    const int c = threadIdx.x;
    double g = 0.0;
    for (int vv = 0; vv < sc.V; ++vv) {
        const float* E = sc.table + (size_t)vv * KPN_TBL_STRIDE + KPN_TBL_EXT;
        const double ax = 2.0 * tot[4 * vv + 0], ay = 2.0 * tot[4 * vv + 1], az = 2.0 * tot[4 * vv + 2] - tot[4 * vv + 3];
        g += (double)E[c] * ax + (double)E[4 + c] * ay + (double)E[8 + c] * az;
    }
    if (g != 0.0) d_kpt[kp * 3 + c] += (float)g;
}

// kpn_reduce.h — the one deterministic fp64 reduction of the loss and metric kernels (k_mse_psnr, k_pix_l1, k_ssim_map,
// k_train_loss, k_vgg_l1).  Every thread brings fp64 sums of its grid-stride loop; a 256-wide LDS tree adds the threads of a
// block; thread 0 stores the block's partials, fences and takes a ticket; the block that draws the last ticket re-reads all
// partials and adds them in slot order.  The result depends on the grid alone, never on which block finishes last.
// tests/reduce_order_cases.py restates the order of every add; the host side of the pattern is reduce_blocks / reduce_scratch (api_common.h).
#pragma once

// Adds acc[q] over the block's 256 threads (tree s = 128 .. 1, red[q][t] += red[q][t + s]), stores the sums to
// partial[slot * NQ + q] and takes a ticket.  Returns true to the threads with `reads` set of the block that drew the last of the
// nslots tickets (block-uniform where `reads` is): those threads have passed the second fence, so every slot's partials are visible
// to their volatile reads.  ALL 256 threads of the block must call it (it holds barriers): no kernel that uses it returns early.
// red is the caller's, so that it can be used again afterwards.
template <int NQ>
__device__ __forceinline__ bool kpn_block_sums_last(const double (&acc)[NQ], double (&red)[NQ][256], double* __restrict__ partial,
                                                    int* __restrict__ ticket, unsigned slot, unsigned nslots, bool reads) {
    __shared__ int last;
#pragma unroll
    for (int q = 0; q < NQ; ++q) red[q][threadIdx.x] = acc[q];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) red[q][threadIdx.x] += red[q][threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) partial[(size_t)slot * NQ + q] = red[q][0];
        __threadfence();                                     // the partials before the ticket
        last = (atomicAdd(ticket, 1) == (int)nslots - 1);
    }
    __syncthreads();
    if (!(last && reads)) return false;
    __threadfence();                                         // the last ticket before the other blocks' partials
    return true;
}
// sum q of all slots, added to 0.0 in slot order (for the threads kpn_block_sums_last returned true to)
__device__ __forceinline__ double kpn_partials_in_order(const double* partial, unsigned nslots, int NQ, int q) {
    double tot = 0.0;
    for (unsigned b = 0; b < nslots; ++b) tot += ((volatile const double*)partial)[(size_t)b * NQ + q];
    return tot;
}

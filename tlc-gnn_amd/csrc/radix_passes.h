// radix_passes.h -- the device-wide LSD radix sort (8-bit digits; a pass = histogram, per-digit scan, stable scatter) of every
// "whole device, one item after the other" class: lp_metrics.hip (u32 / u64 keys with a u8 label), pd_wide.hip and pd_grad.hip (u64 / u32
// keys with a u32 id) and sliced_w.hip (u64 keys with a u64 payload).  Positions are ints: fewer than 2^31 items.
// A pass over n items in nb = rk_tiles(n) tiles:
//     rk_hist_kernel<K>      <<<nb, RK_BS>>>   hist[d * nb + b] = items of tile b with digit d
//     rk_scan_rows_kernel    <<<256, RK_BS>>>  each digit's row -> its exclusive prefix; tot[d] = the row's sum
//     rk_scatter_kernel<K,L> <<<nb, RK_BS>>>   stable scatter of keys and payloads
// hist holds rk_hist_ints(n) ints, tot RK_TOT_INTS: the layout functions size them with the names rk_pass launches by.  The only
// atomics are LDS integer counts, so the result does not depend on the scheduling.  Host side: rk_pass (one pass), rk_sort<BITS> (BITS / 8 of them).
#pragma once
#include "tlc_common.h"

namespace {

#define RK_BS 256                      // threads per workgroup
#define RK_IPT 16                      // items per thread
#define RK_TILE (RK_BS * RK_IPT)       // items per tile

// ---- block-level exclusive sum in a fixed order ---------------------------------------------------------------------------
template <int BS>
struct BlockScratch {
    long long w[BS / 64];
    double h[BS / 64], l[BS / 64];
};

// exclusive prefix sum over the block (thread order); *total = the block's sum
template <int BS>
__device__ long long block_excl_sum(long long v, BlockScratch<BS>& sh, long long* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long o = __shfl_up(inc, d);
        if (lane >= d) inc += o;
    }
    __syncthreads();
    if (lane == 63) sh.w[wave] = inc;
    __syncthreads();
    long long before = 0, tot = 0;
    for (int w = 0; w < BS / 64; ++w) {
        if (w < wave) before += sh.w[w];
        tot += sh.w[w];
    }
    *total = tot;
    return before + inc - v;
}

// hist[d * nb + b] = items of tile b with digit d (LDS integer counts: the total does not depend on the order)
template <typename K>
__global__ __launch_bounds__(RK_BS) void rk_hist_kernel(const K* __restrict__ keys, long long n, int shift, int* __restrict__ hist) {
    __shared__ int h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const long long t0 = (long long)blockIdx.x * RK_TILE;
    for (int j = threadIdx.x; j < RK_TILE; j += RK_BS) {
        const long long i = t0 + j;
        if (i < n) atomicAdd(&h[(int)(keys[i] >> shift) & 255], 1);
    }
    __syncthreads();
    hist[(long long)threadIdx.x * gridDim.x + blockIdx.x] = h[threadIdx.x];
}

// row d of hist (nb tiles) -> its exclusive prefix in place; tot[d] = the row's sum.  One workgroup per digit.
__global__ __launch_bounds__(RK_BS) void rk_scan_rows_kernel(int* __restrict__ hist, int nb, int* __restrict__ tot) {
    __shared__ BlockScratch<RK_BS> sh;
    int* row = hist + (long long)blockIdx.x * nb;
    long long carry = 0;
    for (int b0 = 0; b0 < nb; b0 += RK_BS) {
        const int b = b0 + threadIdx.x;
        const long long v = b < nb ? row[b] : 0;
        long long t;
        const long long ex = block_excl_sum<RK_BS>(v, sh, &t);
        if (b < nb) row[b] = (int)(carry + ex);
        carry += t;
    }
    if (threadIdx.x == 0) tot[blockIdx.x] = (int)carry;
}

// stable scatter of tile b: rounds of RK_BS consecutive items; inside a round, ranks within the wavefront from 8 ballots
template <typename K, typename L>
__global__ __launch_bounds__(RK_BS) void rk_scatter_kernel(const K* __restrict__ kin, const L* __restrict__ lin, K* __restrict__ kout,
                                                           L* __restrict__ lout, long long n, int shift,
                                                           const int* __restrict__ hist, const int* __restrict__ tot) {
    __shared__ int off[256];
    __shared__ int wc[RK_BS / 64][256];
    __shared__ BlockScratch<RK_BS> sh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long long t;
    const long long dbase = block_excl_sum<RK_BS>(tot[tid], sh, &t);
    off[tid] = (int)dbase + hist[(long long)tid * gridDim.x + blockIdx.x];
    const long long t0 = (long long)blockIdx.x * RK_TILE;
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int r = 0; r < RK_IPT; ++r) {
        const long long i = t0 + (long long)r * RK_BS + tid;
        const bool valid = i < n;
        K k = 0;
        L l = 0;
        int d = 0;
        if (valid) {
            k = kin[i];
            l = lin[i];
            d = (int)(k >> shift) & 255;
        }
#pragma unroll
        for (int w = 0; w < RK_BS / 64; ++w) wc[w][tid] = 0;
        __syncthreads();
        unsigned long long m = __ballot(valid);
#pragma unroll
        for (int bt = 0; bt < 8; ++bt) {
            const unsigned long long bb = __ballot((d >> bt) & 1);
            m &= ((d >> bt) & 1) ? bb : ~bb;
        }
        const int rank = __popcll(m & lt);
        if (valid && rank == 0) wc[wave][d] = __popcll(m);
        __syncthreads();
        int run = off[tid];
#pragma unroll
        for (int w = 0; w < RK_BS / 64; ++w) {
            const int c = wc[w][tid];
            wc[w][tid] = run;
            run += c;
        }
        off[tid] = run;
        __syncthreads();
        if (valid) {
            const int dst = wc[wave][d] + rank;
            kout[dst] = k;
            lout[dst] = l;
        }
        __syncthreads();
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------
#define RK_TOT_INTS 256                                                       // ints of tot
inline long long rk_tiles(long long n) { return (n + RK_TILE - 1) / RK_TILE; }
inline long long rk_hist_ints(long long n) { return 256 * rk_tiles(n); }      // ints of hist for passes over n items

// one pass on the digit at `shift`: (kin, lin) -> (kout, lout), three kernels
template <typename K, typename L>
void rk_pass(hipStream_t st, long long n, int shift, const K* kin, const L* lin, K* kout, L* lout, int* hist, int* tot) {
    const unsigned nb = (unsigned)rk_tiles(n);
    hipLaunchKernelGGL(rk_hist_kernel<K>, dim3(nb), dim3(RK_BS), 0, st, kin, n, shift, hist);
    hipLaunchKernelGGL(rk_scan_rows_kernel, dim3(256), dim3(RK_BS), 0, st, hist, (int)nb, tot);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(rk_scatter_kernel<K, L>), dim3(nb), dim3(RK_BS), 0, st, kin, lin, kout, lout, n, shift, hist, tot);
}
// the low BITS of the keys, ascending and stable: BITS / 8 passes that ping-pong between (ka, la) and (kb, lb) -- an even number, so
// the result is back in ka / la, as it is for n < 2, where nothing is launched.  Returns the kernels launched.
template <int BITS, typename K, typename L>
int rk_sort(hipStream_t st, long long n, K* ka, K* kb, L* la, L* lb, int* hist, int* tot) {
    static_assert(BITS % 16 == 0 && BITS <= 8 * (int)sizeof(K), "an even number of passes over digits the key has");
    if (n < 2) return 0;
    for (int shift = 0; shift < BITS; shift += 16) {
        rk_pass(st, n, shift, ka, la, kb, lb, hist, tot);
        rk_pass(st, n, shift + 8, kb, lb, ka, la, hist, tot);
    }
    return 3 * (BITS / 8);
}

}  // namespace

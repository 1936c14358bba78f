// radix_passes.h -- one pass of the device-wide LSD radix sort (8-bit digits: histogram, per-digit scan, stable scatter), shared by
// lp_metrics.hip (u32 / u64 keys with a u8 label) and pd_wide.hip (u64 keys with a u32 id).  Positions are ints: fewer than 2^31 items.
// A pass over n items in nb = ceil(n / RK_TILE) tiles:
//     rk_hist_kernel<K>      <<<nb, RK_BS>>>   hist[d * nb + b] = items of tile b with digit d
//     rk_scan_rows_kernel    <<<256, RK_BS>>>  each digit's row -> its exclusive prefix; tot[d] = the row's sum
//     rk_scatter_kernel<K,L> <<<nb, RK_BS>>>   stable scatter of keys and payloads
// hist holds 256 * nb ints, tot 256.  The only atomics are LDS integer counts, so the result does not depend on the scheduling.
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

}  // namespace

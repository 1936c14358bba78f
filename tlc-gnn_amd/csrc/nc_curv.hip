// nc_curv.hip -- curvGN of the reference's node classifier (Knowledge_Distillation/ConvCurv_GIN.py:149-185), forward and backward.
//
//   out[t] = sum_{e : dst_e = t} alpha[e] (.) xl[src_e],   xl = x W^T + b,
//   alpha  = softmax over the edges of one SOURCE, per channel, of wt = W2 PReLU_a(W1 w_mul[e]) + b2
//
//   tlc_nc_group          stable counting sort of the edge ids by source and by target (built once per graph)
//   tlc_nc_linear_f32     y = x W^T + b on the f32 MFMA (the node projection; any N, any K)
//   tlc_nc_linear_bwd_f32 dW (tlc_gemm_tn_f32), db (its column sums), dx = dy W (f32 MFMA)
//   tlc_nc_curv_fwd_f32   the edge MLP fused with the source-grouped softmax (z and h stay on chip), then the per-target gather
//   tlc_nc_curv_bwd_f32   per source row: d xl and d wt; per edge tile: the MLP backward (z recomputed); weight gradients as
//                         fixed-order split-K sums (tlc_gemm_tn_f32)
//
// No floating-point atomics anywhere: every sum runs in an order fixed by the graph and the shapes, so the same inputs give the same
// bits on every call.  Edges are kept exactly as given (duplicates and self loops stay); E * C is indexed in 64 bits.
#include "tlc_common.h"
#include "scratch_layouts.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---- grouping ------------------------------------------------------------------------------------------------------------------
// edge e's place in its source row / target row is what its counting atomic returned; the rows are then rank-sorted by edge id,
// so the final order (ascending edge id inside a row: a stable sort) does not depend on the atomics' order.
__global__ void nc_count_kernel(long long E, const long long* __restrict__ ei, int n, int* __restrict__ cnt_s, int* __restrict__ cnt_t,
                                int* __restrict__ place_s, int* __restrict__ place_t, int* __restrict__ e_src, int* __restrict__ e_dst,
                                int* __restrict__ bad) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const long long s = ei[e], t = ei[E + e];
    if (s < 0 || t < 0 || s >= n || t >= n) {
        atomicAdd(bad, 1);
        e_src[e] = 0;
        e_dst[e] = 0;
        place_s[e] = place_t[e] = -1;
        return;
    }
    e_src[e] = (int)s;
    e_dst[e] = (int)t;
    place_s[e] = atomicAdd(&cnt_s[s], 1);
    place_t[e] = atomicAdd(&cnt_t[t], 1);
}

// ptr[i + 1] = sum_{j <= i} cnt[j]: one workgroup per array (blockIdx.x 0: sources, 1: targets), chunks of 1024 with a carry
__global__ __launch_bounds__(1024) void nc_scan_kernel(int n, const int* __restrict__ cnt_s, const int* __restrict__ cnt_t,
                                                       int* __restrict__ ptr_s, int* __restrict__ ptr_t) {
    __shared__ int s[1024];
    __shared__ int carry;
    const int* cnt = blockIdx.x == 0 ? cnt_s : cnt_t;
    int* ptr = blockIdx.x == 0 ? ptr_s : ptr_t;
    const int t = threadIdx.x;
    if (t == 0) { carry = 0; ptr[0] = 0; }
    __syncthreads();
    for (int base = 0; base < n; base += 1024) {
        const int i = base + t;
        s[t] = i < n ? cnt[i] : 0;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {
            const int a = t >= o ? s[t - o] : 0;
            __syncthreads();
            s[t] += a;
            __syncthreads();
        }
        if (i < n) ptr[i + 1] = carry + s[t];
        __syncthreads();
        if (t == 1023) carry += s[t];
        __syncthreads();
    }
}

__global__ void nc_fill_kernel(long long E, const int* __restrict__ e_src, const int* __restrict__ e_dst, const int* __restrict__ place_s,
                               const int* __restrict__ place_t, const int* __restrict__ ptr_s, const int* __restrict__ ptr_t,
                               int* __restrict__ raw_s, int* __restrict__ raw_t) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E || place_s[e] < 0) return;
    raw_s[ptr_s[e_src[e]] + place_s[e]] = (int)e;
    raw_t[ptr_t[e_dst[e]] + place_t[e]] = (int)e;
}

// position p of a row holds edge raw[p]; its final place is the row start + the number of the row's edges with a smaller id
// (blockIdx.y 0: by source, 1: by target).  A row of d edges costs d steps in each of its d threads: d^2 in all, spread over d
// threads.  That is cheap for the graphs in scope (the largest degree of the Planetoid / Amazon / Coauthor graphs is a few thousand:
// a few million steps, once per graph), but a node of degree 10^5 would cost 10^10 steps; such graphs need a segmented sort here.
__global__ void nc_rank_kernel(int n, const int* __restrict__ e_src, const int* __restrict__ e_dst, const int* __restrict__ ptr_s,
                               const int* __restrict__ ptr_t, const int* __restrict__ raw_s, const int* __restrict__ raw_t,
                               int* __restrict__ eid_s, int* __restrict__ eid_t) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool by_src = blockIdx.y == 0;
    const int* raw = by_src ? raw_s : raw_t;
    const int* ptr = by_src ? ptr_s : ptr_t;
    if (p >= ptr[n]) return;                                  // (invalid edges leave the tail unplaced)
    const int e = raw[p];
    const int r = by_src ? e_src[e] : e_dst[e];
    const int b = ptr[r], end = ptr[r + 1];
    int rank = 0;
    for (int q = b; q < end; ++q) rank += raw[q] < e;
    (by_src ? eid_s : eid_t)[b + rank] = e;
}

// ---- node projection: C[M,N] = A[M,K] op(B) (+ bias) ---------------------------------------------------------------------------
// TB: B is [N,K] (a Linear weight: y = x W^T); else B is [K,N] (dx = dy W).  Workgroup = 4 wavefronts on a 64 x 64 tile of C, each
// wavefront a 32 x 32 quarter as 2 x 2 blocks of v_mfma_f32_16x16x4_f32.  Operands straight from global memory (the tile's rows
// stay in L1/L2 over the K loop); k is permuted inside each 16-block (lane group g takes k = 4 g + u at step u: a sum over k does
// not care), so that a lane reads four consecutive floats of an A row.  Out-of-range rows / columns / k read as zeros.
template <bool TB>
__global__ __launch_bounds__(256) void nc_gemm_kernel(int M, int N, int K, const float* __restrict__ A, const float* __restrict__ B,
                                                      const float* __restrict__ bias, float* __restrict__ Cm) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, l16 = lane & 15, g = lane >> 4;
    const int m0 = blockIdx.x * 64 + 32 * (w & 1), n0 = blockIdx.y * 64 + 32 * (w >> 1);
    int ma[2], nb[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        ma[i] = m0 + 16 * i + l16;
        nb[i] = n0 + 16 * i + l16;
    }
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int k0 = 0; k0 < K; k0 += 16) {
        float a[2][4], b[2][4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = k0 + 4 * g + u;
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i][u] = (ma[i] < M && k < K) ? A[(size_t)ma[i] * K + k] : 0.0f;
#pragma unroll
            for (int j = 0; j < 2; ++j)
                b[j][u] = (nb[j] < N && k < K) ? (TB ? B[(size_t)nb[j] * K + k] : B[(size_t)k * N + nb[j]]) : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][u], b[j][u], acc[i][j], 0, 0, 0);
    }
    // C/D layout: column l16, row 4 g + r
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = nb[j];
        const float bv = (bias && n < N) ? bias[n] : 0.0f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + 16 * i + 4 * g + r;
                if (m < M && n < N) Cm[(size_t)m * N + n] = acc[i][j][r] + bv;
            }
    }
}

// ---- edge MLP tiles ------------------------------------------------------------------------------------------------------------
// A tile is NC_T edges x C channels.  Wavefront w owns the 16-column blocks w, w + 4, w + 8, w + 12 of C (all 64 rows: 4 x 4
// accumulator blocks); the A operand (the tile's rows) comes from LDS, shared by the four wavefronts, the B operand (W1 / W2, read by
// exactly one wavefront each) from L2.  The LDS buffer holds [64][NC_HS] floats: first the w_mul rows at stride NC_MS, then h, then
// wt (forward) / ds (backward).
#define NC_T 64
#define NC_HS 260
#define NC_MS 68
#define NC_MAX_C 256
#define NC_MAX_D 64
#define NC_LDS_BYTES (NC_T * NC_HS * 4)

// z = m W1^T for the tile's rows m (in LDS, stride NC_MS, D zero-padded to a multiple of 16): acc[rb][j] = rows 16 rb.., columns
// 16 (w + 4 j)..
__device__ __forceinline__ void nc_layer1(f32x4 (&acc)[4][4], const float* s_m, const float* __restrict__ W1, int C, int D, int w,
                                          int l16, int g) {
    const int nb = (C + 15) >> 4, kb = (D + 15) >> 4;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int kk = 0; kk < kb; ++kk) {
        const int k0 = 16 * kk;
        f32x4 av[4];
        float bv[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i) av[i] = *reinterpret_cast<const f32x4*>(s_m + (16 * i + l16) * NC_MS + k0 + 4 * g);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = 16 * (w + 4 * j) + l16;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int k = k0 + 4 * g + u;
                bv[j][u] = (c < C && k < D) ? W1[(size_t)c * D + k] : 0.0f;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (w + 4 * j < nb)
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i][u], bv[j][u], acc[i][j], 0, 0, 0);
    }
}

// acc = s_a W for the tile's rows s_a (in LDS, stride NC_HS, C zero-padded to a multiple of 16) and a C x C matrix W:
// TW: out[e][o] = sum_c s_a[e][c] W[o][c] (wt = h W2^T); else out[e][c] = sum_o s_a[e][o] W[o][c] (dh = ds W2).
// The B operand comes from L2, not LDS: each element of W is read by exactly one wavefront per chunk, so staging it would add a copy
// without reuse (and W2 is 256 KB at C = 256, more than the 160 KiB of LDS).  TW: lane (l16, g) needs W[o][k0 + 4 g .. + 3], four
// consecutive floats of one row -- with VEC (C % 4 == 0, W 16-byte aligned) one 16-byte load instead of four 4-byte ones.  Not TW:
// the 16 lanes of a group read 16 consecutive floats of one row (coalesced as they are).
template <bool TW, bool VEC>
__device__ __forceinline__ void nc_layer2(f32x4 (&acc)[4][4], const float* s_a, const float* __restrict__ W, int C, int w, int l16, int g) {
    const int nb = (C + 15) >> 4;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int kk = 0; kk < nb; ++kk) {
        const int k0 = 16 * kk;
        f32x4 av[4];
        float bv[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i) av[i] = *reinterpret_cast<const f32x4*>(s_a + (16 * i + l16) * NC_HS + k0 + 4 * g);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = 16 * (w + 4 * j) + l16;
            if (TW && VEC) {
                const f32x4 v = (n < C && k0 + 4 * g < C) ? *reinterpret_cast<const f32x4*>(W + (size_t)n * C + k0 + 4 * g)
                                                          : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int u = 0; u < 4; ++u) bv[j][u] = v[u];
            } else {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int k = k0 + 4 * g + u;
                    bv[j][u] = (n < C && k < C) ? (TW ? W[(size_t)n * C + k] : W[(size_t)k * C + n]) : 0.0f;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (w + 4 * j < nb)
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i][u], bv[j][u], acc[i][j], 0, 0, 0);
    }
}

// the tile's w_mul rows into LDS (stride NC_MS; rows past cnt and columns past D as zeros); row i = edge eid(i)
template <typename EidF>
__device__ __forceinline__ void nc_stage_m(float* s_m, const float* __restrict__ wmul, int D, int cnt, EidF eid) {
    const int d16 = (D + 15) & ~15;
    for (int idx = threadIdx.x; idx < NC_T * d16; idx += blockDim.x) {
        const int i = idx / d16, k = idx - i * d16;
        s_m[i * NC_MS + k] = (i < cnt && k < D) ? wmul[(size_t)eid(i) * D + k] : 0.0f;
    }
}

// first index r in [0, n] with ptr[r] >= v (ptr non-decreasing)
__device__ __forceinline__ int nc_lower_bound(const int* __restrict__ ptr, int n, long long v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((long long)ptr[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// ---- forward: edge MLP + source-grouped softmax -> alpha[E][C] (edge order) ------------------------------------------------------
// Tile j = the source rows that START in positions [64 j, 64 j + 64) of the by-source order: whole rows, so a row's softmax ends
// inside its tile.  The tile's positions [a, b) run through the MLP in chunks of 64.  Thread c then takes channel c of the chunk's
// wt: a row that lies inside the chunk is normalised from LDS (max, sum of exp(wt - max), exp(wt - max) / (sum + 1e-16): PyG's
// softmax); a row that spans chunks (a hub) has its raw wt written to alpha first and is normalised from there once its last chunk
// is out (the same thread wrote every value it reads back).
template <bool VEC>
__global__ __launch_bounds__(256, 2) void nc_edge_fwd_kernel(int n, int C, int D, const int* __restrict__ src_ptr, const int* __restrict__ src_eid,
                                                             const int* __restrict__ e_src, const float* __restrict__ wmul,
                                                             const float* __restrict__ W1, const float* __restrict__ prelu,
                                                             const float* __restrict__ W2, const float* __restrict__ b2,
                                                             float* __restrict__ alpha) {
    extern __shared__ float s_buf[];
    __shared__ int s_eid[NC_T], s_row[NC_T];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l16 = lane & 15, g = lane >> 4;
    const int nb = (C + 15) >> 4;
    const long long a = src_ptr[nc_lower_bound(src_ptr, n, (long long)blockIdx.x * NC_T)];
    const long long b = src_ptr[nc_lower_bound(src_ptr, n, (long long)(blockIdx.x + 1) * NC_T)];
    for (long long p0 = a; p0 < b; p0 += NC_T) {
        const int cnt = (int)(b - p0 < NC_T ? b - p0 : NC_T);
        if (tid < NC_T) {
            const int e = tid < cnt ? src_eid[p0 + tid] : 0;
            s_eid[tid] = e;
            s_row[tid] = tid < cnt ? e_src[e] : -1;
        }
        __syncthreads();
        nc_stage_m(s_buf, wmul, D, cnt, [&](int i) { return s_eid[i]; });
        __syncthreads();
        f32x4 acc[4][4];
        nc_layer1(acc, s_buf, W1, C, D, w, l16, g);
        __syncthreads();                                      // every wavefront is done with the w_mul rows: h overwrites them
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (w + 4 * j >= nb) continue;
            const int c = 16 * (w + 4 * j) + l16;
            const float sl = c < C ? prelu[c] : 0.0f;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float z = acc[i][j][r];
                    s_buf[(16 * i + 4 * g + r) * NC_HS + c] = z > 0.0f ? z : sl * z;        // torch.prelu: x > 0 ? x : a x
                }
        }
        __syncthreads();
        nc_layer2<true, VEC>(acc, s_buf, W2, C, w, l16, g);
        __syncthreads();                                      // h read by all: wt overwrites it
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (w + 4 * j >= nb) continue;
            const int o = 16 * (w + 4 * j) + l16;
            const float bo = o < C ? b2[o] : 0.0f;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) s_buf[(16 * i + 4 * g + r) * NC_HS + o] = acc[i][j][r] + bo;
        }
        __syncthreads();
        if (tid < C) {
            const int c = tid;
            int i = 0;
            while (i < cnt) {
                const int r = s_row[i];
                const long long rs = src_ptr[r], re = src_ptr[r + 1];
                const int i_end = (int)(re - p0 < cnt ? re - p0 : cnt);
                if (rs >= p0 && re <= p0 + cnt) {
                    float mx = -INFINITY;
                    for (int q = i; q < i_end; ++q) mx = fmaxf(mx, s_buf[q * NC_HS + c]);
                    float sum = 0.0f;
                    for (int q = i; q < i_end; ++q) sum += expf(s_buf[q * NC_HS + c] - mx);
                    const float den = sum + 1e-16f;
                    for (int q = i; q < i_end; ++q) alpha[(size_t)s_eid[q] * C + c] = expf(s_buf[q * NC_HS + c] - mx) / den;
                } else {
                    for (int q = i; q < i_end; ++q) alpha[(size_t)s_eid[q] * C + c] = s_buf[q * NC_HS + c];
                    if (re <= p0 + cnt) {
                        float mx = -INFINITY;
                        for (long long q = rs; q < re; ++q) mx = fmaxf(mx, alpha[(size_t)src_eid[q] * C + c]);
                        float sum = 0.0f;
                        for (long long q = rs; q < re; ++q) sum += expf(alpha[(size_t)src_eid[q] * C + c] - mx);
                        const float den = sum + 1e-16f;
                        for (long long q = rs; q < re; ++q) {
                            float* pa = alpha + (size_t)src_eid[q] * C + c;
                            *pa = expf(*pa - mx) / den;
                        }
                    }
                }
                i = i_end;
            }
        }
        __syncthreads();                                      // the softmax is done with s_eid / s_row / s_buf before the next chunk
    }
}

// out[t][c] = sum over t's in-edges (ascending edge id) of alpha[e][c] xl[src_e][c]; a node without in-edges gets a zero row
__global__ __launch_bounds__(256) void nc_aggr_kernel(int n, int C, const int* __restrict__ tgt_ptr, const int* __restrict__ tgt_eid,
                                                      const int* __restrict__ e_src, const float* __restrict__ alpha,
                                                      const float* __restrict__ xl, float* __restrict__ out) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long long)n * C) return;
    const int t = (int)(gid / C), c = (int)(gid - (long long)t * C);
    float acc = 0.0f;
    for (int j = tgt_ptr[t], je = tgt_ptr[t + 1]; j < je; ++j) {
        const int e = tgt_eid[j];
        acc += alpha[(size_t)e * C + c] * xl[(size_t)e_src[e] * C + c];
    }
    out[gid] = acc;
}

// ---- backward ------------------------------------------------------------------------------------------------------------------
// per source row s, channel c: dxl[s] = sum_e alpha[e] gout[dst_e]; ds[e] = alpha[e] xl[s] (gout[dst_e] - dxl[s]) -- the softmax
// backward, since sum_e alpha[e] d alpha[e] = xl[s] dxl[s] when d alpha[e] = gout[dst_e] xl[s].  ds in edge order.
__global__ __launch_bounds__(256) void nc_bwd_row_kernel(int n, int C, const int* __restrict__ src_ptr, const int* __restrict__ src_eid,
                                                         const int* __restrict__ e_dst, const float* __restrict__ alpha,
                                                         const float* __restrict__ xl, const float* __restrict__ gout,
                                                         float* __restrict__ gxl, float* __restrict__ ds) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long long)n * C) return;
    const int s = (int)(gid / C), c = (int)(gid - (long long)s * C);
    const int jb = src_ptr[s], je = src_ptr[s + 1];
    float d = 0.0f;
    for (int j = jb; j < je; ++j) {
        const int e = src_eid[j];
        d += alpha[(size_t)e * C + c] * gout[(size_t)e_dst[e] * C + c];
    }
    gxl[gid] = d;
    const float xv = xl[gid];
    for (int j = jb; j < je; ++j) {
        const int e = src_eid[j];
        const float a = alpha[(size_t)e * C + c];
        ds[(size_t)e * C + c] = a * xv * (gout[(size_t)e_dst[e] * C + c] - d);
    }
}

// per tile of 64 edges (edge order): z = W1 m recomputed, h = PReLU(z) -> H; dh = ds W2; dz = dh (z > 0 ? 1 : a) -> DZ;
// da_part[tile][c] = sum over the tile's edges of dh min(z, 0) (a fixed order: a lane's 16 rows, then the lane groups pairwise)
__global__ __launch_bounds__(256, 2) void nc_edge_bwd_kernel(long long E, int C, int D, const float* __restrict__ wmul,
                                                             const float* __restrict__ W1, const float* __restrict__ prelu,
                                                             const float* __restrict__ W2, const float* __restrict__ ds,
                                                             float* __restrict__ H, float* __restrict__ DZ, float* __restrict__ da_part) {
    extern __shared__ float s_buf[];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l16 = lane & 15, g = lane >> 4;
    const int nb = (C + 15) >> 4, c16 = nb * 16;
    const long long e0 = (long long)blockIdx.x * NC_T;
    const int cnt = (int)(E - e0 < NC_T ? E - e0 : NC_T);
    nc_stage_m(s_buf, wmul, D, cnt, [&](int i) { return e0 + i; });
    __syncthreads();
    f32x4 z[4][4];
    nc_layer1(z, s_buf, W1, C, D, w, l16, g);
    __syncthreads();                                          // the w_mul rows are dead: ds takes their place
    for (int idx = tid; idx < NC_T * c16; idx += blockDim.x) {
        const int i = idx / c16, o = idx - i * c16;
        s_buf[i * NC_HS + o] = (i < cnt && o < C) ? ds[(size_t)(e0 + i) * C + o] : 0.0f;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (w + 4 * j >= nb) continue;
        const int c = 16 * (w + 4 * j) + l16;
        if (c >= C) continue;
        const float sl = prelu[c];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * i + 4 * g + r;
                const float zv = z[i][j][r];
                if (row < cnt) H[(size_t)(e0 + row) * C + c] = zv > 0.0f ? zv : sl * zv;
            }
    }
    __syncthreads();
    f32x4 dh[4][4];
    nc_layer2<false, false>(dh, s_buf, W2, C, w, l16, g);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (w + 4 * j >= nb) continue;
        const int c = 16 * (w + 4 * j) + l16;
        const float sl = c < C ? prelu[c] : 0.0f;
        float dap = 0.0f;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * i + 4 * g + r;
                const float zv = z[i][j][r], d = dh[i][j][r];
                if (row < cnt && c < C) DZ[(size_t)(e0 + row) * C + c] = zv > 0.0f ? d : sl * d;
                dap += d * fminf(zv, 0.0f);
            }
        dap += __shfl_xor(dap, 16);
        dap += __shfl_xor(dap, 32);
        if (g == 0 && c < C) da_part[(size_t)blockIdx.x * C + c] = dap;
    }
}

struct NcGroups {
    const int *src_ptr, *tgt_ptr, *src_eid, *tgt_eid, *e_src, *e_dst;
};
NcGroups nc_groups(const int32_t* d_groups, int n, long long E) {
    NcGroups G;
    G.src_ptr = d_groups;
    G.tgt_ptr = d_groups + (n + 1);
    G.src_eid = d_groups + 2 * (size_t)(n + 1);
    G.tgt_eid = G.src_eid + E;
    G.e_src = G.tgt_eid + E;
    G.e_dst = G.e_src + E;
    return G;
}

hipError_t nc_gemm_launch(bool tb, int M, int N, int K, const float* A, const float* B, const float* bias, float* Cm, hipStream_t s) {
    if (M == 0) return hipSuccess;
    const dim3 grid((M + 63) / 64, (N + 63) / 64);
    if (tb) hipLaunchKernelGGL(nc_gemm_kernel<true>, grid, dim3(256), 0, s, M, N, K, A, B, bias, Cm);
    else hipLaunchKernelGGL(nc_gemm_kernel<false>, grid, dim3(256), 0, s, M, N, K, A, B, bias, Cm);
    return hipGetLastError();
}

}  // namespace

// ======================================================================================================================
// C ABI
// ======================================================================================================================
extern "C" int64_t tlc_nc_group_work_ints(int32_t n_nodes, int64_t n_edges) {
    if (n_nodes < 1 || n_edges < 0) return -1;
    return 2 * (int64_t)n_nodes + 4 * n_edges;
}

extern "C" int tlc_nc_group(int32_t n_nodes, int64_t n_edges, const int64_t* d_edge_index, int32_t* d_groups, int32_t* d_work,
                            int32_t* d_bad, void* stream) {
    TLC_REQUIRE(n_nodes >= 1 && n_edges >= 0, "bad sizes");
    if (n_edges >= (1ll << 31)) {
        tlc_set_error("tlc_nc_group: E = %lld: edge ids are int32 (max 2^31 - 1)", (long long)n_edges);
        return TLC_ERR_UNSUPPORTED;
    }
    TLC_REQUIRE(d_groups && d_work && d_bad && (n_edges == 0 || d_edge_index), "null pointer");
    hipStream_t s = (hipStream_t)stream;
    const long long E = n_edges;
    const size_t n = (size_t)n_nodes;
    int* cnt_s = d_work;
    int* cnt_t = cnt_s + n;
    int* place_s = cnt_t + n;
    int* place_t = place_s + E;
    int* raw_s = place_t + E;
    int* raw_t = raw_s + E;
    int* ptr_s = d_groups;
    int* ptr_t = d_groups + n + 1;
    int* eid_s = d_groups + 2 * (n + 1);
    int* eid_t = eid_s + E;
    int* e_src = eid_t + E;
    int* e_dst = e_src + E;
    TLC_HIP_CHECK(hipMemsetAsync(d_work, 0, 2 * n * sizeof(int), s));
    TLC_HIP_CHECK(hipMemsetAsync(d_bad, 0, sizeof(int), s));
    if (E) TLC_HIP_CHECK(hipMemsetAsync(eid_s, 0, 2 * (size_t)E * sizeof(int), s));      // (invalid edges leave holes: ids 0, in bounds)
    const unsigned eb = (unsigned)((E + 255) / 256);
    if (E) hipLaunchKernelGGL(nc_count_kernel, dim3(eb), dim3(256), 0, s, E, (const long long*)d_edge_index, (int)n_nodes, cnt_s, cnt_t,
                              place_s, place_t, e_src, e_dst, d_bad);
    hipLaunchKernelGGL(nc_scan_kernel, dim3(2), dim3(1024), 0, s, (int)n_nodes, (const int*)cnt_s, (const int*)cnt_t, ptr_s, ptr_t);
    if (E) {
        hipLaunchKernelGGL(nc_fill_kernel, dim3(eb), dim3(256), 0, s, E, (const int*)e_src, (const int*)e_dst, (const int*)place_s,
                           (const int*)place_t, (const int*)ptr_s, (const int*)ptr_t, raw_s, raw_t);
        hipLaunchKernelGGL(nc_rank_kernel, dim3(eb, 2), dim3(256), 0, s, (int)n_nodes, (const int*)e_src, (const int*)e_dst,
                           (const int*)ptr_s, (const int*)ptr_t, (const int*)raw_s, (const int*)raw_t, eid_s, eid_t);
    }
    TLC_HIP_CHECK(hipGetLastError());
    return TLC_OK;
}

extern "C" int tlc_nc_linear_f32(int32_t M, int32_t N, int32_t K, const float* d_x, const float* d_w, const float* d_b, float* d_y,
                                 void* stream) {
    TLC_REQUIRE(M >= 0 && N >= 1 && K >= 1, "bad sizes");
    TLC_REQUIRE(d_w && (M == 0 || (d_x && d_y)), "null pointer");                                   // (M = 0: y has no element)
    TLC_HIP_CHECK(nc_gemm_launch(true, M, N, K, d_x, d_w, d_b, d_y, (hipStream_t)stream));
    return TLC_OK;
}

extern "C" int64_t tlc_nc_linear_bwd_work_floats(int32_t N, int32_t K) {
    if (N < 0 || K < 0) return -1;
    return TlcNcLinearBwdScratch(N, K).total;
}

extern "C" int tlc_nc_linear_bwd_f32(int32_t M, int32_t N, int32_t K, const float* d_x, const float* d_w, const float* d_gy, float* d_gx,
                                     float* d_gw, float* d_gb, float* d_work, void* stream) {
    TLC_REQUIRE(M >= 0 && N >= 1 && K >= 1, "bad sizes");
    TLC_REQUIRE(d_w && d_gw && d_work && (M == 0 || (d_x && d_gy)), "null pointer");
    float* tn = d_work + TlcNcLinearBwdScratch(N, K).tn;
    int rc = tlc_gemm_tn_f32(N, K, M, d_gy, d_x, d_gw, tn, stream);                                  // dW[n][k] = sum_m dy[m][n] x[m][k]
    if (rc != TLC_OK) return rc;
    if (d_gb && (rc = tlc_gemm_tn_f32(1, N, M, nullptr, d_gy, d_gb, tn, stream)) != TLC_OK) return rc;
    if (d_gx) TLC_HIP_CHECK(nc_gemm_launch(false, M, K, N, d_gy, d_w, nullptr, d_gx, (hipStream_t)stream));
    return TLC_OK;
}

extern "C" int64_t tlc_nc_curv_work_bytes(int32_t n_nodes, int64_t n_edges, int32_t C, int32_t D) {
    if (n_nodes < 1 || n_edges < 0 || C < 1 || C > NC_MAX_C || D < 1 || D > NC_MAX_D) return -1;
    const long long tiles = (n_edges + NC_T - 1) / NC_T;
    return 4 * (3 * n_edges * C + tiles * C + TlcGemmTnScratch(C, C > D ? C : D).total);      // (tn: the largest of its four products)
}

static int nc_check_shape(const char* fn, int32_t n_nodes, int64_t n_edges, int32_t C, int32_t D) {
    if (n_nodes < 1 || n_edges < 0 || C < 1 || D < 1) {
        tlc_set_error("%s: bad sizes", fn);
        return TLC_ERR_INVALID_ARG;
    }
    if (C > NC_MAX_C || D > NC_MAX_D || n_edges >= (1ll << 31)) {
        tlc_set_error("%s: C = %d (max %d), D = %d (max %d), E = %lld (max 2^31 - 1): not built", fn, C, NC_MAX_C, D, NC_MAX_D,
                      (long long)n_edges);
        return TLC_ERR_UNSUPPORTED;
    }
    return TLC_OK;
}

extern "C" int tlc_nc_curv_fwd_f32(int32_t n_nodes, int64_t n_edges, int32_t C, int32_t D, const int32_t* d_groups, const float* d_xl,
                                   const float* d_wmul, const float* d_w1, const float* d_prelu, const float* d_w2, const float* d_b2,
                                   float* d_alpha, float* d_out, void* stream) {
    int rc = nc_check_shape(__func__, n_nodes, n_edges, C, D);
    if (rc != TLC_OK) return rc;
    TLC_REQUIRE(d_groups && d_xl && d_out, "null pointer");
    TLC_REQUIRE(n_edges == 0 || (d_wmul && d_w1 && d_prelu && d_w2 && d_b2 && d_alpha), "null pointer");
    hipStream_t s = (hipStream_t)stream;
    const NcGroups G = nc_groups(d_groups, n_nodes, n_edges);
    if (n_edges) {
        const bool vec = (C % 4) == 0 && (reinterpret_cast<uintptr_t>(d_w2) & 15) == 0;
        const void* kern = vec ? (const void*)nc_edge_fwd_kernel<true> : (const void*)nc_edge_fwd_kernel<false>;
        TLC_HIP_CHECK(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, NC_LDS_BYTES));
        const unsigned tiles = (unsigned)((n_edges + NC_T - 1) / NC_T);
        if (vec) hipLaunchKernelGGL(nc_edge_fwd_kernel<true>, dim3(tiles), dim3(256), NC_LDS_BYTES, s, (int)n_nodes, (int)C, (int)D, G.src_ptr,
                                    G.src_eid, G.e_src, d_wmul, d_w1, d_prelu, d_w2, d_b2, d_alpha);
        else hipLaunchKernelGGL(nc_edge_fwd_kernel<false>, dim3(tiles), dim3(256), NC_LDS_BYTES, s, (int)n_nodes, (int)C, (int)D, G.src_ptr,
                                G.src_eid, G.e_src, d_wmul, d_w1, d_prelu, d_w2, d_b2, d_alpha);
    }
    const long long th = (long long)n_nodes * C;
    hipLaunchKernelGGL(nc_aggr_kernel, dim3((unsigned)((th + 255) / 256)), dim3(256), 0, s, (int)n_nodes, (int)C, G.tgt_ptr, G.tgt_eid,
                       G.e_src, (const float*)d_alpha, d_xl, d_out);
    TLC_HIP_CHECK(hipGetLastError());
    return TLC_OK;
}

extern "C" int tlc_nc_curv_bwd_f32(int32_t n_nodes, int64_t n_edges, int32_t C, int32_t D, const int32_t* d_groups, const float* d_xl,
                                   const float* d_wmul, const float* d_w1, const float* d_prelu, const float* d_w2, const float* d_alpha,
                                   const float* d_gout, float* d_gxl, float* d_gw1, float* d_gprelu, float* d_gw2, float* d_gb2,
                                   void* d_work, int64_t work_bytes, void* stream) {
    int rc = nc_check_shape(__func__, n_nodes, n_edges, C, D);
    if (rc != TLC_OK) return rc;
    TLC_REQUIRE(d_groups && d_xl && d_gout && d_gxl && d_gw1 && d_gprelu && d_gw2 && d_gb2 && d_work, "null pointer");
    TLC_REQUIRE(n_edges == 0 || (d_wmul && d_w1 && d_prelu && d_w2 && d_alpha), "null pointer");
    TLC_REQUIRE(work_bytes >= tlc_nc_curv_work_bytes(n_nodes, n_edges, C, D), "workspace smaller than tlc_nc_curv_work_bytes");
    hipStream_t s = (hipStream_t)stream;
    const NcGroups G = nc_groups(d_groups, n_nodes, n_edges);
    const long long E = n_edges, EC = E * C, tiles = (E + NC_T - 1) / NC_T;
    float* ds = (float*)d_work;
    float* H = ds + EC;
    float* DZ = H + EC;
    float* da_part = DZ + EC;
    float* tn = da_part + tiles * C;
    const long long th = (long long)n_nodes * C;
    hipLaunchKernelGGL(nc_bwd_row_kernel, dim3((unsigned)((th + 255) / 256)), dim3(256), 0, s, (int)n_nodes, (int)C, G.src_ptr, G.src_eid,
                       G.e_dst, d_alpha, d_xl, d_gout, d_gxl, ds);
    if (E) {
        TLC_HIP_CHECK(hipFuncSetAttribute((const void*)nc_edge_bwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, NC_LDS_BYTES));
        hipLaunchKernelGGL(nc_edge_bwd_kernel, dim3((unsigned)tiles), dim3(256), NC_LDS_BYTES, s, E, (int)C, (int)D, d_wmul, d_w1, d_prelu,
                           d_w2, (const float*)ds, H, DZ, da_part);
    }
    TLC_HIP_CHECK(hipGetLastError());
    // weight gradients: sums over the edges as fixed-order split-K products (tlc_gemm_tn_f32, lp_backward.hip)
    if ((rc = tlc_gemm_tn_f32(C, C, E, ds, H, d_gw2, tn, stream)) != TLC_OK) return rc;             // dW2[o][c] = sum_e ds[e][o] h[e][c]
    if ((rc = tlc_gemm_tn_f32(1, C, E, nullptr, ds, d_gb2, tn, stream)) != TLC_OK) return rc;       // db2 = sum_e ds[e]
    if ((rc = tlc_gemm_tn_f32(C, D, E, DZ, d_wmul, d_gw1, tn, stream)) != TLC_OK) return rc;        // dW1[c][k] = sum_e dz[e][c] m[e][k]
    return tlc_gemm_tn_f32(1, C, tiles, nullptr, da_part, d_gprelu, tn, stream);                    // da = sum of the tiles' partials
}

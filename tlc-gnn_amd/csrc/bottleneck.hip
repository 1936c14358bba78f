// bottleneck.hip -- the bottleneck distance d_B between a predicted and a target persistence diagram, a witness matching and the
// gradient of d_B in both diagrams (include/tlcgnn.h states the function operation by operation).
//
// The N x N problem of tlc_w2_inference_matching (N = n + m: the predicted points, then m copies of the diagonal, onto the targets, then
// n copies of the diagonal) with the objective  max  instead of  sum:  d_B = the least t for which a perfect matching uses only costs
// <= t.  The method is the sibling of w2_match.hip's shortest augmenting paths, lanes = columns, costs recomputed from the two points:
// a path's length is the MAXIMUM of the costs of the edges it adds, so there are no duals and nothing to update.
//     t = max_j min_i c(i, j)                       a lower bound of d_B: every column has to take some row
//     for every row i ascending (rows < i are matched):
//         a Dijkstra search over alternating paths from i; key(j) = max(t, the largest cost on the best path to column j); the column
//         popped next is the least (key, matched, j) -- among equal keys a free column ends the search, then the lowest column;
//         augment along the path to the free column popped; t = its key.
// Invariant: the matching's costs are <= t <= d_B (in the graph of the costs <= d_B a perfect matching exists, so by Berge's lemma a
// free row starts an augmenting path there: the key of the free column found is <= d_B).  At the end the matching is perfect, so its
// largest cost is >= d_B as well: d_dist is read off the matching, one entry of the cost matrix, no arithmetic on it.
// A search pops at most N columns, there are N searches: every loop is bounded by N.  No floating-point atomics, no atomics at all.
//
// Two size classes by N alone: one wavefront per problem up to TLC_BN_WAVE_NMAX rows (64 .. 512 columns in registers, the variant picked
// from the batch's largest such problem -- the selection rule names columns, not lanes, so every variant gives the same bits), one
// 512-thread workgroup per problem up to TLC_BN_NMAX (one barrier per step: the wavefronts' minima go through two alternating LDS rows).
#include <stdlib.h>

#include "tlc_common.h"

namespace {

struct BnParams {
    int n_pairs;
    const long long* xoff;     // [B+1]
    const double* X;           // [sum n, 2] predicted (birth, death)
    const long long* yoff;     // [B+1]
    const double* Y;           // [sum m, 2] target
    double* dist;              // [B]
    int* arg;                  // [B, 2]
    int* assign_x;             // [sum n]: target index (problem-local), -1 = diagonal
    int* assign_y;             // [sum m]: predicted index, -1 = diagonal
    double* gradX;             // [sum n, 2] or null
    double* gradY;             // [sum m, 2] or null
    unsigned char* status;     // [B]
};

constexpr int BN_WAVE_NMAX = TLC_BN_WAVE_NMAX, BN_NMAX = TLC_BN_NMAX;
constexpr int BN_WIDE_THREADS = 512, BN_WIDE_CPL = BN_NMAX / BN_WIDE_THREADS, BN_NONE = 0x7fffffff, BN_MATCHED = 1 << 30;
static_assert(BN_WIDE_THREADS * BN_WIDE_CPL == BN_NMAX, "the workgroup's columns");

template <int T>
__device__ __forceinline__ void bn_sync() {
    if (T == 64) { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); }
    else __syncthreads();
}

// The least (MAX: the greatest) val over the threads and, among the threads that hold it, the least code; every thread gets both.
// T > 64: through row `slot` (0 / 1, alternating between consecutive calls) of red / redi, ONE barrier: a thread that writes row s again
// has passed the barrier of the call in between, which every reader of row s reaches only after its reads.
template <int T, bool MAX>
__device__ __forceinline__ void bn_select(double& val, int& code, double* red, int* redi, int slot) {
    const double w = MAX ? tlc_wave_max_f64(val) : tlc_wave_min_f64(val);
    const int c = tlc_wave_min_i32(val == w ? code : BN_NONE);
    if (T == 64) { val = w; code = c; return; }
    constexpr int NWV = T / 64;
    const int wave = (int)threadIdx.x >> 6;
    if (tlc_lane() == 0) { red[slot * NWV + wave] = w; redi[slot * NWV + wave] = c; }
    __syncthreads();
    double v = red[slot * NWV];
    int k = redi[slot * NWV];
#pragma unroll
    for (int q = 1; q < NWV; ++q) {
        const double d = red[slot * NWV + q];
        const int e = redi[slot * NWV + q];
        if ((MAX ? d > v : d < v) || (d == v && e < k)) { v = d; k = e; }
    }
    val = v; code = k;
}

// A problem that is not solved: defined outputs (distance 0 or NaN, no matching, no witness pair, zero gradients)
template <int T>
__device__ __forceinline__ void bn_fail(const BnParams& p, int b, long long x0, long long y0, int n, int m, int code, double d, int tid) {
    if (tid == 0) { p.status[b] = (unsigned char)code; p.dist[b] = d; p.arg[2 * b] = -1; p.arg[2 * b + 1] = -1; }
    for (int i = tid; i < n; i += T) {
        p.assign_x[x0 + i] = -1;
        if (p.gradX) { p.gradX[2 * (x0 + i)] = 0.0; p.gradX[2 * (x0 + i) + 1] = 0.0; }
    }
    for (int j = tid; j < m; j += T) {
        p.assign_y[y0 + j] = -1;
        if (p.gradY) { p.gradY[2 * (y0 + j)] = 0.0; p.gradY[2 * (y0 + j) + 1] = 0.0; }
    }
}

__device__ __forceinline__ double bn_sign(double v) { return v > 0.0 ? 1.0 : (v < 0.0 ? -1.0 : 0.0); }

// One problem of 1 <= N <= T * CPL rows on T threads; column j belongs to thread j % T (register slot j / T).
// LDS: xs, ys [N] the predicted points (0 for the diagonal rows), pcol [N] the row of column j or -1, way [N] the column before j on
// the best path (-1: the row the search started from), red [2 T/64] / redi [2 T/64 + 2] the reductions and two words to share.
template <int T, int CPL>
__device__ __forceinline__ void bn_solve(const BnParams& p, int b, long long x0, long long y0, int n, int m, double* xs, double* ys,
                                         int* pcol, int* way, double* red, int* redi) {
    constexpr int NWV = T / 64;
    const int tid = (int)threadIdx.x, N = n + m;
    const double INF = __longlong_as_double(0x7FF0000000000000ll);
    const double QNAN = __longlong_as_double(0x7FF8000000000000ll);
    bool finite = true;
    for (int i = tid; i < N; i += T) {
        double bx = 0.0, by = 0.0;
        if (i < n) { bx = p.X[2 * (x0 + i)]; by = p.X[2 * (x0 + i) + 1]; }
        finite = finite && (bx - bx == 0.0) && (by - by == 0.0);
        xs[i] = bx; ys[i] = by; pcol[i] = -1;
    }
    double yx[CPL], yy[CPL], cdy[CPL], key[CPL];
    bool used[CPL], taken[CPL];
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
        const int j = tid + T * c;
        yx[c] = yy[c] = 0.0;
        if (j < m) { yx[c] = p.Y[2 * (y0 + j)]; yy[c] = p.Y[2 * (y0 + j) + 1]; }
        finite = finite && (yx[c] - yx[c] == 0.0) && (yy[c] - yy[c] == 0.0);
        cdy[c] = fabs(yy[c] - yx[c]) * 0.5;
    }
    if (T == 64) {
        if (__ballot(!finite)) { bn_fail<T>(p, b, x0, y0, n, m, 3, QNAN, tid); return; }
    } else {
        if (tid == 0) redi[2 * NWV] = 0;
        __syncthreads();
        if (!finite) redi[2 * NWV] = 1;
        __syncthreads();
        if (redi[2 * NWV]) { bn_fail<T>(p, b, x0, y0, n, m, 3, QNAN, tid); return; }     // (uniform)
    }
    bn_sync<T>();
    // c(i, j) from the two points: plain subtract, abs, max and multiply
    auto cost_of = [&](bool row_real, double xi, double yi, double cd, int j, int c) -> double {
        if (j < m) {
            if (row_real) {
                const double dx = fabs(xi - yx[c]), dy = fabs(yi - yy[c]);
                return dx > dy ? dx : dy;
            }
            return cdy[c];
        }
        return row_real ? cd : 0.0;
    };
    // ---- the start threshold: every column takes some row, so d_B >= max_j min_i c(i, j) ------------------------------------------
    double t = 0.0;
    {
#pragma unroll
        for (int c = 0; c < CPL; ++c) key[c] = INF;
        for (int i = 0; i < N; ++i) {
            const double xi = xs[i], yi = ys[i], cd = fabs(yi - xi) * 0.5;
#pragma unroll
            for (int c = 0; c < CPL; ++c) {
                const double cost = cost_of(i < n, xi, yi, cd, tid + T * c, c);
                key[c] = cost < key[c] ? cost : key[c];
            }
        }
#pragma unroll
        for (int c = 0; c < CPL; ++c) if (tid + T * c < N && key[c] > t) t = key[c];
        int none = BN_NONE;
        bn_select<T, true>(t, none, red, redi, 0);
    }
    int slot = 1;
    // ---- one search and one augmentation per row ---------------------------------------------------------------------------------
    for (int i = 0; i < N; ++i) {
#pragma unroll
        for (int c = 0; c < CPL; ++c) { const int j = tid + T * c; used[c] = false; taken[c] = j < N && pcol[j] >= 0; key[c] = INF; }
        int i0 = i, j0 = -1;
        double cur = t;
        for (;;) {
            const double xi = xs[i0], yi = ys[i0], cd = fabs(yi - xi) * 0.5;
            const bool real = i0 < n;
            double best = INF;
            int bc = BN_NONE;
#pragma unroll
            for (int c = 0; c < CPL; ++c) {
                const int j = tid + T * c;
                if (j < N && !used[c]) {
                    const double cost = cost_of(real, xi, yi, cd, j, c);
                    const double cand = cost > cur ? cost : cur;
                    // (the first step of a search sets every key, so a key that is +Inf has its link too)
                    if (j0 < 0 || cand < key[c]) { key[c] = cand; way[j] = j0; }
                    const int code = j | (taken[c] ? BN_MATCHED : 0);
                    if (key[c] < best || (key[c] == best && code < bc)) { best = key[c]; bc = code; }
                }
            }
            bn_select<T, false>(best, bc, red, redi, slot);
            slot ^= 1;
            if (bc == BN_NONE) {                                      // (uniform; cannot happen: a free column is never popped twice)
                bn_sync<T>();
                bn_fail<T>(p, b, x0, y0, n, m, 3, QNAN, tid);
                return;
            }
            const int j1 = bc & (BN_MATCHED - 1);
            cur = best;
            j0 = j1;
#pragma unroll
            for (int c = 0; c < CPL; ++c) if (tid + T * c == j1) used[c] = true;
            if (!(bc & BN_MATCHED)) break;
            i0 = pcol[j1];
        }
        t = cur;
        bn_sync<T>();                                                 // the links of this search
        if (tid == 0) {
            int j = j0;
            while (j >= 0) {                                          // (at most N links)
                const int jp = way[j];
                pcol[j] = jp < 0 ? i : pcol[jp];
                j = jp;
            }
        }
        bn_sync<T>();
    }
    // ---- the witness: the matching, its largest cost and the pair that attains it --------------------------------------------------
    double dmax = 0.0;
    int dcode = BN_NONE;
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
        const int j = tid + T * c;
        if (j < N) {
            const int i = pcol[j];
            double cost = 0.0;
            int code = BN_NONE;                                       // a predicted point under its index; then the pairs (-1, j) by j
            if (i < n) {
                code = i;
                if (j < m) {
                    const double dx = fabs(xs[i] - yx[c]), dy = fabs(ys[i] - yy[c]);
                    cost = dx > dy ? dx : dy;
                    p.assign_x[x0 + i] = j; p.assign_y[y0 + j] = i;
                } else {
                    cost = fabs(ys[i] - xs[i]) * 0.5;
                    p.assign_x[x0 + i] = -1;
                }
            } else if (j < m) {
                code = n + j;
                cost = cdy[c];
                p.assign_y[y0 + j] = -1;
            }
            if (code != BN_NONE && (cost > dmax || (cost == dmax && code < dcode))) { dmax = cost; dcode = code; }
        }
    }
    bn_select<T, true>(dmax, dcode, red, redi, slot);
    // (N >= 1: some pair has a point, and every cost is >= +0.0 = the start of the maximum, so dcode names a pair)
    int ai = -1, aj = -1;
    if (dcode != BN_NONE) {
        if (dcode < n) { ai = dcode; }
        else aj = dcode - n;
    }
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
        const int j = tid + T * c;
        if (j < N && ai >= 0 && pcol[j] == ai) redi[2 * NWV + 1] = j < m ? j : -1;
    }
    bn_sync<T>();
    if (ai >= 0) aj = redi[2 * NWV + 1];
    if (tid == 0) { p.status[b] = 0; p.dist[b] = dmax; p.arg[2 * b] = ai; p.arg[2 * b + 1] = aj; }
    // ---- the gradient: one pair's rows, everything else zero ----------------------------------------------------------------------
    double gxb = 0.0, gxd = 0.0, gyb = 0.0, gyd = 0.0;                // d d_B / d X[ai], d d_B / d Y[aj]
    if (ai >= 0 && aj >= 0) {
        const double ex = xs[ai] - p.Y[2 * (y0 + aj)], ey = ys[ai] - p.Y[2 * (y0 + aj) + 1];
        if (fabs(ex) >= fabs(ey)) { gxb = bn_sign(ex); gyb = bn_sign(-ex); }             // (birth wins an exact tie)
        else { gxd = bn_sign(ey); gyd = bn_sign(-ey); }
    } else if (ai >= 0) {
        const double s = bn_sign(ys[ai] - xs[ai]);
        gxb = s > 0.0 ? -0.5 : (s < 0.0 ? 0.5 : 0.0); gxd = s > 0.0 ? 0.5 : (s < 0.0 ? -0.5 : 0.0);
    } else if (aj >= 0) {
        const double s = bn_sign(p.Y[2 * (y0 + aj) + 1] - p.Y[2 * (y0 + aj)]);
        gyb = s > 0.0 ? -0.5 : (s < 0.0 ? 0.5 : 0.0); gyd = s > 0.0 ? 0.5 : (s < 0.0 ? -0.5 : 0.0);
    }
    if (p.gradX)
        for (int i = tid; i < n; i += T) { p.gradX[2 * (x0 + i)] = i == ai ? gxb : 0.0; p.gradX[2 * (x0 + i) + 1] = i == ai ? gxd : 0.0; }
    if (p.gradY)
        for (int j = tid; j < m; j += T) { p.gradY[2 * (y0 + j)] = j == aj ? gyb : 0.0; p.gradY[2 * (y0 + j) + 1] = j == aj ? gyd : 0.0; }
}

// N <= 64 CPL (<= TLC_BN_WAVE_NMAX): a wavefront per problem, the problems by the grid's stride; larger ones are the workgroup kernel's
template <int CPL>
__global__ __launch_bounds__(64) void tlc_bn_wave_kernel(BnParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char bn_lds[];
    constexpr int NMAX = 64 * CPL;
    double* xs = (double*)bn_lds;
    double* ys = xs + NMAX;
    double* red = ys + NMAX;                   // [2] (a wavefront reduces in registers)
    int* pcol = (int*)(red + 2);
    int* way = pcol + NMAX;
    int* redi = way + NMAX;                    // [4]
    const int lane = tlc_lane();
    for (int b = blockIdx.x; b < p.n_pairs; b += gridDim.x) {
        const long long x0 = p.xoff[b], y0 = p.yoff[b];
        const long long n = p.xoff[b + 1] - x0, m = p.yoff[b + 1] - y0;
        if (n + m > NMAX) continue;            // (the entry picked CPL from the offsets: this is a problem above TLC_BN_WAVE_NMAX)
        if (n + m == 0) { bn_fail<64>(p, b, x0, y0, 0, 0, 0, 0.0, lane); continue; }
        bn_solve<64, CPL>(p, b, x0, y0, (int)n, (int)m, xs, ys, pcol, way, red, redi);
        bn_sync<64>();
    }
}

// TLC_BN_WAVE_NMAX < N <= TLC_BN_NMAX: a workgroup per problem; above: status 2
__global__ __launch_bounds__(BN_WIDE_THREADS) void tlc_bn_wide_kernel(BnParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char bn_lds[];
    constexpr int NWV = BN_WIDE_THREADS / 64;
    double* xs = (double*)bn_lds;
    double* ys = xs + BN_NMAX;
    double* red = ys + BN_NMAX;                // [2 NWV]
    int* pcol = (int*)(red + 2 * NWV);
    int* way = pcol + BN_NMAX;
    int* redi = way + BN_NMAX;                 // [2 NWV + 2]
    const int b = blockIdx.x;
    if (b >= p.n_pairs) return;
    const long long x0 = p.xoff[b], y0 = p.yoff[b];
    const long long n = p.xoff[b + 1] - x0, m = p.yoff[b + 1] - y0;
    if (n + m <= BN_WAVE_NMAX) return;         // (the wavefront kernel took it)
    if (n + m > BN_NMAX) {
        // (counts clamped for the loops: the rows of such a problem are still its own)
        bn_fail<BN_WIDE_THREADS>(p, b, x0, y0, (int)(n < 0x7fffffff ? n : 0x7fffffff), (int)(m < 0x7fffffff ? m : 0x7fffffff), 2, 0.0, (int)threadIdx.x);
        return;
    }
    bn_solve<BN_WIDE_THREADS, BN_WIDE_CPL>(p, b, x0, y0, (int)n, (int)m, xs, ys, pcol, way, red, redi);
}

template <int CPL>
static int launch_bn_wave(const BnParams& p, hipStream_t s) {
    const size_t lds = (size_t)64 * CPL * (2 * 8 + 2 * 4) + 2 * 8 + 4 * 4;
    const int grid = p.n_pairs < 16384 ? p.n_pairs : 16384;
    hipLaunchKernelGGL((tlc_bn_wave_kernel<CPL>), dim3(grid), dim3(64), lds, s, p);
    TLC_HIP_CHECK(hipGetLastError());
    return TLC_OK;
}

static int launch_bn_wide(const BnParams& p, hipStream_t s) {
    constexpr int NWV = BN_WIDE_THREADS / 64;
    const size_t lds = (size_t)BN_NMAX * (2 * 8 + 2 * 4) + 2 * NWV * 8 + (2 * NWV + 2) * 4;
    TLC_HIP_CHECK(hipFuncSetAttribute((const void*)tlc_bn_wide_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(tlc_bn_wide_kernel, dim3(p.n_pairs), dim3(BN_WIDE_THREADS), lds, s, p);
    TLC_HIP_CHECK(hipGetLastError());
    return TLC_OK;
}

}  // namespace

extern "C" int tlc_bottleneck_matching(int32_t n_problems, const int64_t* d_xoff, const double* d_X, const int64_t* d_yoff, const double* d_Y,
                                       int32_t max_points, double* d_dist, int32_t* d_arg, int32_t* d_assign_x, int32_t* d_assign_y,
                                       double* d_gradX, double* d_gradY, uint8_t* d_status, void* stream) {
    TLC_REQUIRE(n_problems >= 0, "n_problems < 0");
    TLC_REQUIRE(max_points >= 0, "max_points < 0");
    if (n_problems == 0) return TLC_OK;
    TLC_REQUIRE(d_xoff && d_yoff && d_dist && d_arg && d_assign_x && d_assign_y && d_status, "null pointer");
    TLC_REQUIRE(max_points == 0 || d_X || d_Y, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    const size_t B = (size_t)n_problems;
    int64_t* offs = (int64_t*)malloc((B + 1) * 2 * sizeof(int64_t));
    if (!offs) { tlc_set_error("%s: out of host memory", __func__); return TLC_ERR_OUT_OF_MEMORY; }
    struct Free { int64_t* p; ~Free() { free(p); } } guard{offs};
    if (hipMemcpyAsync(offs, d_xoff, (B + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(offs + B + 1, d_yoff, (B + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) {
        tlc_set_error("%s: reading the offsets failed: %s", __func__, hipGetErrorString(hipGetLastError()));
        return TLC_ERR_HIP;
    }
    const int64_t *xo = offs, *yo = offs + B + 1;
    if (xo[0] < 0 || yo[0] < 0) { tlc_set_error("%s: negative offset", __func__); return TLC_ERR_INVALID_ARG; }
    long long wave_max = 0, n_wave = 0, n_wide = 0, sum_n = 0, sum_m = 0;
    for (size_t q = 0; q < B; ++q) {
        const long long n = xo[q + 1] - xo[q], m = yo[q + 1] - yo[q];
        if (n < 0 || m < 0) { tlc_set_error("%s: the offsets of problem %lld decrease", __func__, (long long)q); return TLC_ERR_INVALID_ARG; }
        if (n + m > max_points) {
            tlc_set_error("%s: problem %lld has %lld points, max_points is %lld", __func__, (long long)q, n + m, (long long)max_points);
            return TLC_ERR_INVALID_ARG;
        }
        if (n + m <= BN_WAVE_NMAX) { ++n_wave; wave_max = n + m > wave_max ? n + m : wave_max; }
        else ++n_wide;
        sum_n += n; sum_m += m;
    }
    TLC_REQUIRE((sum_n == 0 || d_X) && (sum_m == 0 || d_Y), "null pointer");
    BnParams p;
    memset(&p, 0, sizeof(p));
    p.n_pairs = n_problems; p.xoff = (const long long*)d_xoff; p.X = d_X; p.yoff = (const long long*)d_yoff; p.Y = d_Y;
    p.dist = d_dist; p.arg = d_arg; p.assign_x = d_assign_x; p.assign_y = d_assign_y; p.gradX = d_gradX; p.gradY = d_gradY; p.status = d_status;
    int rc = TLC_OK;
    if (n_wave) {
        if (wave_max <= 64) rc = launch_bn_wave<1>(p, st);
        else if (wave_max <= 128) rc = launch_bn_wave<2>(p, st);
        else if (wave_max <= 256) rc = launch_bn_wave<4>(p, st);
        else rc = launch_bn_wave<8>(p, st);
    }
    if (rc == TLC_OK && n_wide) rc = launch_bn_wide(p, st);
    return rc;
}

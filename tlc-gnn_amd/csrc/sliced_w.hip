// sliced_w.hip -- the sliced Wasserstein distance between persistence diagrams and its gradient (tlc_sliced_wasserstein).
//
// Replaces the 'sliced' branch of Knowledge_Distillation/Teacher_model.py:110-124 (`compute_PD_loss(kernel='sliced')`, the distance of
// Carriere et al.): for every direction l on the half circle each diagram is projected on l and augmented by the projections of the
// OTHER diagram's diagonal points, both lists are sorted and the L1 distance of the sorted lists is summed over the directions.  The
// function, the stable order and the one sequence of roundings of the gradient are defined in include/tlcgnn.h; this file is three
// implementations of that definition, cut on the device by N = n + m (every kernel skips the problems of the other classes):
//
//   N <= TLC_SW_WAVE_NMAX   one wavefront per problem, SW_BS / 64 problems per workgroup, grid-stride over the batch.  Lane a holds element
//                           a of V1 and element a of V2 as (order-preserving u64 key, listing index); the bitonic network runs across
//                           the lanes on the vector ALU (tlc_lane_xor_*: DPP and the permlane swaps, no LDS).  A rank's sign is pushed to
//                           the lane of its listing index (ds_permute: the crossbar, no LDS memory); lane a owns the point at position a
//                           of V1 and keeps its two accumulators in registers across the directions.
//                           Rank sum: the butterfly  k ^ 1, k ^ 2, ... k ^ 32  over the 64 ranks (absent ranks add +0.0).
//   N <= TLC_SW_LDS_NMAX    one workgroup per problem: both (key, index) lists in LDS (2 x 10 B per element), one bitonic network for both,
//                           the signs scattered to listing positions as bytes in LDS; thread t owns the points at positions t, t + SW_BS, ...
//                           of V1 (coordinates and accumulators in registers).
//                           Rank sum: thread t adds its ranks t, t + SW_BS, ... ascending; the butterfly inside each wavefront; the
//                           wavefronts ascending.
//   above                   the whole device, one problem after the other: the items (direction, list, element) of as many directions as
//                           the workspace holds are sorted by radix_passes.h -- eight passes over the keys and a ninth over the segment
//                           number 2 * direction + list, the leading digit -- the sign bytes go to [segment][listing position], and one
//                           kernel sums each point's directions in ascending order (continuing from the stored value in later groups:
//                           the same roundings whatever the group size).
//                           Rank sum: tiles of SW_TILE ranks (inside a tile as in the workgroup class), the tiles ascending.
// A wavefront of the LDS bitonic reads key[i] / key[i | j] for consecutive t as 8-byte words: for j >= 32 a 32-lane half reads 32
// consecutive words (conflict free); for j < 32 the pairs interleave and the half touches every bank twice (2-way), the same as the
// 4-byte sorts of pd_grad.hip / lp_metrics.hip at j = 1.
#include "radix_passes.h"

#include <stdlib.h>

namespace {

#define SW_BS 256
#define SW_WAVES (SW_BS / 64)
#define SW_MAX_GRID 2048
#define SW_WAVE_N TLC_SW_WAVE_NMAX
#define SW_LDS_N TLC_SW_LDS_NMAX
#define SW_PER_THREAD (SW_LDS_N / SW_BS)     // points a thread of the workgroup class owns
#define SW_TILE 1024                         // ranks per partial sum of the device-wide class
#define SW_WIDE_MAX_ITEMS (1ll << 27)        // directions x points of one group
static_assert(SW_BS == RK_BS, "the radix passes and the kernels here share one workgroup width");
static_assert(SW_WAVE_N == 64, "one lane per element");
static_assert((SW_LDS_N & (SW_LDS_N - 1)) == 0 && SW_LDS_N >= 2048 && SW_LDS_N <= 65536, "a power of two whose indices fit 16 bits");
static_assert(2 * TLC_SW_MAX_DIRS <= 256, "the segment number is one radix digit");
static_assert(SW_TILE % SW_BS == 0, "whole rounds");

// tlc_ord_f64 back to the double (-0.0 comes back as +0.0)
__device__ __forceinline__ double sw_val(unsigned long long k) {
    return __longlong_as_double((long long)((k & 0x8000000000000000ull) ? (k ^ 0x8000000000000000ull) : ~k));
}
__device__ __forceinline__ bool sw_finite(double x) {
    return ((unsigned long long)__double_as_longlong(x) & 0x7FF0000000000000ull) != 0x7FF0000000000000ull;
}
__device__ __forceinline__ double sw_sign(double x) { return x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : 0.0); }
__device__ __forceinline__ double sw_nan() { return __longlong_as_double(0x7FF8000000000000ll); }

struct SwArgs {
    int n_problems;
    const long long *xoff, *yoff;
    const double *X, *Y;
    int n_dirs;
    const double* dirs;      // [n_dirs, 2]
    double scale;
    double *loss, *gradX, *gradY;
    unsigned char* status;
};

// One point of a problem at position a of V1 (X's points, then Y's): its two list values for direction (l0, l1), where its V2 element
// sits, and its gradient step.
struct SwPoint {
    double b, d;
    __device__ __forceinline__ double proj(double l0, double l1) const { return l0 * b + l1 * d; }
    __device__ __forceinline__ double diag(double l0, double l1) const { return (l0 + l1) * (fabs(b + d) * 0.5); }
};
// position in V2 of the point at position a of V1
__device__ __forceinline__ int sw_other(int a, int n, int m) { return a < n ? m + a : a - n; }
// the header's sequence for one direction: sa = the sign at position a of V1, sb = the sign at this point's position of V2
__device__ __forceinline__ void sw_step(double& g0, double& g1, bool is_x, double sa, double sb, double sg, double t0, double t1, double u) {
    if (is_x) {
        g0 += sa * t0; g0 -= sb * sg * u;
        g1 += sa * t1; g1 -= sb * sg * u;
    } else {
        g0 -= sb * t0; g0 += sa * sg * u;
        g1 -= sb * t1; g1 += sa * sg * u;
    }
}

// ---- N <= 64: one wavefront per problem ---------------------------------------------------------------------------------------
template <int K, int J>
__device__ __forceinline__ void sw_wave_cx(unsigned long long& k, unsigned& i, int lane) {
    const unsigned long long ok = tlc_lane_xor_u64<J>(k);
    const unsigned oi = tlc_lane_xor_u32<J>(i);
    const bool other_less = ok < k || (ok == k && oi < i);
    const bool take_min = ((lane & J) == 0) == ((lane & K) == 0);
    if (take_min == other_less) { k = ok; i = oi; }
}
template <int K, int J>
__device__ __forceinline__ void sw_wave_merge(unsigned long long& k1, unsigned& i1, unsigned long long& k2, unsigned& i2, int lane) {
    sw_wave_cx<K, J>(k1, i1, lane);
    sw_wave_cx<K, J>(k2, i2, lane);
    if constexpr (J > 1) sw_wave_merge<K, J / 2>(k1, i1, k2, i2, lane);
}
__device__ __forceinline__ void sw_wave_sort2(unsigned long long& k1, unsigned& i1, unsigned long long& k2, unsigned& i2, int lane) {
    sw_wave_merge<2, 1>(k1, i1, k2, i2, lane);
    sw_wave_merge<4, 2>(k1, i1, k2, i2, lane);
    sw_wave_merge<8, 4>(k1, i1, k2, i2, lane);
    sw_wave_merge<16, 8>(k1, i1, k2, i2, lane);
    sw_wave_merge<32, 16>(k1, i1, k2, i2, lane);
    sw_wave_merge<64, 32>(k1, i1, k2, i2, lane);
}
__device__ __forceinline__ double sw_wave_sum(double v) {
    v += tlc_lane_xor_f64<1>(v);
    v += tlc_lane_xor_f64<2>(v);
    v += tlc_lane_xor_f64<4>(v);
    v += tlc_lane_xor_f64<8>(v);
    v += tlc_lane_xor_f64<16>(v);
    v += tlc_lane_xor_f64<32>(v);
    return v;
}

__global__ __launch_bounds__(SW_BS) void sw_wave_kernel(SwArgs A) {
    const int lane = (int)(threadIdx.x & 63);
    const long long w0 = (long long)blockIdx.x * SW_WAVES + (threadIdx.x >> 6), stride = (long long)gridDim.x * SW_WAVES;
    for (long long p = w0; p < A.n_problems; p += stride) {
        const long long x0 = A.xoff[p], y0 = A.yoff[p];
        const long long nn = A.xoff[p + 1] - x0, mm = A.yoff[p + 1] - y0;
        if (nn + mm > SW_WAVE_N) continue;
        const int n = (int)nn, m = (int)mm, N = n + m;
        const bool has = lane < N;
        // element `lane` of V1 is point P (X's points, then Y's); element `lane` of V2 is point Q (Y's points, then X's)
        const bool p_is_x = lane < n, q_is_y = lane < m;
        SwPoint P{0.0, 0.0}, Q{0.0, 0.0};
        if (has) {
            const double* src = p_is_x ? A.X + 2 * (x0 + lane) : A.Y + 2 * (y0 + lane - n);
            P.b = src[0]; P.d = src[1];
            const double* sq = q_is_y ? A.Y + 2 * (y0 + lane) : A.X + 2 * (x0 + lane - m);
            Q.b = sq[0]; Q.d = sq[1];
        }
        if (__any(!(sw_finite(P.b) && sw_finite(P.d)))) {          // (every point is some lane's P)
            if (lane == 0) { A.status[p] = 3; A.loss[p] = sw_nan(); }
            if (has) {
                double* g = p_is_x ? (A.gradX ? A.gradX + 2 * (x0 + lane) : nullptr) : (A.gradY ? A.gradY + 2 * (y0 + lane - n) : nullptr);
                if (g) { g[0] = 0.0; g[1] = 0.0; }
            }
            continue;
        }
        const double sg = sw_sign(P.b + P.d);
        const int other = has ? sw_other(lane, n, m) : lane;
        double g0 = 0.0, g1 = 0.0, loss = 0.0;
        for (int i = 0; i < A.n_dirs; ++i) {
            const double l0 = A.dirs[2 * i], l1 = A.dirs[2 * i + 1];
            unsigned long long k1 = ~0ull, k2 = ~0ull;
            unsigned i1 = (unsigned)lane, i2 = (unsigned)lane;
            if (has) {
                k1 = tlc_ord_f64(p_is_x ? P.proj(l0, l1) : P.diag(l0, l1));
                k2 = tlc_ord_f64(q_is_y ? Q.proj(l0, l1) : Q.diag(l0, l1));
            }
            sw_wave_sort2(k1, i1, k2, i2, lane);
            // lane = rank now; the absent elements (index >= N, key ~0 or not: the index breaks the tie) fill the ranks N .. 63
            const double diff = has ? sw_val(k1) - sw_val(k2) : 0.0;
            const int s = diff > 0.0 ? 1 : (diff < 0.0 ? -1 : 0);
            loss += A.scale * sw_wave_sum(fabs(diff));
            const int sa = __builtin_amdgcn_ds_permute((int)(i1 << 2), s);      // to the lane of the listing index: i1 / i2 are
            const int sb = __builtin_amdgcn_ds_permute((int)(i2 << 2), s);      // permutations of 0 .. 63
            const int sbo = __shfl(sb, other);
            const double t0 = A.scale * l0, t1 = A.scale * l1, u = A.scale * ((l0 + l1) * 0.5);
            sw_step(g0, g1, p_is_x, (double)sa, (double)sbo, sg, t0, t1, u);
        }
        if (lane == 0) { A.status[p] = 0; A.loss[p] = loss; }
        if (has) {
            double* g = p_is_x ? (A.gradX ? A.gradX + 2 * (x0 + lane) : nullptr) : (A.gradY ? A.gradY + 2 * (y0 + lane - n) : nullptr);
            if (g) { g[0] = g0; g[1] = g1; }
        }
    }
}

// ---- 65 .. TLC_SW_LDS_NMAX points: one workgroup per problem --------------------------------------------------------------------
// the block's sum of v: butterfly inside a wavefront, then the wavefronts ascending (every thread returns the same bits)
__device__ __forceinline__ double sw_block_sum(double v, double* red) {
    v = sw_wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < SW_WAVES; ++w) s += red[w];
    return s;
}

__global__ __launch_bounds__(SW_BS) void sw_lds_kernel(SwArgs A) {
    __shared__ unsigned long long key1[SW_LDS_N], key2[SW_LDS_N];
    __shared__ unsigned short idx1[SW_LDS_N], idx2[SW_LDS_N];
    __shared__ signed char sgA[SW_LDS_N], sgB[SW_LDS_N];
    __shared__ double red[2][SW_WAVES];
    const int tid = (int)threadIdx.x;
    for (long long p = blockIdx.x; p < A.n_problems; p += gridDim.x) {
        const long long x0 = A.xoff[p], y0 = A.yoff[p];
        const long long nn = A.xoff[p + 1] - x0, mm = A.yoff[p + 1] - y0;
        if (nn + mm <= SW_WAVE_N || nn + mm > SW_LDS_N) continue;           // uniform over the workgroup
        const int n = (int)nn, m = (int)mm, N = n + m;
        int P2 = 128;
        while (P2 < N) P2 <<= 1;
        SwPoint pt[SW_PER_THREAD];
        double g0[SW_PER_THREAD], g1[SW_PER_THREAD];
        bool bad = false;
#pragma unroll
        for (int q = 0; q < SW_PER_THREAD; ++q) {
            const int a = tid + q * SW_BS;
            pt[q].b = 0.0; pt[q].d = 0.0;
            g0[q] = 0.0; g1[q] = 0.0;
            if (a < N) {
                const double* src = a < n ? A.X + 2 * (x0 + a) : A.Y + 2 * (y0 + a - n);
                pt[q].b = src[0]; pt[q].d = src[1];
                bad |= !(sw_finite(pt[q].b) && sw_finite(pt[q].d));
            }
        }
        if (__syncthreads_or(bad)) {
            if (tid == 0) { A.status[p] = 3; A.loss[p] = sw_nan(); }
#pragma unroll
            for (int q = 0; q < SW_PER_THREAD; ++q) {
                const int a = tid + q * SW_BS;
                if (a < N) {
                    double* g = a < n ? (A.gradX ? A.gradX + 2 * (x0 + a) : nullptr) : (A.gradY ? A.gradY + 2 * (y0 + a - n) : nullptr);
                    if (g) { g[0] = 0.0; g[1] = 0.0; }
                }
            }
            continue;
        }
        double loss = 0.0;
        for (int i = 0; i < A.n_dirs; ++i) {
            const double l0 = A.dirs[2 * i], l1 = A.dirs[2 * i + 1];
            // a point writes its element of V1 and its element of V2; the tail up to the power of two sorts behind (index >= N)
#pragma unroll
            for (int q = 0; q < SW_PER_THREAD; ++q) {
                const int a = tid + q * SW_BS;
                if (a < N) {
                    const bool is_x = a < n;
                    const int o = sw_other(a, n, m);
                    const double pr = pt[q].proj(l0, l1), dg = pt[q].diag(l0, l1);
                    key1[a] = tlc_ord_f64(is_x ? pr : dg); idx1[a] = (unsigned short)a;
                    key2[o] = tlc_ord_f64(is_x ? dg : pr); idx2[o] = (unsigned short)o;
                } else if (a < P2) {
                    key1[a] = ~0ull; idx1[a] = (unsigned short)a;
                    key2[a] = ~0ull; idx2[a] = (unsigned short)a;
                }
            }
            __syncthreads();
            for (int k = 2; k <= P2; k <<= 1)
                for (int j = k >> 1; j > 0; j >>= 1) {
                    for (int t = tid; t < (P2 >> 1); t += SW_BS) {
                        const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                        const bool asc = (lo & k) == 0;
                        {
                            const unsigned long long ka = key1[lo], kb = key1[hi];
                            const unsigned short va = idx1[lo], vb = idx1[hi];
                            if ((ka > kb || (ka == kb && va > vb)) == asc) { key1[lo] = kb; key1[hi] = ka; idx1[lo] = vb; idx1[hi] = va; }
                        }
                        {
                            const unsigned long long ka = key2[lo], kb = key2[hi];
                            const unsigned short va = idx2[lo], vb = idx2[hi];
                            if ((ka > kb || (ka == kb && va > vb)) == asc) { key2[lo] = kb; key2[hi] = ka; idx2[lo] = vb; idx2[hi] = va; }
                        }
                    }
                    __syncthreads();
                }
            double part = 0.0;
#pragma unroll
            for (int q = 0; q < SW_PER_THREAD; ++q) {
                const int k = tid + q * SW_BS;
                if (k < N) {
                    const double diff = sw_val(key1[k]) - sw_val(key2[k]);
                    const signed char s = diff > 0.0 ? 1 : (diff < 0.0 ? -1 : 0);
                    sgA[idx1[k]] = s;            // (the ranks below N hold the indices below N: the tail sorts behind)
                    sgB[idx2[k]] = s;
                    part += fabs(diff);
                }
            }
            loss += A.scale * sw_block_sum(part, red[i & 1]);                  // (its barrier also publishes sgA / sgB)
            const double t0 = A.scale * l0, t1 = A.scale * l1, u = A.scale * ((l0 + l1) * 0.5);
#pragma unroll
            for (int q = 0; q < SW_PER_THREAD; ++q) {
                const int a = tid + q * SW_BS;
                if (a < N)
                    sw_step(g0[q], g1[q], a < n, (double)sgA[a], (double)sgB[sw_other(a, n, m)], sw_sign(pt[q].b + pt[q].d), t0, t1, u);
            }
            __syncthreads();                                                   // the lists and the signs are the next direction's
        }
        if (tid == 0) { A.status[p] = 0; A.loss[p] = loss; }
#pragma unroll
        for (int q = 0; q < SW_PER_THREAD; ++q) {
            const int a = tid + q * SW_BS;
            if (a < N) {
                double* g = a < n ? (A.gradX ? A.gradX + 2 * (x0 + a) : nullptr) : (A.gradY ? A.gradY + 2 * (y0 + a - n) : nullptr);
                if (g) { g[0] = g0[q]; g[1] = g1[q]; }
            }
        }
    }
}

// ---- above TLC_SW_LDS_NMAX points: the whole device, one problem at a time -----------------------------------------------------------
// One group = the directions d0 .. d0 + G - 1.  Segment s = 2 * g + list (g the direction inside the group) holds N items; before the
// sort item (s, position) sits at s * N + position, after it rank k of segment s does.
struct SwCtl {
    int status;
    int pad;
    double loss;
};
struct SwWide {
    long long x0, y0;
    int n, m;
    const double *X, *Y, *dirs;
    double scale;
    SwCtl* ctl;
};
__device__ __forceinline__ SwPoint sw_wide_point(const SwWide& W, long long a) {
    const double* src = a < W.n ? W.X + 2 * (W.x0 + a) : W.Y + 2 * (W.y0 + a - W.n);
    return SwPoint{src[0], src[1]};
}
#define SW_FOR(i, count) \
    for (long long i = (long long)blockIdx.x * SW_BS + threadIdx.x; i < (count); i += (long long)gridDim.x * SW_BS)

// status of the problem: 3 where a coordinate is NaN / Inf (the control block was zeroed before; an integer OR, so no order matters)
__global__ __launch_bounds__(SW_BS) void sww_begin_kernel(SwWide W) {
    const long long N = (long long)W.n + W.m;
    bool bad = false;
    SW_FOR(a, N) {
        const SwPoint P = sw_wide_point(W, a);
        bad |= !(sw_finite(P.b) && sw_finite(P.d));
    }
    if (__syncthreads_or(bad) && threadIdx.x == 0) atomicOr(&W.ctl->status, 3);
}
__global__ __launch_bounds__(SW_BS) void sww_keys_kernel(SwWide W, int d0, int G, unsigned long long* __restrict__ key,
                                                         unsigned long long* __restrict__ pay) {
    const long long N = (long long)W.n + W.m;
    SW_FOR(a, N) {
        const SwPoint P = sw_wide_point(W, a);
        const bool is_x = a < W.n;
        const long long o = is_x ? W.m + a : a - W.n;
        for (int g = 0; g < G; ++g) {
            const double l0 = W.dirs[2 * (d0 + g)], l1 = W.dirs[2 * (d0 + g) + 1];
            const double pr = P.proj(l0, l1), dg = P.diag(l0, l1);
            const long long s1 = 2 * g, s2 = 2 * g + 1;
            key[s1 * N + a] = tlc_ord_f64(is_x ? pr : dg);
            pay[s1 * N + a] = ((unsigned long long)s1 << 32) | (unsigned long long)a;
            key[s2 * N + o] = tlc_ord_f64(is_x ? dg : pr);
            pay[s2 * N + o] = ((unsigned long long)s2 << 32) | (unsigned long long)o;
        }
    }
}
// tile (blockIdx.x) of the ranks of direction g (blockIdx.y): the sign bytes to [segment][listing position], the tile's sum of |difference|
__global__ __launch_bounds__(SW_BS) void sww_signs_kernel(long long N, int n_tiles, const unsigned long long* __restrict__ key,
                                                          const unsigned long long* __restrict__ pay, signed char* __restrict__ signs,
                                                          double* __restrict__ partial) {
    __shared__ double red[SW_WAVES];
    const int g = (int)blockIdx.y;
    const long long s1 = 2ll * g * N, s2 = s1 + N;
    double part = 0.0;
#pragma unroll
    for (int q = 0; q < SW_TILE / SW_BS; ++q) {
        const long long k = (long long)blockIdx.x * SW_TILE + q * SW_BS + threadIdx.x;
        if (k < N) {
            const double diff = sw_val(key[s1 + k]) - sw_val(key[s2 + k]);
            const signed char s = diff > 0.0 ? 1 : (diff < 0.0 ? -1 : 0);
            signs[s1 + (long long)(unsigned)pay[s1 + k]] = s;
            signs[s2 + (long long)(unsigned)pay[s2 + k]] = s;
            part += fabs(diff);
        }
    }
    const double sum = sw_block_sum(part, red);
    if (threadIdx.x == 0) partial[(long long)g * n_tiles + blockIdx.x] = sum;
}
// one workgroup: thread g sums the tiles of direction g ascending, thread 0 adds scale * sum of the directions ascending to the
// accumulator; after the last group the problem's loss and status
__global__ __launch_bounds__(TLC_SW_MAX_DIRS) void sww_loss_kernel(SwCtl* ctl, int G, int n_tiles, const double* __restrict__ partial,
                                                                   double scale, int last, double* loss, unsigned char* status) {
    __shared__ double r[TLC_SW_MAX_DIRS];
    const int g = (int)threadIdx.x;
    if (g < G) {
        double s = 0.0;
        for (int t = 0; t < n_tiles; ++t) s += partial[(long long)g * n_tiles + t];
        r[g] = s;
    }
    __syncthreads();
    if (g == 0) {
        double acc = ctl->loss;
        for (int k = 0; k < G; ++k) acc += scale * r[k];
        ctl->loss = acc;
        if (last) {
            *status = (unsigned char)ctl->status;
            *loss = ctl->status ? sw_nan() : acc;
        }
    }
}
// the point at position a of V1 continues its sum over the group's directions (from +0.0 in the first group)
__global__ __launch_bounds__(SW_BS) void sww_grad_kernel(SwWide W, int d0, int G, const signed char* __restrict__ signs, double* gradX,
                                                         double* gradY) {
    const long long N = (long long)W.n + W.m;
    const bool failed = W.ctl->status != 0;
    SW_FOR(a, N) {
        const bool is_x = a < W.n;
        double* out = is_x ? (gradX ? gradX + 2 * (W.x0 + a) : nullptr) : (gradY ? gradY + 2 * (W.y0 + a - W.n) : nullptr);
        if (!out) continue;
        if (failed) { out[0] = 0.0; out[1] = 0.0; continue; }
        const SwPoint P = sw_wide_point(W, a);
        const double sg = sw_sign(P.b + P.d);
        const long long o = is_x ? W.m + a : a - W.n;
        double g0 = d0 ? out[0] : 0.0, g1 = d0 ? out[1] : 0.0;
        for (int g = 0; g < G; ++g) {
            const double l0 = W.dirs[2 * (d0 + g)], l1 = W.dirs[2 * (d0 + g) + 1];
            const double t0 = W.scale * l0, t1 = W.scale * l1, u = W.scale * ((l0 + l1) * 0.5);
            sw_step(g0, g1, is_x, (double)signs[2ll * g * N + a], (double)signs[(2ll * g + 1) * N + o], sg, t0, t1, u);
        }
        out[0] = g0; out[1] = g1;
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------
struct SwLay {
    size_t ctl, key_a, key_b, pay_a, pay_b, signs, hist, tot, partial, bytes;
};
// workspace of a group of G directions with T = 2 * G * N items: a function of (T, G) alone, growing in both
SwLay sw_layout(long long T, int G) {
    SwLay L;
    TlcCarver W;
    L.ctl = W.take(1, sizeof(SwCtl));
    L.key_a = W.take(T, 8); L.key_b = W.take(T, 8);
    L.pay_a = W.take(T, 8); L.pay_b = W.take(T, 8);
    L.signs = W.take(T, 1);
    L.hist = W.take(rk_hist_ints(T), 4); L.tot = W.take(RK_TOT_INTS, 4);
    L.partial = W.take(T / (2 * SW_TILE) + G + 1, 8);        // >= G * ceil(N / SW_TILE)
    L.bytes = W.bytes();
    return L;
}
// the size that runs n_dirs directions of a problem of N points at once (as many as fit SW_WIDE_MAX_ITEMS)
long long sw_work_need(long long N, int n_dirs) {
    if (N <= SW_LDS_N) return 0;
    if (N > SW_WIDE_MAX_ITEMS) N = SW_WIDE_MAX_ITEMS;
    long long T = 2 * N * n_dirs;
    if (T > 2 * SW_WIDE_MAX_ITEMS) T = 2 * SW_WIDE_MAX_ITEMS;
    return (long long)sw_layout(T, n_dirs).bytes;
}
unsigned sw_grid(long long count) { return tlc_grid_for(count, SW_BS, SW_MAX_GRID); }

// One problem of the third class: 1 + groups x 31 kernel launches (the coordinate check; per group of directions the keys, 9 radix
// passes of 3 kernels, the signs, the loss and -- where a gradient is wanted -- the point sums).
int sw_run_wide(const SwArgs& A, long long p, long long x0, long long y0, long long n, long long m, char* w, int64_t work_bytes, hipStream_t st) {
    const long long N = n + m;
    int G = 1;                                               // (the entry checked that one direction fits)
    while (G < A.n_dirs && (long long)(G + 1) * N <= SW_WIDE_MAX_ITEMS && (int64_t)sw_layout(2 * N * (G + 1), G + 1).bytes <= work_bytes) ++G;
    const int n_tiles = (int)((N + SW_TILE - 1) / SW_TILE);
    SwWide W{x0, y0, (int)n, (int)m, A.X, A.Y, A.dirs, A.scale, nullptr};
    for (int d0 = 0; d0 < A.n_dirs; d0 += G) {
        const int Gc = A.n_dirs - d0 < G ? A.n_dirs - d0 : G;
        const long long T = 2 * N * Gc;
        const SwLay L = sw_layout(2 * N * G, G);             // one layout for every group of the problem
        W.ctl = (SwCtl*)(w + L.ctl);
        unsigned long long *ka = (unsigned long long*)(w + L.key_a), *kb = (unsigned long long*)(w + L.key_b);
        unsigned long long *pa = (unsigned long long*)(w + L.pay_a), *pb = (unsigned long long*)(w + L.pay_b);
        signed char* signs = (signed char*)(w + L.signs);
        int *hist = (int*)(w + L.hist), *tot = (int*)(w + L.tot);
        double* partial = (double*)(w + L.partial);
        if (d0 == 0) {
            if (hipMemsetAsync(W.ctl, 0, sizeof(SwCtl), st) != hipSuccess) return TLC_ERR_HIP;       // status 0, loss +0.0
            hipLaunchKernelGGL(sww_begin_kernel, dim3(sw_grid(N)), dim3(SW_BS), 0, st, W);
        }
        hipLaunchKernelGGL(sww_keys_kernel, dim3(sw_grid(N)), dim3(SW_BS), 0, st, W, d0, Gc, ka, pa);
        rk_sort<64>(st, T, ka, kb, pa, pb, hist, tot);       // the values, stable (T >= 2: the class starts above SW_LDS_N points)
        // the leading digit: the segment number, bits 32 .. 39 of the payload -- the payload is this pass's key
        rk_pass(st, T, 32, pa, ka, pb, kb, hist, tot);
        hipLaunchKernelGGL(sww_signs_kernel, dim3((unsigned)n_tiles, (unsigned)Gc), dim3(SW_BS), 0, st, N, n_tiles, kb, pb, signs, partial);
        hipLaunchKernelGGL(sww_loss_kernel, dim3(1), dim3(TLC_SW_MAX_DIRS), 0, st, W.ctl, Gc, n_tiles, partial, A.scale,
                           (int)(d0 + Gc == A.n_dirs), A.loss + p, A.status + p);
        if (A.gradX || A.gradY)
            hipLaunchKernelGGL(sww_grad_kernel, dim3(sw_grid(N)), dim3(SW_BS), 0, st, W, d0, Gc, signs, A.gradX, A.gradY);
    }
    return TLC_OK;
}

}  // namespace

extern "C" int64_t tlc_sliced_w_work_bytes(int32_t n_problems, int64_t total_points, int64_t max_points, int32_t n_dirs) {
    if (n_problems < 0 || total_points < 0 || max_points < 0 || n_dirs < 1 || n_dirs > TLC_SW_MAX_DIRS) {
        tlc_set_error("%s: negative size or n_dirs outside 1 .. %d", __func__, TLC_SW_MAX_DIRS);
        return -1;
    }
    return sw_work_need(max_points, n_dirs);
}

extern "C" int tlc_sliced_wasserstein(int32_t n_problems, const int64_t* d_xoff, const double* d_X, const int64_t* d_yoff, const double* d_Y,
                                      int32_t n_dirs, const double* d_dirs, double scale, int64_t max_points, double* d_loss,
                                      double* d_gradX, double* d_gradY, uint8_t* d_status, void* d_work, int64_t work_bytes, void* stream) {
    TLC_REQUIRE(n_problems >= 0 && max_points >= 0 && work_bytes >= 0, "negative size");
    TLC_REQUIRE(n_dirs >= 1 && n_dirs <= TLC_SW_MAX_DIRS, "n_dirs outside 1 .. TLC_SW_MAX_DIRS");
    if (n_problems == 0) return TLC_OK;
    TLC_REQUIRE(d_xoff && d_yoff && d_dirs && d_loss && d_status, "null pointer");
    TLC_REQUIRE(max_points == 0 || d_X || d_Y, "null pointer");
    const long long least = sw_work_need(max_points, 1);
    if (work_bytes < least || (least > 0 && !d_work)) {
        if (!d_work && work_bytes >= least) tlc_set_error("%s: null pointer", __func__);
        else tlc_set_error("%s: d_work holds %lld bytes; a problem of %lld points needs %lld for one direction (tlc_sliced_w_work_bytes)",
                           __func__, (long long)work_bytes, (long long)max_points, least);
        return TLC_ERR_INVALID_ARG;
    }
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
    long long n_wave = 0, n_lds = 0, n_wide = 0;
    if (xo[0] < 0 || yo[0] < 0) { tlc_set_error("%s: negative offset", __func__); return TLC_ERR_INVALID_ARG; }
    for (size_t p = 0; p < B; ++p) {
        const long long n = xo[p + 1] - xo[p], m = yo[p + 1] - yo[p];
        if (n < 0 || m < 0) { tlc_set_error("%s: the offsets of problem %lld decrease", __func__, (long long)p); return TLC_ERR_INVALID_ARG; }
        if (n + m > max_points) {
            tlc_set_error("%s: problem %lld has %lld points, max_points is %lld", __func__, (long long)p, n + m, (long long)max_points);
            return TLC_ERR_INVALID_ARG;
        }
        if (n + m > SW_WIDE_MAX_ITEMS) { tlc_set_error("%s: problem %lld has more than 2^27 points", __func__, (long long)p); return TLC_ERR_UNSUPPORTED; }
        if (n + m <= SW_WAVE_N) ++n_wave;
        else if (n + m <= SW_LDS_N) ++n_lds;
        else ++n_wide;
    }
    SwArgs A{n_problems, (const long long*)d_xoff, (const long long*)d_yoff, d_X, d_Y, n_dirs, d_dirs, scale, d_loss, d_gradX, d_gradY, d_status};
    if (n_wave) hipLaunchKernelGGL(sw_wave_kernel, dim3(sw_grid((long long)n_problems * 64)), dim3(SW_BS), 0, st, A);
    if (n_lds) hipLaunchKernelGGL(sw_lds_kernel, dim3((unsigned)(n_problems < SW_MAX_GRID ? n_problems : SW_MAX_GRID)), dim3(SW_BS), 0, st, A);
    if (n_wide) {
        char* w = tlc_align256(d_work);
        for (size_t p = 0; p < B; ++p) {
            const long long n = xo[p + 1] - xo[p], m = yo[p + 1] - yo[p];
            if (n + m > SW_LDS_N && sw_run_wide(A, (long long)p, xo[p], yo[p], n, m, w, work_bytes, st) != TLC_OK) {
                tlc_set_error("%s: clearing the control block failed: %s", __func__, hipGetErrorString(hipGetLastError()));
                return TLC_ERR_HIP;
            }
        }
    }
    TLC_HIP_CHECK(hipGetLastError());
    return TLC_OK;
}

// w2_match.hip -- the diagram loss of PDGNN training: partial-matching Wasserstein distance between a predicted and a target
// persistence diagram.
//
// Replaces Knowledge_Distillation/wasserstein.py:198-379 (`wasserstein_distance(X, Y, order=p, enable_autodiff=True,
// num_models=1)`, called from Teacher_model.py:107-139 `compute_PD_loss(kernel='wasserstein')`): the reference builds the
// cost matrix  C[i, j] = ||X_i - Y_j||_inf ^ p,  C[i, m] = ((X_i.y - X_i.x) / 2) ^ p  (:45-67), gives every predicted point
// mass 1, every target point mass 1 and the diagonal mass n - m (:262-264), solves the transport with POT's `ot.emd`
// (third-party, absent here), and sums the matched distances:  loss = (sum_k |d_k|^p)^(1/p)  over the X-Y pairs and the
// points sent to the diagonal (:303-372; with num_models = 1 every diagonal point is kept, :329-337).
//
// With unit masses the transport is an ASSIGNMENT: n rows (predicted points) onto m target columns plus n - m copies of the
// diagonal.  w2_solve<T, CPL, INFER> solves one problem on T threads with the shortest-augmenting-path (Hungarian) method,
// threads = columns: the cost of (row, column) is recomputed from the two points (no matrix is stored), column duals / slack in
// registers, row duals, the column -> row map and the alternating-path links in LDS; O(n^2) steps of ~60 instructions.  Two thin
// kernels call it: a wavefront per problem up to 512 rows (T = 64, CPL = 1 / 2 / 4 / 8 by the batch's largest problem; no barrier
// at all) and a 512-thread workgroup per problem for 513 .. 4 096 rows (T = 512, CPL = 8; two barriers per step, ~1.5 us per step
// -- a 2 000-point problem takes a few hundred thousand steps at worst).  The two size classes differ in three compile-time
// properties of w2_solve, and in nothing else: the wavefront starts with a column reduction, keeps the rows' diagonal costs in
// LDS (the workgroup has no LDS left for them and recomputes the same bits), and breaks ties among equal minima by lane
// (w2_select states both rules).
// Also returned: which target every predicted point went to, the two partial sums the reference logs (wxy, wxd) and the
// gradient of the loss with respect to the predicted points (what `loss.backward()` would put on PD-hat).  The cost of a pair,
// the outputs of an unsolved problem and the loss and gradient of a finished matching are w2_common.h's, shared with the
// workspace tier above 4 096 rows (w2_large.hip).
//
// Evaluation (INFER = true): `wasserstein_distance_inference` (wasserstein.py:93-195, called with pair_diagonal=True from
// train_Teacher_Model.py:99 -> Teacher_model.py:66,134-136) is the classic transport in which BOTH diagrams may use the
// diagonal: masses a = [1]*n + [m], b = [1]*m + [n], cost matrix (n+1) x (m+1) with C[n, j] = ((Y_j.y - Y_j.x) / 2) ^ p and
// C[n, m] = 0 (:45-67,127-131).  With integer masses that is the assignment of n + m rows (the predicted points, then m copies
// of the diagonal) onto n + m columns (the targets, then n copies of the diagonal): same kernels, matrix dimension N = n + m,
// a third partial sum (wyd, the targets sent to the diagonal, :170-176) and the target -> predicted map beside the other one.
// Empty diagrams: the total persistence of the other one and zero partial sums (:98-113).
//
// PARITY UNPINNED: `ot.emd` is not available; the optimal COST is unique and is checked against
// scipy.optimize.linear_sum_assignment (tests/test_gpu_train.py); among several optimal assignments
// (ties) `ot.emd` may pick another one than this kernel.
#include "w2_common.h"

namespace {

struct W2Params : W2Problem {
    int n_pairs;
    int leave_big;             // the wavefront kernel leaves problems beyond its capacity alone (the workgroup kernel takes them)
};

constexpr int W2_WIDE_THREADS = 512, W2_WIDE_CPL = 8, W2_NONE = 0x7fffffff;
static_assert(W2_WIDE_THREADS * W2_WIDE_CPL == TLC_W2_LDS_NMAX, "the workgroup's columns");

template <int T>
__device__ __forceinline__ void w2_sync() {
    if (T == 64) { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); }
    else __syncthreads();
}

// The LDS of one problem of up to T * CPL rows on T threads
template <int T, int CPL>
struct W2Lds {
    static constexpr int NMAX = T * CPL, NWV = T / 64;
    static constexpr bool WAVE = T == 64;
    static constexpr size_t BYTES = (size_t)NMAX * (3 * 8 + 2 * 4) + (size_t)(WAVE ? NMAX : NWV) * (8 + 4);
    double* xs;                // [NMAX] predicted births (0 for the diagonal rows)
    double* ys;                // [NMAX] predicted deaths
    double* u;                 // [NMAX] row duals
    double* cxd;               // WAVE: [NMAX] cost of the diagonal for row i
    double* red;               // !WAVE: [NWV] a value per wavefront (a wavefront alone reduces in registers)
    int* pcol;                 // [NMAX] row assigned to column j, -1 = free
    int* way;                  // [NMAX] previous column on the alternating path, -1 = the start
    int* rdone;                // WAVE: [NMAX] row already assigned by the column reduction
    int* redj;                 // !WAVE: [NWV] a column per wavefront
    __device__ explicit W2Lds(unsigned char* base) {
        xs = (double*)base; ys = xs + NMAX; u = ys + NMAX;
        cxd = red = u + NMAX;
        pcol = (int*)(red + (WAVE ? NMAX : NWV)); way = pcol + NMAX;
        rdone = redj = way + NMAX;
    }
};

// A step's minimum over the T threads and the column that takes it; false: no thread has a candidate (bj < 0 everywhere).  best / bj:
// the thread's least value and the lowest of its own columns that holds it.  Which of several columns at the minimum is taken decides
// which optimal matching a tied problem returns, and the two size classes have each their rule:
//   T = 64, in registers: the lowest LANE that holds the minimum, then that lane's bj.  For CPL > 1 that is not the lowest column
//       (lane 0's column 64 goes before lane 1's column 1).
//   T > 64, one barrier:  the lowest column of each wavefront, then the least (value, column) over the wavefronts ascending: the
//       lowest column of the workgroup.
template <int T>
__device__ __forceinline__ bool w2_select(double best, int bj, double& delta, int& j1, double* red, int* redj) {
    const double wmin = tlc_wave_min_f64(best);
    const bool mine = best == wmin && bj >= 0;
    if (T == 64) {
        const unsigned long long who = __ballot(mine);
        if (who == 0ull) return false;                        // (never index with lane 64)
        delta = wmin; j1 = __builtin_amdgcn_readlane(bj, __builtin_ctzll(who));
        return true;
    }
    const int cand = tlc_wave_min_i32(mine ? bj : W2_NONE);
    if (tlc_lane() == 0) { red[threadIdx.x >> 6] = wmin; redj[threadIdx.x >> 6] = cand; }
    __syncthreads();
    delta = red[0]; j1 = redj[0];
#pragma unroll
    for (int k = 1; k < T / 64; ++k) {
        const double d = red[k];
        const int jj = redj[k];
        if (d < delta || (d == delta && jj < j1)) { delta = d; j1 = jj; }
    }
    return j1 != W2_NONE;
}

// One problem of N <= T * CPL rows (N = n, INFER: n + m) on T threads; column j belongs to thread j % T (register slot j / T).
template <int T, int CPL, bool INFER>
__device__ __forceinline__ void w2_solve(const W2Params& p, int b, long long x0, long long y0, int n, int m, const W2Lds<T, CPL>& lds) {
    constexpr bool WAVE = T == 64;
    double* const xs = lds.xs; double* const ys = lds.ys; double* const u = lds.u;
    int* const pcol = lds.pcol; int* const way = lds.way;
    const int tid = (int)threadIdx.x, N = INFER ? n + m : n;
    const double INF = __longlong_as_double(0x7FF0000000000000ll);
    const double QNAN = __longlong_as_double(0x7FF8000000000000ll);
    bool finite = true;
    for (int i = tid; i < N; i += T) {
        double bx = 0.0, by = 0.0;
        if (i < n) { bx = p.X[2 * (x0 + i)]; by = p.X[2 * (x0 + i) + 1]; }
        finite = finite && w2_finite(bx, by);
        xs[i] = bx; ys[i] = by;
        if (WAVE) lds.cxd[i] = w2_pow((by - bx) * 0.5, p.order);
        u[i] = 0.0; pcol[i] = -1;
    }
    double yx[CPL], yy[CPL], cdy[CPL], v[CPL], minv[CPL];
    bool used[CPL];
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
        const int j = tid + T * c;
        yx[c] = yy[c] = 0.0;
        if (j < m) { yx[c] = p.Y[2 * (y0 + j)]; yy[c] = p.Y[2 * (y0 + j) + 1]; }
        finite = finite && w2_finite(yx[c], yy[c]);
        cdy[c] = w2_pow((yy[c] - yx[c]) * 0.5, p.order);
        v[c] = 0.0;
    }
    // NaN / Inf coordinates (a diverging training step): the augmenting loop would not end.  (T > 64: the threads that saw one, counted)
    if (WAVE ? __ballot(!finite) != 0ull : w2_block_sum<T>(finite ? 0.0 : 1.0, lds.red) != 0.0) {
        w2_fail<INFER, T>(p, b, x0, y0, n, m, 3, QNAN, tid);
        return;
    }
    w2_sync<T>();
    // the cost of (row, column slot c) from the two points; the row's values are uniform
    auto cost_of = [&](bool row_real, double xi, double yi, double cd, int j, int c) -> double {
        return w2_cost<INFER>(row_real, xi, yi, cd, j < m, yx[c], yy[c], cdy[c], p.order);
    };
    if constexpr (WAVE) {
        // ---- column reduction (the usual start of the shortest-augmenting-path method): v_j = min_i c_ij, and a row that is the
        // minimiser of some column takes the lowest such column -- duals feasible (u = 0), every such pair tight; on random
        // diagrams this assigns ~60 % of the rows before the first augmentation.  (The workgroup kernel starts from v = 0.)
        int rj[CPL];
#pragma unroll
        for (int c = 0; c < CPL; ++c) { v[c] = INF; rj[c] = 0; }
        // (unrolled by the row only where a row is one column of work: unrolled further, or at all for CPL > 1, the loop costs occupancy)
        constexpr int ROWS_AT_ONCE = CPL == 1 ? 4 : 1;
#pragma unroll ROWS_AT_ONCE
        for (int i = 0; i < N; ++i) {
            const double xi = xs[i], yi = ys[i], cd = lds.cxd[i];
#pragma unroll
            for (int c = 0; c < CPL; ++c) {
                const double cost = cost_of(i < n, xi, yi, cd, tid + T * c, c);
                if (cost < v[c]) { v[c] = cost; rj[c] = i; }
            }
        }
        for (int i = tid; i < N; i += T) way[i] = W2_NONE;
        w2_sync<T>();
#pragma unroll
        for (int c = 0; c < CPL; ++c) { const int j = tid + T * c; if (j < N) atomicMin(&way[rj[c]], j); else v[c] = 0.0; }
        w2_sync<T>();
#pragma unroll
        for (int c = 0; c < CPL; ++c) { const int j = tid + T * c; if (j < N && way[rj[c]] == j) pcol[j] = rj[c]; }
        for (int i = tid; i < N; i += T) lds.rdone[i] = way[i] != W2_NONE;
        w2_sync<T>();
    }
    // ---- an augmenting path from every row that is still free ---------------------------------------------------------------------
    bool failed = false;
    for (int i = 0; i < N && !failed; ++i) {
        if (WAVE && lds.rdone[i]) continue;                   // (uniform: LDS)
#pragma unroll
        for (int c = 0; c < CPL; ++c) { minv[c] = INF; used[c] = false; }
        int i0 = i, j0 = -1;
        for (;;) {
            const double xi = xs[i0], yi = ys[i0], ui = u[i0];
            const double cd = WAVE ? lds.cxd[i0] : w2_pow((yi - xi) * 0.5, p.order);
            double best = INF;
            int bj = -1;
#pragma unroll
            for (int c = 0; c < CPL; ++c) {
                const int j = tid + T * c;
                if (j < N && !used[c]) {
                    const double cur = cost_of(i0 < n, xi, yi, cd, j, c) - ui - v[c];
                    if (cur < minv[c]) { minv[c] = cur; way[j] = j0; }
                    if (minv[c] < best) { best = minv[c]; bj = j; }
                }
            }
            double delta = 0.0;
            int j1 = -1;
            if (!w2_select<T>(best, bj, delta, j1, lds.red, lds.redj)) { failed = true; break; }     // (uniform; cannot happen with finite inputs)
            // dual update: rows of the used columns and the row that started the path go up, used columns go down,
            // the slack of the others shrinks
#pragma unroll
            for (int c = 0; c < CPL; ++c) {
                const int j = tid + T * c;
                if (j < N) {
                    if (used[c]) { u[pcol[j]] += delta; v[c] -= delta; }
                    else minv[c] -= delta;
                }
            }
            if (tid == 0) u[i] += delta;
            j0 = j1;
#pragma unroll
            for (int c = 0; c < CPL; ++c) if (tid + T * c == j1) used[c] = true;
            w2_sync<T>();
            i0 = pcol[j1];
            if (i0 < 0) break;
        }
        if (failed) break;
        // augment along the alternating path (one thread: at most N links)
        if (tid == 0) {
            int j = j0;
            while (j >= 0) {
                const int jp = way[j];
                pcol[j] = jp < 0 ? i : pcol[jp];
                j = jp;
            }
        }
        w2_sync<T>();
    }
    if (failed) { w2_sync<T>(); w2_fail<INFER, T>(p, b, x0, y0, n, m, 3, QNAN, tid); return; }
    // ---- the loss, its parts and the maps, then d loss / d X, from the finished matching: a thread's own columns ----------------------
    W2Sums sums;
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
        const int j = tid + T * c;
        if (j < N) {
            const int i = pcol[j];
            sums = w2_pair_loss<INFER>(p, x0, y0, n, m, i, j, xs[i], ys[i], yx[c], yy[c], sums);
        }
    }
    const double L = w2_finish<INFER, T>(p, b, sums, lds.red, tid);
    if (p.gradX) {
#pragma unroll
        for (int c = 0; c < CPL; ++c) {
            const int j = tid + T * c;
            if (j < N) {
                const int i = pcol[j];
                if (i >= n) continue;
                double gx, gy;
                w2_pair_grad(p.order, L, j < m, xs[i], ys[i], yx[c], yy[c], gx, gy);
                p.gradX[2 * (x0 + i)] = gx;
                p.gradX[2 * (x0 + i) + 1] = gy;
            }
        }
    }
}

// N <= 64 CPL: a wavefront per problem, the problems by the grid's stride
template <int CPL, bool INFER>
__global__ __launch_bounds__(64) void tlc_w2_match_kernel(W2Params p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char w2_lds[];
    const W2Lds<64, CPL> lds(w2_lds);
    const int lane = tlc_lane();
    for (int b = blockIdx.x; b < p.n_pairs; b += gridDim.x) {
        const long long x0 = p.xoff[b], y0 = p.yoff[b];
        const int n = (int)(p.xoff[b + 1] - x0), m = (int)(p.yoff[b + 1] - y0);
        const int N = INFER ? n + m : n;       // dimension of the assignment
        if (N > lds.NMAX && p.leave_big) continue;
        if ((!INFER && n < m) || N > lds.NMAX) {
            // (n < m: the diagonal would need negative mass, wasserstein.py:264 -- the reference's transport has no solution)
            w2_fail<INFER, 64>(p, b, x0, y0, n, m, (!INFER && n < m) ? 1 : 2, 0.0, lane);
            continue;
        }
        if (INFER && (n == 0 || m == 0)) { w2_empty<64>(p, b, x0, y0, n, m, nullptr, lane); continue; }
        w2_solve<64, CPL, INFER>(p, b, x0, y0, n, m, lds);
        w2_sync<64>();
    }
}

// min_points < N <= 4 096: a workgroup per problem (the wavefront kernel took the others); above: status 2
template <bool INFER>
__global__ __launch_bounds__(W2_WIDE_THREADS) void tlc_w2_match_wide_kernel(W2Params p, int min_points) {
    extern __shared__ __attribute__((aligned(16))) unsigned char w2_lds[];
    const W2Lds<W2_WIDE_THREADS, W2_WIDE_CPL> lds(w2_lds);
    const int tid = threadIdx.x, b = blockIdx.x;
    if (b >= p.n_pairs) return;
    const long long x0 = p.xoff[b], y0 = p.yoff[b];
    const int n = (int)(p.xoff[b + 1] - x0), m = (int)(p.yoff[b + 1] - y0);
    const int N = INFER ? n + m : n;
    if (N <= min_points) return;
    if ((!INFER && n < m) || N > lds.NMAX) {
        w2_fail<INFER, W2_WIDE_THREADS>(p, b, x0, y0, n, m, (!INFER && n < m) ? 1 : 2, 0.0, tid);
        return;
    }
    if (INFER && (n == 0 || m == 0)) { w2_empty<W2_WIDE_THREADS>(p, b, x0, y0, n, m, lds.red, tid); return; }
    w2_solve<W2_WIDE_THREADS, W2_WIDE_CPL, INFER>(p, b, x0, y0, n, m, lds);
}

template <bool INFER>
static int launch_w2_wide(const W2Params& p, int min_points, hipStream_t s) {
    const size_t lds = W2Lds<W2_WIDE_THREADS, W2_WIDE_CPL>::BYTES;
    TLC_HIP_CHECK(hipFuncSetAttribute((const void*)tlc_w2_match_wide_kernel<INFER>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((tlc_w2_match_wide_kernel<INFER>), dim3(p.n_pairs), dim3(W2_WIDE_THREADS), lds, s, p, min_points);
    TLC_HIP_CHECK(hipGetLastError());
    return TLC_OK;
}

template <int CPL, bool INFER>
static int launch_w2(const W2Params& p, hipStream_t s) {
    const size_t lds = W2Lds<64, CPL>::BYTES;
    if (lds > 64 * 1024) TLC_HIP_CHECK(hipFuncSetAttribute((const void*)tlc_w2_match_kernel<CPL, INFER>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int grid = p.n_pairs < 16384 ? p.n_pairs : 16384;
    hipLaunchKernelGGL((tlc_w2_match_kernel<CPL, INFER>), dim3(grid), dim3(64), lds, s, p);
    TLC_HIP_CHECK(hipGetLastError());
    return TLC_OK;
}

// max_points: an upper bound of the rows of one problem (the caller knows its offsets): picks the wavefront kernel's variant (64 / 128 /
// 256 / 512 columns); above 512 a second launch gives every larger problem a 512-thread workgroup (up to 4 096 rows); beyond: status 2.
template <bool INFER>
static int dispatch_w2(W2Params& p, int max_points, hipStream_t s) {
    p.leave_big = max_points > 512;
    if (max_points <= 64) return launch_w2<1, INFER>(p, s);
    if (max_points <= 128) return launch_w2<2, INFER>(p, s);
    if (max_points <= 256) return launch_w2<4, INFER>(p, s);
    int rc = launch_w2<8, INFER>(p, s);
    if (rc != TLC_OK || max_points <= 512) return rc;
    return launch_w2_wide<INFER>(p, 512, s);
}

// The arguments of either entry, checked and packed (INFER = false: d_wyd and d_assign_y are null)
template <bool INFER>
static int w2_entry(int32_t n_problems, const int64_t* d_xoff, const double* d_X, const int64_t* d_yoff, const double* d_Y, int order,
                    int32_t max_points, double* d_loss, double* d_wxy, double* d_wxd, double* d_wyd, int32_t* d_assign_x,
                    int32_t* d_assign_y, double* d_gradX, uint8_t* d_status, void* stream) {
    auto bad = [](const char* msg) {
        tlc_set_error("%s: %s", INFER ? "tlc_w2_inference_matching" : "tlc_w2_partial_matching", msg);
        return (int)TLC_ERR_INVALID_ARG;
    };
    if (n_problems < 0) return bad("n_problems < 0");
    if (order != 1 && order != 2) return bad("order must be 1 or 2");
    if (n_problems == 0) return TLC_OK;
    if (!(d_xoff && d_yoff && d_loss && d_wxy && d_wxd && d_assign_x && d_status && (!INFER || (d_wyd && d_assign_y)))) return bad("null pointer");
    W2Params p;
    memset(&p, 0, sizeof(p));
    p.n_pairs = n_problems; p.xoff = (const long long*)d_xoff; p.X = d_X; p.yoff = (const long long*)d_yoff; p.Y = d_Y;
    p.order = order; p.loss = d_loss; p.wxy = d_wxy; p.wxd = d_wxd; p.wyd = d_wyd; p.assign = d_assign_x; p.assign_y = d_assign_y;
    p.gradX = d_gradX; p.status = d_status;
    return dispatch_w2<INFER>(p, max_points, (hipStream_t)stream);
}

}  // namespace

// The training form: max_points bounds the predicted points n of one problem.
extern "C" int tlc_w2_partial_matching(int32_t n_problems, const int64_t* d_xoff, const double* d_X, const int64_t* d_yoff,
                                       const double* d_Y, int order, int32_t max_points, double* d_loss, double* d_wxy,
                                       double* d_wxd, int32_t* d_assign, double* d_gradX, uint8_t* d_status, void* stream) {
    return w2_entry<false>(n_problems, d_xoff, d_X, d_yoff, d_Y, order, max_points, d_loss, d_wxy, d_wxd, nullptr, d_assign, nullptr, d_gradX,
                           d_status, stream);
}

// The evaluation form (wasserstein_distance_inference, wasserstein.py:93-195): both diagrams may use the diagonal.
// max_points bounds n + m (predicted + target points) of one problem.
extern "C" int tlc_w2_inference_matching(int32_t n_problems, const int64_t* d_xoff, const double* d_X, const int64_t* d_yoff,
                                         const double* d_Y, int order, int32_t max_points, double* d_loss, double* d_wxy,
                                         double* d_wxd, double* d_wyd, int32_t* d_assign_x, int32_t* d_assign_y, double* d_gradX,
                                         uint8_t* d_status, void* stream) {
    return w2_entry<true>(n_problems, d_xoff, d_X, d_yoff, d_Y, order, max_points, d_loss, d_wxy, d_wxd, d_wyd, d_assign_x, d_assign_y, d_gradX,
                          d_status, stream);
}

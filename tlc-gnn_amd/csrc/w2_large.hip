// w2_large.hip -- the matching Wasserstein loss of w2_match.hip for diagrams above one workgroup's LDS: 4 097 .. 65 536 rows
// (tlc_w2_large_matching).  The reference trains and evaluates with this loss up to 30 000 points
// (train_Teacher_Model.py:46-48, "ot.emd cannot compute loss for large graph" only beyond).
//
// The same problem, costs and outputs as w2_match.hip (its header comment defines them; the code of all three is w2_common.h's): the
// assignment of N rows onto N columns by shortest augmenting paths, every cost recomputed from the two points, no matrix.  Among
// several columns at a step's minimum the lowest one is taken (w2l_argmin), the rule of w2_match.hip's workgroup kernel.  What differs:
//   * the O(N) state (row duals u, column duals v, path lengths minv, column -> row map pcol, path links way, used marks) lies in a
//     slot of the caller's workspace (TlcW2LargeScratch), 34 B per row: 2.2 MB at the cap, resident in L2.  One workgroup of 1 024
//     threads per slot; thread t owns the columns t, t + 1 024, ...: v, minv, way and the used mark of a column are only ever touched by
//     its owner, so a step needs one barrier (the minimum over the workgroup, double-buffered in LDS) and no other exchange.
//   * a dual-feasible start: u_i = min_j c(i, j), then v_j = min_i (c(i, j) - u_i), then the rows in ascending order each take their
//     lowest free tight column.  Augmenting paths are searched only for the rows left free.
//   * the duals are updated once per augmentation: minv holds the path length from the start row (not the slack that shrinks every
//     step), and at the end of a search a used column j moves by (length of the whole path - minv[j]), like its row.  A step is then
//     one pass over the columns instead of two.
// Every loop is bounded by the problem: at most N augmentations of at most N steps.  No workgroup waits for another, no floating-point
// atomics; the order of every sum is fixed by the column index alone, so a problem's bits do not depend on the batch, the slot, the
// size of the workspace or the run.
#include <vector>

#include "scratch_layouts.h"
#include "w2_common.h"

namespace {

constexpr int W2L_THREADS = 1024, W2L_NWV = W2L_THREADS / 64, W2L_NONE = 0x7fffffff;

struct W2LargeParams : W2Problem {
    int n_problems;
    long long min_rows;        // problems of at most this many rows are left alone
    char* work;
    TlcW2LargeScratch L;       // the slot's layout (offsets in bytes)
};

// The least (val, j) of the workgroup in lexicographic order, threads without a candidate pass j < 0; -> j = W2L_NONE when nobody has
// one.  One barrier: the buffers alternate (par), and a wavefront can only reach the call after next, which writes this call's buffer
// again, through the next call's barrier -- behind every other wavefront's reads of this one.
__device__ __forceinline__ void w2l_argmin(double& val, int& j, double (*red)[W2L_NWV], int (*redj)[W2L_NWV], int& par, int lane, int wave) {
    const double wmin = tlc_wave_min_f64(j >= 0 ? val : __longlong_as_double(0x7FF0000000000000ll));
    const int cand = tlc_wave_min_i32((j >= 0 && val == wmin) ? j : W2L_NONE);
    if (lane == 0) { red[par][wave] = wmin; redj[par][wave] = cand; }
    __syncthreads();
    double d = red[par][0];
    int jj = redj[par][0];
#pragma unroll
    for (int k = 1; k < W2L_NWV; ++k) {
        const double dk = red[par][k];
        const int jk = redj[par][k];
        if (jk != W2L_NONE && (jj == W2L_NONE || dk < d || (dk == d && jk < jj))) { d = dk; jj = jk; }
    }
    par ^= 1;
    val = d; j = jj;
}

template <bool INFER>
__global__ __launch_bounds__(W2L_THREADS) void tlc_w2_large_kernel(W2LargeParams p) {
    __shared__ double red[2][W2L_NWV];
    __shared__ int redj[2][W2L_NWV];
    __shared__ double sumbuf[W2L_NWV];
    constexpr int W = W2L_THREADS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double INF = __longlong_as_double(0x7FF0000000000000ll);
    const double QNAN = __longlong_as_double(0x7FF8000000000000ll);
    char* slot = p.work + (long long)blockIdx.x * p.L.slot_bytes;
    long long* ctr = (long long*)(slot + p.L.head);
    double* u = (double*)(slot + p.L.u);
    double* v = (double*)(slot + p.L.v);
    double* minv = (double*)(slot + p.L.minv);
    int* pcol = (int*)(slot + p.L.pcol);
    int* way = (int*)(slot + p.L.way);
    unsigned char* used = (unsigned char*)(slot + p.L.used);
    unsigned char* rdone = (unsigned char*)(slot + p.L.rdone);
    long long c_steps = 0, c_augs = 0, c_start = 0, c_problems = 0;    // (uniform)
    int par = 0;
    long long taken = 0;
    for (int b = 0; b < p.n_problems; ++b) {
        const long long x0 = p.xoff[b], y0 = p.yoff[b];
        const long long nn = p.xoff[b + 1] - x0, mm = p.yoff[b + 1] - y0;
        const long long NN = INFER ? nn + mm : nn;
        if (NN <= p.min_rows) continue;                               // (left alone: the LDS kernels' class)
        if (taken++ % gridDim.x != blockIdx.x) continue;              // (this slot's problems: a fixed stride)
        ++c_problems;
        if ((!INFER && nn < mm) || NN > p.L.rows) {
            // (n < m: the diagonal would need negative mass, wasserstein.py:264.  p.L.rows: the host sized the slots for the largest
            // problem up to TlcW2LargeScratch::NMAX rows, so only a problem above the cap is beyond it)
            w2_fail<INFER, W>(p, b, x0, y0, nn, mm, (!INFER && nn < mm) ? 1 : 2, 0.0, tid);
            continue;
        }
        const int n = (int)nn, m = (int)mm, N = (int)NN;
        if (INFER && (n == 0 || m == 0)) { w2_empty<W>(p, b, x0, y0, n, m, sumbuf, tid); continue; }
        bool finite = true;
        for (int i = tid; i < n; i += W) finite = finite && w2_finite(p.X[2 * (x0 + i)], p.X[2 * (x0 + i) + 1]);
        for (int j = tid; j < m; j += W) finite = finite && w2_finite(p.Y[2 * (y0 + j)], p.Y[2 * (y0 + j) + 1]);
        if (__syncthreads_or(!finite)) {
            w2_fail<INFER, W>(p, b, x0, y0, n, m, 3, QNAN, tid);
            continue;
        }
        // a row's own values (uniform: every thread loads the same words) and the cost of (row, column) from the two points
        struct Row { bool real; double x, y, cd; };
        auto row_of = [&](int i) -> Row {
            Row r;
            r.real = !INFER || i < n;
            r.x = r.y = r.cd = 0.0;
            if (r.real) { r.x = p.X[2 * (x0 + i)]; r.y = p.X[2 * (x0 + i) + 1]; r.cd = w2_pow((r.y - r.x) * 0.5, p.order); }
            return r;
        };
        auto cost_at = [&](const Row& r, bool target, double yx, double yy) -> double {      // (yx, yy) = Y_j, loaded where j < m
            return w2_cost<INFER>(r.real, r.x, r.y, r.cd, target, yx, yy, w2_pow((yy - yx) * 0.5, p.order), p.order);
        };
        auto cost_of = [&](const Row& r, int j) -> double {
            return j < m ? cost_at(r, true, p.Y[2 * (y0 + j)], p.Y[2 * (y0 + j) + 1]) : cost_at(r, false, 0.0, 0.0);
        };
        // ---- the start, 1: u_i = min_j c(i, j), a thread per row.  The columns from m on all cost a row the same.
        for (int i = tid; i < N; i += W) {
            const Row r = row_of(i);
            double best = N > m ? cost_of(r, m) : INF;
            for (int j = 0; j < m; ++j) { const double c = cost_of(r, j); best = c < best ? c : best; }
            u[i] = best;
        }
        __syncthreads();
        // ---- 2: v_j = min_i (c(i, j) - u_i), a thread per target column.  The rows from n on (INFER) all have the same cost and the
        // same u (the same operations made them), so row n stands for them; then the one value of the columns from m on.
        for (int j = tid; j < m; j += W) {
            const double yx = p.Y[2 * (y0 + j)], yy = p.Y[2 * (y0 + j) + 1];
            double best = INF;
            for (int i = 0; i < n; ++i) { const double c = cost_at(row_of(i), true, yx, yy) - u[i]; best = c < best ? c : best; }
            if (INFER) { const double c = cost_at(row_of(n), true, yx, yy) - u[n]; best = c < best ? c : best; }
            v[j] = best;
        }
        if (N > m) {
            double best = INF;
            for (int i = tid; i < n; i += W) { const double c = cost_at(row_of(i), false, 0.0, 0.0) - u[i]; best = c < best ? c : best; }
            if (INFER && tid == 0) { const double c = 0.0 - u[n]; best = c < best ? c : best; }
            int any = 0;
            w2l_argmin(best, any, red, redj, par, lane, wave);
            for (int j = tid; j < N; j += W) if (j >= m) v[j] = best;
        }
        for (int j = tid; j < N; j += W) { pcol[j] = -1; rdone[j] = 0; }
        __syncthreads();
        // ---- 3: the rows in ascending order each take their lowest free tight column.  pcol[j] is read by j's owner alone here.
        for (int i = 0; i < N; ++i) {
            const Row r = row_of(i);
            const double ui = u[i];
            int found = -1;
            for (int j = tid; j < N; j += W)
                if (pcol[j] < 0 && (cost_of(r, j) - ui) - v[j] <= 0.0) { found = j; break; }
            double z = 0.0;
            w2l_argmin(z, found, red, redj, par, lane, wave);
            if (found != W2L_NONE) {
                if ((found & (W - 1)) == tid) { pcol[found] = i; rdone[i] = 1; }
                ++c_start;
            }
        }
        __syncthreads();
        // ---- the augmentations: a shortest path from every row the start left free ---------------------------------------------
        bool failed = false;
        for (int i = 0; i < N && !failed; ++i) {
            if (rdone[i]) continue;                                   // (uniform)
            for (int j = tid; j < N; j += W) { minv[j] = INF; used[j] = 0; }
            double dist = 0.0;                                        // the length of the path to the column settled last
            int i0 = i, j0 = -1, sink = -1;
            for (int step = 0; step < N; ++step) {
                const Row r = row_of(i0);
                const double ui = u[i0];
                double best = INF;
                int bj = -1;
                // four of the thread's columns at a time, every load of the four issued before the first use: a step then waits
                // for one round trip to L2 per four columns, not two per column (used[j], then the rest)
                for (int jb = tid; jb < N; jb += 4 * W) {
                    bool us[4];
                    double vj[4], mv[4], yx[4], yy[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int j = jb + k * W;
                        us[k] = j < N ? used[j] != 0 : true;
                        vj[k] = j < N ? v[j] : 0.0;
                        mv[k] = j < N ? minv[j] : INF;
                        yx[k] = j < m ? p.Y[2 * (y0 + j)] : 0.0;
                        yy[k] = j < m ? p.Y[2 * (y0 + j) + 1] : 0.0;
                    }
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int j = jb + k * W;
                        if (us[k]) continue;
                        // (w2_cost on the loaded point, written out: through cost_at this loop measured 1 % slower in the
                        // evaluation form, 5 408 against 5 352 ms at 2 049 + 2 048 points; like this 5 369)
                        double c;
                        if (j < m) {
                            if (r.real) {
                                const double dx = fabs(r.x - yx[k]), dy = fabs(r.y - yy[k]);
                                c = w2_pow(dx > dy ? dx : dy, p.order);
                            } else c = w2_pow((yy[k] - yx[k]) * 0.5, p.order);
                        } else c = r.real ? r.cd : 0.0;
                        const double cur = dist + ((c - ui) - vj[k]);
                        if (cur < mv[k]) { mv[k] = cur; minv[j] = cur; way[j] = j0; }
                        if (mv[k] < best) { best = mv[k]; bj = j; }   // (ascending j: among equal lengths the lowest column)
                    }
                }
                w2l_argmin(best, bj, red, redj, par, lane, wave);
                if (bj == W2L_NONE) break;                            // (uniform; cannot happen with finite costs)
                ++c_steps;
                dist = best; j0 = bj;
                if ((bj & (W - 1)) == tid) used[bj] = 1;
                i0 = pcol[bj];                                        // (written in the start and by the augmentations, behind barriers)
                if (i0 < 0) { sink = bj; break; }
            }
            if (sink < 0) { failed = true; break; }
            // the dual update of the whole search at once: a used column, and the row it holds, by what was left of the path when the
            // column was settled (the sink: 0); the start row by the whole length.  The rows of distinct columns are distinct.
            for (int j = tid; j < N; j += W)
                if (used[j]) {
                    const double d = dist - minv[j];
                    v[j] -= d;
                    const int rj = pcol[j];
                    if (rj >= 0) u[rj] += d;
                }
            if (tid == 0) u[i] += dist;
            __syncthreads();
            // augment along the alternating path (one thread: at most N links)
            if (tid == 0) {
                int j = sink;
                for (int k = 0; k < N && j >= 0; ++k) {
                    const int jp = way[j];
                    pcol[j] = jp < 0 ? i : pcol[jp];
                    j = jp;
                }
            }
            ++c_augs;
            __syncthreads();
        }
        if (failed) {
            w2_fail<INFER, W>(p, b, x0, y0, n, m, 3, QNAN, tid);
            __syncthreads();
            continue;
        }
        // ---- the loss, its parts and the maps, then d loss / d X, from the finished matching: a thread's own columns ------------------
        W2Sums sums;
        for (int j = tid; j < N; j += W) {
            const int i = pcol[j];
            const Row r = row_of(i);
            const double yx = j < m ? p.Y[2 * (y0 + j)] : 0.0, yy = j < m ? p.Y[2 * (y0 + j) + 1] : 0.0;
            sums = w2_pair_loss<INFER>(p, x0, y0, n, m, i, j, r.x, r.y, yx, yy, sums);
        }
        const double Lv = w2_finish<INFER, W>(p, b, sums, sumbuf, tid);
        if (p.gradX) {
            for (int j = tid; j < N; j += W) {
                const int i = pcol[j];
                if (i >= n) continue;
                const double yx = j < m ? p.Y[2 * (y0 + j)] : 0.0, yy = j < m ? p.Y[2 * (y0 + j) + 1] : 0.0;
                double gx, gy;
                w2_pair_grad(p.order, Lv, j < m, p.X[2 * (x0 + i)], p.X[2 * (x0 + i) + 1], yx, yy, gx, gy);
                p.gradX[2 * (x0 + i)] = gx;
                p.gradX[2 * (x0 + i) + 1] = gy;
            }
        }
        __syncthreads();
    }
    // the counters of this slot's problems (read by tools/time_w2_large.py alone)
    if (tid == 0) { ctr[0] = c_steps; ctr[1] = c_augs; ctr[2] = c_start; ctr[3] = c_problems; }
}

}  // namespace

extern "C" int64_t tlc_w2_large_work_bytes(int64_t max_rows, int32_t slots) {
    if (max_rows < 0 || slots < 0) return -1;
    return TlcW2LargeScratch(max_rows).total(slots);
}

// Reads the offsets back (one copy that waits for the stream): the host counts the problems above min_rows and finds the largest
// one, which size the slots and the grid.
extern "C" int tlc_w2_large_matching(int32_t n_problems, const int64_t* d_xoff, const double* d_X, const int64_t* d_yoff, const double* d_Y,
                                     int order, int infer, int32_t min_rows, double* d_loss, double* d_wxy, double* d_wxd, double* d_wyd,
                                     int32_t* d_assign_x, int32_t* d_assign_y, double* d_gradX, uint8_t* d_status, void* d_work,
                                     int64_t work_bytes, void* stream) {
    TLC_REQUIRE(n_problems >= 0, "n_problems < 0");
    TLC_REQUIRE(order == 1 || order == 2, "order must be 1 or 2");
    TLC_REQUIRE(infer == 0 || infer == 1, "infer must be 0 or 1");
    TLC_REQUIRE(min_rows >= -1, "min_rows < -1");
    if (n_problems == 0) return TLC_OK;
    TLC_REQUIRE(d_xoff && d_yoff && d_loss && d_wxy && d_wxd && d_assign_x && d_status, "null pointer");
    TLC_REQUIRE(!infer || (d_wyd && d_assign_y), "null pointer (d_wyd / d_assign_y of the evaluation form)");
    TLC_REQUIRE(d_work && work_bytes >= 0, "no workspace");
    TLC_REQUIRE(((uintptr_t)d_work & 255) == 0, "d_work is not 256-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    std::vector<int64_t> hx((size_t)n_problems + 1), hy((size_t)n_problems + 1);
    TLC_HIP_CHECK(hipMemcpyAsync(hx.data(), d_xoff, hx.size() * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    TLC_HIP_CHECK(hipMemcpyAsync(hy.data(), d_yoff, hy.size() * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    TLC_HIP_CHECK(hipStreamSynchronize(s));
    int64_t count = 0, rows_max = 0;
    for (int32_t b = 0; b < n_problems; ++b) {
        const int64_t n = hx[b + 1] - hx[b], m = hy[b + 1] - hy[b];
        TLC_REQUIRE(hx[b] >= 0 && hy[b] >= 0 && n >= 0 && m >= 0, "offsets must start at >= 0 and not decrease");
        const int64_t N = infer ? n + m : n;
        if (N <= min_rows) continue;
        ++count;
        if (N <= TlcW2LargeScratch::NMAX && (infer || n >= m)) rows_max = std::max(rows_max, N);
    }
    if (count == 0) return TLC_OK;
    TLC_REQUIRE((d_X || hx[n_problems] == 0) && (d_Y || hy[n_problems] == 0), "null pointer (points)");
    W2LargeParams p;
    memset((void*)&p, 0, sizeof(p));
    p.L = TlcW2LargeScratch(rows_max);
    TLC_REQUIRE(work_bytes >= p.L.total(1), "d_work is smaller than tlc_w2_large_work_bytes(rows of the largest problem, 1)");
    p.n_problems = n_problems; p.xoff = (const long long*)d_xoff; p.X = d_X; p.yoff = (const long long*)d_yoff; p.Y = d_Y;
    p.order = order; p.min_rows = min_rows; p.loss = d_loss; p.wxy = d_wxy; p.wxd = d_wxd; p.wyd = d_wyd; p.assign = d_assign_x;
    p.assign_y = d_assign_y; p.gradX = d_gradX; p.status = d_status; p.work = (char*)d_work;
    const unsigned grid = (unsigned)std::min<int64_t>(std::min<int64_t>(p.L.slots_in(work_bytes), count), 65535);
    if (infer) hipLaunchKernelGGL((tlc_w2_large_kernel<true>), dim3(grid), dim3(W2L_THREADS), 0, s, p);
    else hipLaunchKernelGGL((tlc_w2_large_kernel<false>), dim3(grid), dim3(W2L_THREADS), 0, s, p);
    TLC_HIP_CHECK(hipGetLastError());
    return TLC_OK;
}

// w2_large.hip -- the matching Wasserstein loss of w2_match.hip for diagrams above one workgroup's LDS: 4 097 .. 65 536 rows
// (tlc_w2_large_matching).  The reference trains and evaluates with this loss up to 30 000 points
// (train_Teacher_Model.py:46-48, "ot.emd cannot compute loss for large graph" only beyond).
//
// The same problem, costs, tie rule and outputs as w2_match.hip (its header comment defines them): the assignment of N rows onto N
// columns by shortest augmenting paths, every cost recomputed from the two points, no matrix.  What differs:
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
#include "tlc_common.h"

namespace {

constexpr int W2L_THREADS = 1024, W2L_NWV = W2L_THREADS / 64, W2L_NONE = 0x7fffffff;

struct W2LargeParams {
    int n_problems;
    const long long* xoff;
    const double* X;
    const long long* yoff;
    const double* Y;
    int order;
    long long min_rows;        // problems of at most this many rows are left alone
    double* loss;
    double* wxy;
    double* wxd;
    double* wyd;               // INFER only
    int* assign;               // [sum n]
    int* assign_y;             // INFER only, [sum m]
    double* gradX;             // or null
    unsigned char* status;
    char* work;
    TlcW2LargeScratch L;       // the slot's layout (offsets in bytes)
};

__device__ __forceinline__ double w2l_pow(double d, int order) { return order == 2 ? d * d : d; }

// what w2_fail of w2_match.hip writes: the outputs of a problem that is not solved (or of one against the empty diagram)
template <bool INFER>
__device__ __forceinline__ void w2l_fail(const W2LargeParams& p, int b, long long x0, long long y0, long long n, long long m, int code,
                                         double lossv, int tid) {
    if (tid == 0) {
        p.status[b] = (unsigned char)code; p.loss[b] = lossv; p.wxy[b] = 0.0; p.wxd[b] = 0.0;
        if (INFER) p.wyd[b] = 0.0;
    }
    for (long long i = tid; i < n; i += W2L_THREADS) {
        p.assign[x0 + i] = -1;
        if (p.gradX) { p.gradX[2 * (x0 + i)] = 0.0; p.gradX[2 * (x0 + i) + 1] = 0.0; }
    }
    if (INFER) for (long long j = tid; j < m; j += W2L_THREADS) p.assign_y[y0 + j] = -1;
}

__device__ __forceinline__ int w2l_wave_min_i32(int v) {
    int t;
    t = (int)tlc_lane_xor_u32<1>((unsigned)v);  v = t < v ? t : v;
    t = (int)tlc_lane_xor_u32<2>((unsigned)v);  v = t < v ? t : v;
    t = (int)tlc_lane_xor_u32<4>((unsigned)v);  v = t < v ? t : v;
    t = (int)tlc_lane_xor_u32<8>((unsigned)v);  v = t < v ? t : v;
    t = (int)tlc_lane_xor_u32<16>((unsigned)v); v = t < v ? t : v;
    t = (int)tlc_lane_xor_u32<32>((unsigned)v); v = t < v ? t : v;
    return v;
}

// The least (val, j) of the workgroup in lexicographic order, threads without a candidate pass j < 0; -> j = W2L_NONE when nobody has
// one.  One barrier: the buffers alternate (par), and a wavefront can only reach the call after next, which writes this call's buffer
// again, through the next call's barrier -- behind every other wavefront's reads of this one.
__device__ __forceinline__ void w2l_argmin(double& val, int& j, double (*red)[W2L_NWV], int (*redj)[W2L_NWV], int& par, int lane, int wave) {
    const double wmin = tlc_wave_min_f64(j >= 0 ? val : __longlong_as_double(0x7FF0000000000000ll));
    const int cand = w2l_wave_min_i32((j >= 0 && val == wmin) ? j : W2L_NONE);
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

// the sum of the workgroup: the butterfly inside each wavefront, then the wavefronts ascending (buf: [W2L_NWV])
__device__ __forceinline__ double w2l_sum(double s, double* buf, int lane, int wave) {
    for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o);
    __syncthreads();
    if (lane == 0) buf[wave] = s;
    __syncthreads();
    double t = 0.0;
    for (int k = 0; k < W2L_NWV; ++k) t += buf[k];
    return t;
}

// INFER = false: n rows (predicted) onto m targets + (n - m) diagonal copies.  INFER = true: N = n + m rows (predicted, then m
// diagonal rows) onto N columns (targets, then n diagonal columns).  cost(i, j):
//     i < n, j < m: ||X_i - Y_j||_inf ^ p      i < n, j >= m: cxd_i      i >= n, j < m: cdy_j      i >= n, j >= m: 0
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
            w2l_fail<INFER>(p, b, x0, y0, nn, mm, (!INFER && nn < mm) ? 1 : 2, 0.0, tid);
            continue;
        }
        const int n = (int)nn, m = (int)mm, N = (int)NN;
        if (INFER && (n == 0 || m == 0)) {
            // empty diagram(s) (:98-113): distance to the empty diagram, the parts are reported as 0
            const double* P = n ? p.X : p.Y;
            const long long o = n ? x0 : y0;
            const int cnt = n ? n : m;
            double s = 0.0;
            for (int i = tid; i < cnt; i += W) {
                const double d = fabs((P[2 * (o + i) + 1] - P[2 * (o + i)]) * 0.5);
                s += p.order == 2 ? d * d : d;
            }
            const double t = w2l_sum(s, sumbuf, lane, wave);
            const double Lv = p.order == 2 ? sqrt(t) : t;
            w2l_fail<INFER>(p, b, x0, y0, n, m, 0, Lv, tid);
            if (p.gradX)
                for (int i = tid; i < n; i += W) {
                    const double sd = (p.X[2 * (x0 + i) + 1] - p.X[2 * (x0 + i)]) * 0.5;
                    const double w = p.order == 2 ? (Lv > 0.0 ? sd / Lv : 0.0) : (sd > 0.0 ? 1.0 : (sd < 0.0 ? -1.0 : 0.0));
                    p.gradX[2 * (x0 + i)] = -0.5 * w; p.gradX[2 * (x0 + i) + 1] = 0.5 * w;
                }
            continue;
        }
        bool finite = true;
        for (int i = tid; i < n; i += W) {
            const double bx = p.X[2 * (x0 + i)], by = p.X[2 * (x0 + i) + 1];
            finite = finite && (bx - bx == 0.0) && (by - by == 0.0);
        }
        for (int j = tid; j < m; j += W) {
            const double bx = p.Y[2 * (y0 + j)], by = p.Y[2 * (y0 + j) + 1];
            finite = finite && (bx - bx == 0.0) && (by - by == 0.0);
        }
        if (__syncthreads_or(!finite)) {
            // NaN / Inf coordinates: every reduced cost would be NaN and no column would ever be the minimum
            w2l_fail<INFER>(p, b, x0, y0, n, m, 3, QNAN, tid);
            continue;
        }
        // a row's own values (uniform: every thread loads the same words) and the cost of (row, column) from the two points
        struct Row { bool real; double x, y, cd; };
        auto row_of = [&](int i) -> Row {
            Row r;
            r.real = !INFER || i < n;
            r.x = r.y = r.cd = 0.0;
            if (r.real) { r.x = p.X[2 * (x0 + i)]; r.y = p.X[2 * (x0 + i) + 1]; r.cd = w2l_pow((r.y - r.x) * 0.5, p.order); }
            return r;
        };
        auto cost_of = [&](const Row& r, int j) -> double {
            if (j < m) {
                const double yx = p.Y[2 * (y0 + j)], yy = p.Y[2 * (y0 + j) + 1];
                if (r.real) {
                    const double dx = fabs(r.x - yx), dy = fabs(r.y - yy);
                    return w2l_pow(dx > dy ? dx : dy, p.order);            // chebyshev ^ order (:59-60)
                }
                return w2l_pow((yy - yx) * 0.5, p.order);
            }
            return r.real ? r.cd : 0.0;
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
            for (int i = 0; i < n; ++i) {
                const double dx = fabs(p.X[2 * (x0 + i)] - yx), dy = fabs(p.X[2 * (x0 + i) + 1] - yy);
                const double c = w2l_pow(dx > dy ? dx : dy, p.order) - u[i];
                best = c < best ? c : best;
            }
            if (INFER) { const double c = w2l_pow((yy - yx) * 0.5, p.order) - u[n]; best = c < best ? c : best; }
            v[j] = best;
        }
        if (N > m) {
            double best = INF;
            for (int i = tid; i < n; i += W) {
                const double c = w2l_pow((p.X[2 * (x0 + i) + 1] - p.X[2 * (x0 + i)]) * 0.5, p.order) - u[i];
                best = c < best ? c : best;
            }
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
                        double c;                                     // (cost_of on the loaded point)
                        if (j < m) {
                            if (r.real) {
                                const double dx = fabs(r.x - yx[k]), dy = fabs(r.y - yy[k]);
                                c = w2l_pow(dx > dy ? dx : dy, p.order);
                            } else c = w2l_pow((yy[k] - yx[k]) * 0.5, p.order);
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
            w2l_fail<INFER>(p, b, x0, y0, n, m, 3, QNAN, tid);
            __syncthreads();
            continue;
        }
        // ---- the loss and its pieces (:303-372 / :140-195): matched distances d_k, loss = (sum |d_k|^p)^(1/p) -------------------
        double sxy = 0.0, sxd = 0.0, syd = 0.0;
        for (int j = tid; j < N; j += W) {
            const int i = pcol[j];
            if (i < n) {
                const double xi = p.X[2 * (x0 + i)], yi = p.X[2 * (x0 + i) + 1];
                if (j < m) {
                    const double dx = fabs(xi - p.Y[2 * (y0 + j)]), dy = fabs(yi - p.Y[2 * (y0 + j) + 1]);
                    const double d = dx > dy ? dx : dy;
                    sxy += p.order == 2 ? d * d : d;
                    p.assign[x0 + i] = j;
                    if (INFER) p.assign_y[y0 + j] = i;
                } else {
                    const double d = fabs((yi - xi) * 0.5);
                    sxd += p.order == 2 ? d * d : d;
                    p.assign[x0 + i] = -1;
                }
            } else if (j < m) {                                       // (INFER) a target sent to the diagonal
                const double d = fabs((p.Y[2 * (y0 + j) + 1] - p.Y[2 * (y0 + j)]) * 0.5);
                syd += p.order == 2 ? d * d : d;
                p.assign_y[y0 + j] = -1;
            }
        }
        sxy = w2l_sum(sxy, sumbuf, lane, wave);
        sxd = w2l_sum(sxd, sumbuf, lane, wave);
        if (INFER) syd = w2l_sum(syd, sumbuf, lane, wave);
        const double tot = sxy + sxd + syd;
        const double Lv = p.order == 2 ? sqrt(tot) : tot;
        if (tid == 0) {
            p.status[b] = 0;
            p.loss[b] = Lv;
            p.wxy[b] = p.order == 2 ? sqrt(sxy) : sxy;
            p.wxd[b] = p.order == 2 ? sqrt(sxd) : sxd;
            if (INFER) p.wyd[b] = p.order == 2 ? sqrt(syd) : syd;
        }
        // ---- d loss / d X: through the matched distances only (the matching is piecewise constant) ----------------------------
        if (p.gradX) {
            for (int j = tid; j < N; j += W) {
                const int i = pcol[j];
                if (i >= n) continue;
                const double xi = p.X[2 * (x0 + i)], yi = p.X[2 * (x0 + i) + 1];
                double gx = 0.0, gy = 0.0;
                if (j < m) {
                    const double ex = p.Y[2 * (y0 + j)] - xi, ey = p.Y[2 * (y0 + j) + 1] - yi;          // Y - X (:311)
                    const double ax = fabs(ex), ay = fabs(ey);
                    const double d = ax > ay ? ax : ay;
                    const double w = p.order == 2 ? (Lv > 0.0 ? d / Lv : 0.0) : 1.0;                     // dL/dd
                    if (ax >= ay) gx = -w * (ex > 0.0 ? 1.0 : (ex < 0.0 ? -1.0 : 0.0));
                    else gy = -w * (ey > 0.0 ? 1.0 : (ey < 0.0 ? -1.0 : 0.0));
                } else {
                    const double s = (yi - xi) * 0.5;                                                    // signed distance to the diagonal
                    const double w = p.order == 2 ? (Lv > 0.0 ? s / Lv : 0.0) : (s > 0.0 ? 1.0 : (s < 0.0 ? -1.0 : 0.0));
                    gx = -0.5 * w; gy = 0.5 * w;
                }
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

// w2_common.h -- what is the same problem in every tier of the matching Wasserstein loss: the wavefront and the workgroup kernel of
// w2_match.hip (rows in LDS, columns in registers) and the workspace tier of w2_large.hip (everything in global memory).
// The problem, its costs and its outputs are defined in w2_match.hip's header comment.  Here: the problem's arguments, the cost of a
// (row, column) pair, the outputs of a problem that is not solved or that meets the empty diagram, and the loss, its parts, the two maps
// and d loss / d X of a finished matching, pair by pair.  Every function works on values its caller has loaded: where the points lie
// (LDS, registers, global memory) and the loop over a thread's own columns are the kernel's business.
#pragma once
#include "tlc_common.h"

// The inputs and outputs of a batch of problems (tlc_w2_partial_matching / tlc_w2_inference_matching / tlc_w2_large_matching)
struct W2Problem {
    const long long* xoff;     // [B+1] rows of X per problem
    const double* X;           // [sum n, 2] predicted (birth, death)
    const long long* yoff;     // [B+1]
    const double* Y;           // [sum m, 2] target
    int order;                 // p: 1 or 2
    double* loss;              // [B]
    double* wxy;               // [B]
    double* wxd;               // [B]
    double* wyd;               // [B], INFER only
    int* assign;               // [sum n]: target index (problem-local), -1 = diagonal
    int* assign_y;             // [sum m], INFER only: predicted index (problem-local) a target is matched to, -1 = diagonal
    double* gradX;             // [sum n, 2] or null
    unsigned char* status;     // [B]: 0 ok, 1 fewer predicted than target points, 2 too many points, 3 non-finite coordinates
};

#ifdef __HIPCC__
__device__ __forceinline__ double w2_pow(double d, int order) { return order == 2 ? d * d : d; }
__device__ __forceinline__ double w2_sign(double v) { return v > 0.0 ? 1.0 : (v < 0.0 ? -1.0 : 0.0); }
// neither NaN nor Inf: with one of them every reduced cost would be NaN, no column would ever be the minimum
__device__ __forceinline__ bool w2_finite(double bx, double by) { return (bx - bx == 0.0) && (by - by == 0.0); }

// INFER = false: n rows (predicted) onto m targets + (n - m) diagonal copies.  INFER = true: N = n + m rows (predicted, then m
// diagonal rows) onto N columns (targets, then n diagonal columns).  cost(i, j):
//     i < n, j < m: ||X_i - Y_j||_inf ^ p      i < n, j >= m: cxd_i      i >= n, j < m: cdy_j      i >= n, j >= m: 0
// row_real: i < n, (xi, yi) = X_i, cxd = w2_pow((yi - xi) / 2);  col_target: j < m, (yx, yy) = Y_j, cdy = w2_pow((yy - yx) / 2)
// (_dist_to_diag with internal_p = inf, wasserstein.py:30-42; chebyshev ^ order, :59-60)
template <bool INFER>
__device__ __forceinline__ double w2_cost(bool row_real, double xi, double yi, double cxd, bool col_target, double yx, double yy, double cdy,
                                          int order) {
    if (col_target) {
        if (!INFER || row_real) {
            const double dx = fabs(xi - yx), dy = fabs(yi - yy);
            return w2_pow(dx > dy ? dx : dy, order);
        }
        return cdy;
    }
    return (!INFER || row_real) ? cxd : 0.0;
}

// The sum over the T threads of a workgroup, in one order whatever T is: the xor butterfly 32, 16, .., 1 inside each wavefront, then the
// wavefronts ascending (buf: [T / 64] in LDS, not needed for T = 64; the first barrier lets a caller use buf for sum after sum)
template <int T>
__device__ __forceinline__ double w2_block_sum(double s, double* buf) {
    for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o);
    if (T == 64) return s;
    __syncthreads();
    if (tlc_lane() == 0) buf[threadIdx.x >> 6] = s;
    __syncthreads();
    double t = 0.0;
    for (int k = 0; k < T / 64; ++k) t += buf[k];
    return t;
}

// A problem that is not solved: its outputs are defined (zero loss or NaN, no matching, zero gradient).  T threads, tid = 0 .. T - 1.
template <bool INFER, int T>
__device__ __forceinline__ void w2_fail(const W2Problem& p, int b, long long x0, long long y0, long long n, long long m, int code, double lossv,
                                        int tid) {
    if (tid == 0) {
        p.status[b] = (unsigned char)code; p.loss[b] = lossv; p.wxy[b] = 0.0; p.wxd[b] = 0.0;
        if (INFER) p.wyd[b] = 0.0;
    }
    for (long long i = tid; i < n; i += T) {
        p.assign[x0 + i] = -1;
        if (p.gradX) { p.gradX[2 * (x0 + i)] = 0.0; p.gradX[2 * (x0 + i) + 1] = 0.0; }
    }
    if (INFER) for (long long j = tid; j < m; j += T) p.assign_y[y0 + j] = -1;
}

// The three parts of sum |d_k|^p: predicted points on targets, predicted points on the diagonal, (INFER) targets on the diagonal
struct W2Sums { double xy = 0.0, xd = 0.0, yd = 0.0; };

// One pair (row i, column j) of the finished matching (:303-372 / :140-195): its |d|^p goes to the part it belongs to and the two maps
// get their entries; -> the sums with it.  (xi, yi) = X_i where i < n, (yx, yy) = Y_j where j < m; a diagonal row on a diagonal column is
// nothing.  (The sums go in and out by value: through a reference the compiler picks the part by address and keeps all three in scratch.)
template <bool INFER>
__device__ __forceinline__ W2Sums w2_pair_loss(const W2Problem& p, long long x0, long long y0, int n, int m, int i, int j, double xi, double yi,
                                               double yx, double yy, W2Sums s) {
    if (i < n) {
        if (j < m) {
            const double dx = fabs(xi - yx), dy = fabs(yi - yy);
            s.xy += w2_pow(dx > dy ? dx : dy, p.order);
            p.assign[x0 + i] = j;
            if (INFER) p.assign_y[y0 + j] = i;
        } else {
            s.xd += w2_pow(fabs((yi - xi) * 0.5), p.order);
            p.assign[x0 + i] = -1;
        }
    } else if (INFER && j < m) {
        s.yd += w2_pow(fabs((yy - yx) * 0.5), p.order);
        p.assign_y[y0 + j] = -1;
    }
    return s;
}

// d loss / d X_i of a predicted point: through its own matched distance d only (the matching is piecewise constant), dL/dd = d^(p-1) /
// L^(p-1).  on_target: matched to the target (yx, yy), the coordinate that attains the chebyshev distance moves (birth wins a tie);
// else the point went to the diagonal and both coordinates move.
__device__ __forceinline__ void w2_pair_grad(int order, double L, bool on_target, double xi, double yi, double yx, double yy, double& gx,
                                             double& gy) {
    gx = 0.0; gy = 0.0;
    if (on_target) {
        const double ex = yx - xi, ey = yy - yi;                              // Y - X (:311)
        const double ax = fabs(ex), ay = fabs(ey);
        const double d = ax > ay ? ax : ay;
        const double w = order == 2 ? (L > 0.0 ? d / L : 0.0) : 1.0;
        if (ax >= ay) gx = -w * w2_sign(ex);
        else gy = -w * w2_sign(ey);
    } else {
        const double s = (yi - xi) * 0.5;                                     // signed distance to the diagonal
        const double w = order == 2 ? (L > 0.0 ? s / L : 0.0) : w2_sign(s);
        gx = -0.5 * w; gy = 0.5 * w;
    }
}

// The outputs of a solved problem from a thread's three sums (buf: w2_block_sum's): loss = (sum |d_k|^p)^(1/p); -> the loss
template <bool INFER, int T>
__device__ __forceinline__ double w2_finish(const W2Problem& p, int b, W2Sums s, double* buf, int tid) {
    s.xy = w2_block_sum<T>(s.xy, buf);
    s.xd = w2_block_sum<T>(s.xd, buf);
    if (INFER) s.yd = w2_block_sum<T>(s.yd, buf);
    const double tot = s.xy + s.xd + s.yd;
    const double L = p.order == 2 ? sqrt(tot) : tot;
    if (tid == 0) {
        p.status[b] = 0;
        p.loss[b] = L;
        p.wxy[b] = p.order == 2 ? sqrt(s.xy) : s.xy;
        p.wxd[b] = p.order == 2 ? sqrt(s.xd) : s.xd;
        if (INFER) p.wyd[b] = p.order == 2 ? sqrt(s.yd) : s.yd;
    }
    return L;
}

// (INFER) one diagram against the empty diagram (n == 0 or m == 0, wasserstein.py:98-113): the total persistence of the other one,
// (sum |d/2|^p)^(1/p); the three logged parts are returned as 0, nothing is matched, and the predicted points (if they are the ones
// there) get the gradient of going to the diagonal.
template <int T>
__device__ __forceinline__ void w2_empty(const W2Problem& p, int b, long long x0, long long y0, int n, int m, double* buf, int tid) {
    const double* P = n ? p.X : p.Y;
    const long long o = n ? x0 : y0;
    const int cnt = n ? n : m;
    double s = 0.0;
    for (int i = tid; i < cnt; i += T) s += w2_pow(fabs((P[2 * (o + i) + 1] - P[2 * (o + i)]) * 0.5), p.order);
    s = w2_block_sum<T>(s, buf);
    const double L = p.order == 2 ? sqrt(s) : s;
    w2_fail<true, T>(p, b, x0, y0, n, m, 0, L, tid);
    if (p.gradX)
        for (int i = tid; i < n; i += T) {
            double gx, gy;
            w2_pair_grad(p.order, L, false, p.X[2 * (x0 + i)], p.X[2 * (x0 + i) + 1], 0.0, 0.0, gx, gy);
            p.gradX[2 * (x0 + i)] = gx; p.gradX[2 * (x0 + i) + 1] = gy;
        }
}
#endif

// dgm_gram.hip -- Gram matrices of persistence diagram kernels and their gradient (tlc_dgm_gram, tlc_dgm_gram_vjp).
//
// out[i, j] = scale * sum_p sum_q w_p w_q (e1 - mirror * e2), a double sum of Gaussians over the point pairs of X_i and Y_j;
// include/tlcgnn.h defines it and its summation order operation by operation.  The forward's work item is a UNIT: one slice of
// DG_SLICE points of X_i against one group of DG_GROUP points of Y_j.  A wavefront takes a unit: lane l holds point q of a 64-point
// chunk of the group, the slice's points pass by as wave-uniform readlanes (64 at a time, loaded coalesced), the lane adds its summands
// over p ascending, one butterfly folds the chunk and the chunks are added ascending.  A fixed grid walks the units.
//
//   every pair one unit     (max_nx_points <= DG_SLICE and max_ny_points <= DG_GROUP, decided by the DECLARED sizes): unit u is pair u,
//                           the wavefront stores scale * P itself.  No workspace, one launch.
//   otherwise               the entry uploads the unit-prefix arrays (slices of X, groups of Y; PAIRED: units of the pairs), a wavefront
//                           finds its pair by binary search and writes P to the unit's slot of d_work, and a merge kernel (a thread per
//                           pair) adds a pair's partials in ascending (slice, group).  The X diagrams go in groups of consecutive
//                           diagrams, as many as d_work holds: a smaller workspace means more launches and the same bits, because
//                           R = +0.0 + P of a single unit is P (no partial sum is ever -0.0).
//
// The VJP gives a lane one point p of X and keeps (gb, gd, gw) in registers; the points q pass by as readlanes, Y's diagrams ascending.
// ALL mode: a wavefront takes 64 consecutive ROWS of X whatever diagrams they belong to (every diagram of X meets the same Y, only the
// upstream G[i, j] is per lane), so small diagrams still fill the lanes.  PAIRED mode: a wavefront takes one 64-point chunk of one X_i
// (by binary search in the chunk prefix when a diagram can have more than one).  Neither splits the walk over Y: a row's cost is
// the number of points of Y it meets, whatever X holds (DESIGN.md 6.17 names the shape that loses by it).
#include "tlc_common.h"

#include <stdlib.h>

#include <cmath>

#include "scratch_layouts.h"

namespace {

#define DG_BS 256
#define DG_WAVES (DG_BS / 64)
#define DG_MAX_GRID 4096                     // workgroups of a grid-stride launch: 16 per CU
#define DG_SLICE TLC_DG_SLICE
#define DG_GROUP TLC_DG_GROUP
#define DG_FLAGS (TLC_DG_ALL | TLC_DG_PAIRED | TLC_DG_SYMMETRIC | TLC_DG_MIRROR)
static_assert(DG_SLICE == TlcDgmGramScratch::SLICE && DG_GROUP == TlcDgmGramScratch::GROUP && TlcDgmGramScratch::CHUNK == 64,
              "the header's cuts are the layout's");
static_assert(DG_GROUP % 64 == 0 && DG_SLICE % 64 == 0, "whole chunks");

__device__ __forceinline__ bool dg_finite(double x) {
    return ((unsigned long long)__double_as_longlong(x) & 0x7FF0000000000000ull) != 0x7FF0000000000000ull;
}
__device__ __forceinline__ double dg_nan() { return __longlong_as_double(0x7FF8000000000000ll); }
__device__ __forceinline__ double dg_readlane_f64(double v, int l) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, l);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), l);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
__device__ __forceinline__ long long dg_uniform(long long v) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(unsigned long long)v);
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)((unsigned long long)v >> 32));
    return (long long)(((unsigned long long)hi << 32) | lo);
}
// the largest i in [0, n) with pre[i] <= v (pre ascending, pre[0] <= v)
__device__ __forceinline__ int dg_search(const long long* pre, int n, long long v) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (pre[mid] <= v) lo = mid;
        else hi = mid;
    }
    return lo;
}

struct DgSide {
    const long long* offs;
    const double* pts;       // [sum n, 2]
    const double* w;         // [sum n] or null
};

// ---- status: a wavefront per diagram -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DG_BS) void dg_status_kernel(int n_dgms, DgSide S, unsigned char* status) {
    const int lane = (int)(threadIdx.x & 63);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (long long d = (long long)blockIdx.x * DG_WAVES + wave; d < n_dgms; d += (long long)gridDim.x * DG_WAVES) {
        const long long o0 = S.offs[d], n = S.offs[d + 1] - o0;
        bool bad = false;
        for (long long p = lane; p < n; p += 64) {
            bad |= !(dg_finite(S.pts[2 * (o0 + p)]) && dg_finite(S.pts[2 * (o0 + p) + 1]));
            if (S.w) bad |= !dg_finite(S.w[o0 + p]);
        }
        const bool any = __ballot(bad) != 0ull;
        if (lane == 0) status[d] = any ? 3 : 0;
    }
}

// ---- the forward -----------------------------------------------------------------------------------------------------------------------
struct DgArgs {
    int nx, ny;
    DgSide X, Y;
    double ng, scale;        // ng = -gamma
    unsigned flags;
    double* out;
    const unsigned char* sx;
    const unsigned char* sy;
    int simple;              // every pair is one unit: unit u is pair u and stores its own entry
    const long long* xpre;   // ALL: the slice prefix of X [nx + 1]; PAIRED: the unit prefix of the pairs [nx + 1]
    const long long* ypre;   // ALL: the group prefix of Y [ny + 1]
    long long gtot;          // ALL: ypre[ny]
    long long u0, u1;        // the units of this launch
    double* partial;         // unit u writes partial[u - u0]
};

__device__ __forceinline__ void dg_store(const DgArgs& A, int i, int j, long long n, long long m, bool bad, double R) {
    const double v = bad ? dg_nan() : (n == 0 || m == 0) ? 0.0 : A.scale * R;
    if (A.flags & TLC_DG_PAIRED) { A.out[i] = v; return; }
    A.out[(long long)i * A.ny + j] = v;
    if (A.flags & TLC_DG_SYMMETRIC) A.out[(long long)j * A.ny + i] = v;
}

// P of one unit: rows [p0, p1) of X_i against rows [q0, q1) of Y_j (rows local to the diagrams at ox / oy); wave-uniform on return
template <bool MIRROR, bool WEIGHTS>
__device__ __forceinline__ double dg_unit(const DgArgs& A, long long ox, long long p0, long long p1, long long oy, long long q0, long long q1,
                                          int lane) {
    double P = 0.0;
    for (long long qc = q0; qc < q1; qc += 64) {
        const bool have = qc + lane < q1;
        double qb = 0.0, qd = 0.0, qw = 1.0;
        if (have) {
            qb = A.Y.pts[2 * (oy + qc + lane)];
            qd = A.Y.pts[2 * (oy + qc + lane) + 1];
            if (WEIGHTS && A.Y.w) qw = A.Y.w[oy + qc + lane];
        }
        double a = 0.0;
        for (long long pc = p0; pc < p1; pc += 64) {
            const int cnt = (int)(p1 - pc < 64 ? p1 - pc : 64);
            double xb = 0.0, xd = 0.0, xw = 1.0;
            if (lane < cnt) {
                xb = A.X.pts[2 * (ox + pc + lane)];
                xd = A.X.pts[2 * (ox + pc + lane) + 1];
                if (WEIGHTS && A.X.w) xw = A.X.w[ox + pc + lane];
            }
            for (int k = 0; k < cnt; ++k) {
                const double pb = dg_readlane_f64(xb, k), pd = dg_readlane_f64(xd, k);
                const double db = pb - qb, dd = pd - qd;
                double e = exp(A.ng * (db * db + dd * dd));
                if (MIRROR) {
                    const double mb = pb - qd, md = pd - qb;
                    e = e - exp(A.ng * (mb * mb + md * md));
                }
                double t = e;
                if (WEIGHTS) t = (dg_readlane_f64(xw, k) * qw) * e;
                a = a + t;
            }
        }
        if (!have) a = 0.0;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) a = a + __shfl_xor(a, d);
        P = P + dg_readlane_f64(a, 0);
    }
    return P;
}

template <bool MIRROR, bool WEIGHTS>
__global__ __launch_bounds__(DG_BS) void dg_unit_kernel(DgArgs A) {
    const int lane = (int)(threadIdx.x & 63);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const bool paired = (A.flags & TLC_DG_PAIRED) != 0;
    const long long stride = (long long)gridDim.x * DG_WAVES;
    for (long long u = A.u0 + (long long)blockIdx.x * DG_WAVES + wave; u < A.u1; u += stride) {
        int i, j;
        long long s = 0, g = 0;
        if (A.simple) {
            if (paired) i = j = (int)u;
            else { i = (int)(u / A.ny); j = (int)(u - (long long)i * A.ny); }
        } else if (paired) {
            i = j = dg_search(A.xpre, A.nx, u);
            const long long m = A.Y.offs[j + 1] - A.Y.offs[j], G = m > DG_GROUP ? (m + DG_GROUP - 1) / DG_GROUP : 1, r = u - A.xpre[i];
            s = r / G;
            g = r - s * G;
        } else {
            const long long srow = u / A.gtot, gcol = u - srow * A.gtot;
            i = dg_search(A.xpre, A.nx, srow);
            j = dg_search(A.ypre, A.ny, gcol);
            s = srow - A.xpre[i];
            g = gcol - A.ypre[j];
        }
        i = __builtin_amdgcn_readfirstlane(i);
        j = __builtin_amdgcn_readfirstlane(j);
        s = dg_uniform(s);
        g = dg_uniform(g);
        if ((A.flags & TLC_DG_SYMMETRIC) && j < i) continue;
        const long long ox = dg_uniform(A.X.offs[i]), n = dg_uniform(A.X.offs[i + 1]) - ox;
        const long long oy = dg_uniform(A.Y.offs[j]), m = dg_uniform(A.Y.offs[j + 1]) - oy;
        const bool bad = A.sx[i] == 3 || A.sy[j] == 3;
        double P = 0.0;
        if (!bad) {
            const long long p0 = s * DG_SLICE, q0 = g * DG_GROUP;
            P = dg_unit<MIRROR, WEIGHTS>(A, ox, p0, n - p0 < DG_SLICE ? n : p0 + DG_SLICE, oy, q0, m - q0 < DG_GROUP ? m : q0 + DG_GROUP, lane);
        }
        if (lane == 0) {
            if (A.simple) dg_store(A, i, j, n, m, bad, P);
            else A.partial[u - A.u0] = P;
        }
    }
}

// a thread per pair of the X diagrams [i0, i1): the pair's partials in ascending (slice, group)
__global__ __launch_bounds__(DG_BS) void dg_merge_kernel(DgArgs A, int i0, int i1) {
    const bool paired = (A.flags & TLC_DG_PAIRED) != 0;
    const long long pairs = paired ? (long long)(i1 - i0) : (long long)(i1 - i0) * A.ny;
    for (long long t = (long long)blockIdx.x * DG_BS + threadIdx.x; t < pairs; t += (long long)gridDim.x * DG_BS) {
        const int i = paired ? i0 + (int)t : i0 + (int)(t / A.ny);
        const int j = paired ? i : (int)(t - (long long)(i - i0) * A.ny);
        if ((A.flags & TLC_DG_SYMMETRIC) && j < i) continue;
        double R = 0.0;
        if (paired) {
            const double* P = A.partial + (A.xpre[i] - A.xpre[i0]);
            const long long cnt = A.xpre[i + 1] - A.xpre[i];
            for (long long k = 0; k < cnt; ++k) R = R + P[k];
        } else {
            const long long S = A.xpre[i + 1] - A.xpre[i], G = A.ypre[j + 1] - A.ypre[j];
            for (long long s = 0; s < S; ++s) {
                const double* P = A.partial + (A.xpre[i] - A.xpre[i0] + s) * A.gtot + A.ypre[j];
                for (long long g = 0; g < G; ++g) R = R + P[g];
            }
        }
        dg_store(A, i, j, A.X.offs[i + 1] - A.X.offs[i], A.Y.offs[j + 1] - A.Y.offs[j], A.sx[i] == 3 || A.sy[j] == 3, R);
    }
}

// ---- the VJP ------------------------------------------------------------------------------------------------------------------------
struct DgVjpArgs {
    int nx, ny;
    DgSide X, Y;
    double ng, scale, twog;  // twog = 2 * gamma
    unsigned flags;
    const unsigned char* sx;
    const unsigned char* sy;
    const double* gout;      // [nx, ny] or [nx]
    double* gpts;            // [sum n, 2]
    double* gw;              // [sum n] or null
    long long r0, r1;        // ALL: the rows of X
    int simple;              // PAIRED: no diagram of X has more than one chunk, unit u is diagram u
    const long long* cpre;   // PAIRED, else: the chunk prefix of X [nx + 1]
    long long units;
};

// (ib, id, iw) of the point (pb, pd) against the m points of Y from row oy (oy, m wave-uniform)
template <bool MIRROR, bool WEIGHTS>
__device__ __forceinline__ void dg_vjp_inner(const DgVjpArgs& A, long long oy, long long m, double pb, double pd, int lane, double& ib,
                                             double& id, double& iw) {
    ib = id = iw = 0.0;
    for (long long qc = 0; qc < m; qc += 64) {
        const int cnt = (int)(m - qc < 64 ? m - qc : 64);
        double yb = 0.0, yd = 0.0, yw = 1.0;
        if (lane < cnt) {
            yb = A.Y.pts[2 * (oy + qc + lane)];
            yd = A.Y.pts[2 * (oy + qc + lane) + 1];
            if (WEIGHTS && A.Y.w) yw = A.Y.w[oy + qc + lane];
        }
        for (int k = 0; k < cnt; ++k) {
            const double qb = dg_readlane_f64(yb, k), qd = dg_readlane_f64(yd, k);
            const double db = pb - qb, dd = pd - qd;
            double t1 = exp(A.ng * (db * db + dd * dd));
            if (WEIGHTS) t1 = dg_readlane_f64(yw, k) * t1;
            if (!MIRROR) {
                ib = ib - db * t1;
                id = id - dd * t1;
                iw = iw + t1;
            } else {
                const double mb = pb - qd, md = pd - qb;
                double t2 = exp(A.ng * (mb * mb + md * md));
                if (WEIGHTS) t2 = dg_readlane_f64(yw, k) * t2;
                ib = ib + (mb * t2 - db * t1);
                id = id + (md * t2 - dd * t1);
                iw = iw + (t1 - t2);
            }
        }
    }
}

template <bool WEIGHTS>
__device__ __forceinline__ void dg_vjp_store(const DgVjpArgs& A, long long r, bool bad, double pw, double gb, double gd, double gw) {
    const double c = WEIGHTS ? A.scale * pw : A.scale, c2 = c * A.twog;
    A.gpts[2 * r] = bad ? 0.0 : c2 * gb;
    A.gpts[2 * r + 1] = bad ? 0.0 : c2 * gd;
    if (A.gw) A.gw[r] = bad ? 0.0 : A.scale * gw;
}

// ALL: 64 consecutive rows of X per wavefront, every diagram of Y in turn
template <bool MIRROR, bool WEIGHTS>
__global__ __launch_bounds__(DG_BS) void dg_vjp_all_kernel(DgVjpArgs A) {
    const int lane = (int)(threadIdx.x & 63);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (long long u = (long long)blockIdx.x * DG_WAVES + wave; u < A.units; u += (long long)gridDim.x * DG_WAVES) {
        const long long r = A.r0 + u * 64 + lane;
        const bool have = r < A.r1;
        int i = 0;
        double pb = 0.0, pd = 0.0, pw = 1.0;
        if (have) {
            i = dg_search(A.X.offs, A.nx, r);
            pb = A.X.pts[2 * r];
            pd = A.X.pts[2 * r + 1];
            if (WEIGHTS && A.X.w) pw = A.X.w[r];
        }
        double gb = 0.0, gd = 0.0, gw = 0.0;
        for (int j = 0; j < A.ny; ++j) {
            if (A.sy[j] == 3) continue;
            const long long oy = dg_uniform(A.Y.offs[j]), m = dg_uniform(A.Y.offs[j + 1]) - oy;
            double ib, id, iw;
            dg_vjp_inner<MIRROR, WEIGHTS>(A, oy, m, pb, pd, lane, ib, id, iw);
            const double G = have ? A.gout[(long long)i * A.ny + j] : 0.0;
            gb = gb + G * ib;
            gd = gd + G * id;
            gw = gw + G * iw;
        }
        if (have) dg_vjp_store<WEIGHTS>(A, r, A.sx[i] == 3, pw, gb, gd, gw);
    }
}

// PAIRED: one 64-point chunk of one X_i per wavefront, against Y_i
template <bool MIRROR, bool WEIGHTS>
__global__ __launch_bounds__(DG_BS) void dg_vjp_paired_kernel(DgVjpArgs A) {
    const int lane = (int)(threadIdx.x & 63);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (long long u = (long long)blockIdx.x * DG_WAVES + wave; u < A.units; u += (long long)gridDim.x * DG_WAVES) {
        const int i = __builtin_amdgcn_readfirstlane(A.simple ? (int)u : dg_search(A.cpre, A.nx, u));
        const long long c = A.simple ? 0 : dg_uniform(u - A.cpre[i]);
        const long long ox = dg_uniform(A.X.offs[i]), n = dg_uniform(A.X.offs[i + 1]) - ox;
        const long long p = c * 64 + lane, r = ox + p;
        const bool have = p < n;
        double pb = 0.0, pd = 0.0, pw = 1.0;
        if (have) {
            pb = A.X.pts[2 * r];
            pd = A.X.pts[2 * r + 1];
            if (WEIGHTS && A.X.w) pw = A.X.w[r];
        }
        double gb = 0.0, gd = 0.0, gw = 0.0;
        if (A.sy[i] != 3 && n > 0) {
            const long long oy = dg_uniform(A.Y.offs[i]), m = dg_uniform(A.Y.offs[i + 1]) - oy;
            double ib, id, iw;
            dg_vjp_inner<MIRROR, WEIGHTS>(A, oy, m, pb, pd, lane, ib, id, iw);
            const double G = A.gout[i];
            gb = gb + G * ib;
            gd = gd + G * id;
            gw = gw + G * iw;
        }
        if (have) dg_vjp_store<WEIGHTS>(A, r, A.sx[i] == 3, pw, gb, gd, gw);
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------
unsigned dg_grid(long long items) { return (unsigned)(items < 1 ? 1 : items > DG_MAX_GRID ? DG_MAX_GRID : items); }

// what the three entries check before a pointer is read; TLC_OK or the refusal
int dg_check_sizes(const char* fn, int32_t nx, int32_t ny, int64_t max_nx_points, int64_t max_ny_points, uint32_t flags) {
    if (nx < 0 || ny < 0 || max_nx_points < 0 || max_ny_points < 0) { tlc_set_error("%s: negative size", fn); return TLC_ERR_INVALID_ARG; }
    if (flags & ~DG_FLAGS) { tlc_set_error("%s: unknown flag bits %#x", fn, flags & ~DG_FLAGS); return TLC_ERR_INVALID_ARG; }
    const bool all = (flags & TLC_DG_ALL) != 0, paired = (flags & TLC_DG_PAIRED) != 0;
    if (all == paired) { tlc_set_error("%s: exactly one of TLC_DG_ALL and TLC_DG_PAIRED", fn); return TLC_ERR_INVALID_ARG; }
    if (paired && nx != ny) { tlc_set_error("%s: TLC_DG_PAIRED with nx = %d and ny = %d", fn, nx, ny); return TLC_ERR_INVALID_ARG; }
    if ((flags & TLC_DG_SYMMETRIC) && !all) { tlc_set_error("%s: TLC_DG_SYMMETRIC without TLC_DG_ALL", fn); return TLC_ERR_INVALID_ARG; }
    if ((flags & TLC_DG_SYMMETRIC) && (nx != ny || max_nx_points != max_ny_points)) {
        tlc_set_error("%s: TLC_DG_SYMMETRIC with different sizes of X and Y", fn);
        return TLC_ERR_INVALID_ARG;
    }
    return TLC_OK;
}

struct DgCall {
    int32_t nx, ny;
    const int64_t *x_offs, *y_offs;
    const double *x_pts, *x_w, *y_pts, *y_w;
    double gamma, scale;
    uint32_t flags;
    int64_t max_nx_points, max_ny_points;
    void* d_work;
    int64_t work_bytes;
};

// the refusals of both launching entries that need no read-back; *done: nothing to do (an empty batch)
int dg_check_call(const char* fn, const DgCall& c, const TlcDgmGramScratch& S, int64_t need, bool* done) {
    *done = false;
    const int rc = dg_check_sizes(fn, c.nx, c.ny, c.max_nx_points, c.max_ny_points, c.flags);
    if (rc != TLC_OK) return rc;
    if (!(std::isfinite(c.gamma) && c.gamma > 0.0)) { tlc_set_error("%s: gamma should be finite and > 0", fn); return TLC_ERR_INVALID_ARG; }
    if (!std::isfinite(c.scale)) { tlc_set_error("%s: scale should be finite", fn); return TLC_ERR_INVALID_ARG; }
    if (c.work_bytes < 0) { tlc_set_error("%s: negative size", fn); return TLC_ERR_INVALID_ARG; }
    if (c.nx == 0 || c.ny == 0) { *done = true; return TLC_OK; }
    if (!c.x_offs || !c.y_offs || (c.max_nx_points > 0 && !c.x_pts) || (c.max_ny_points > 0 && !c.y_pts)) {
        tlc_set_error("%s: null pointer", fn);
        return TLC_ERR_INVALID_ARG;
    }
    if ((c.flags & TLC_DG_SYMMETRIC) && (c.x_offs != c.y_offs || c.x_pts != c.y_pts || c.x_w != c.y_w)) {
        tlc_set_error("%s: TLC_DG_SYMMETRIC with different X and Y buffers", fn);
        return TLC_ERR_INVALID_ARG;
    }
    if (S.least >= TlcDgmGramScratch::SAT) { tlc_set_error("%s: the workspace of these sizes is beyond int64", fn); return TLC_ERR_INVALID_ARG; }
    if (c.work_bytes < need || (need > 0 && !c.d_work)) {
        if (!c.d_work && c.work_bytes >= need) tlc_set_error("%s: null pointer", fn);
        else tlc_set_error("%s: d_work holds %lld bytes; these sizes need %lld (tlc_dgm_gram_work_bytes)", fn, (long long)c.work_bytes,
                           (long long)need);
        return TLC_ERR_INVALID_ARG;
    }
    return TLC_OK;
}

// the offsets of both sides, read back once
struct DgHost {
    int64_t* offs = nullptr;     // X's [nx + 1], then Y's [ny + 1]
    int64_t* pre = nullptr;      // what the entry uploads
    ~DgHost() { free(offs); free(pre); }
};
int dg_check_offsets(const char* fn, const char* side, const int64_t* o, int32_t n, int64_t max_points) {
    if (o[0] < 0) { tlc_set_error("%s: negative offset of %s", fn, side); return TLC_ERR_INVALID_ARG; }
    for (int32_t d = 0; d < n; ++d) {
        const long long k = o[d + 1] - o[d];
        if (k < 0) { tlc_set_error("%s: the offsets of diagram %d of %s decrease", fn, d, side); return TLC_ERR_INVALID_ARG; }
        if (k > max_points) {
            tlc_set_error("%s: diagram %d of %s has %lld points, its max_points is %lld", fn, d, side, k, (long long)max_points);
            return TLC_ERR_INVALID_ARG;
        }
    }
    return TLC_OK;
}
int dg_read_back(const char* fn, DgHost& H, const DgCall& c, hipStream_t st) {
    const size_t bx = (size_t)c.nx + 1, by = (size_t)c.ny + 1;
    H.offs = (int64_t*)malloc((bx + by) * sizeof(int64_t));
    if (!H.offs) { tlc_set_error("%s: out of host memory", fn); return TLC_ERR_OUT_OF_MEMORY; }
    if (hipMemcpyAsync(H.offs, c.x_offs, bx * sizeof(int64_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(H.offs + bx, c.y_offs, by * sizeof(int64_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) {
        tlc_set_error("%s: reading the offsets failed: %s", fn, hipGetErrorString(hipGetLastError()));
        return TLC_ERR_HIP;
    }
    const int rx = dg_check_offsets(fn, "X", H.offs, c.nx, c.max_nx_points);
    return rx != TLC_OK ? rx : dg_check_offsets(fn, "Y", H.offs + bx, c.ny, c.max_ny_points);
}
// count entries of a host prefix -> the workspace at byte offset `at`; the host copy is free to go afterwards
int dg_upload(const char* fn, const int64_t* src, char* w, int64_t at, size_t count, hipStream_t st) {
    if (hipMemcpyAsync(w + at, src, count * sizeof(int64_t), hipMemcpyHostToDevice, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
        tlc_set_error("%s: uploading the unit prefix failed: %s", fn, hipGetErrorString(hipGetLastError()));
        return TLC_ERR_HIP;
    }
    return TLC_OK;
}

template <bool MIRROR, bool WEIGHTS>
void dg_launch_units(const DgArgs& A, hipStream_t st) {
    hipLaunchKernelGGL((dg_unit_kernel<MIRROR, WEIGHTS>), dim3(dg_grid((A.u1 - A.u0 + DG_WAVES - 1) / DG_WAVES)), dim3(DG_BS), 0, st, A);
}
void dg_units(const DgArgs& A, bool weights, hipStream_t st) {
    const bool mirror = (A.flags & TLC_DG_MIRROR) != 0;
    if (mirror && weights) dg_launch_units<true, true>(A, st);
    else if (mirror) dg_launch_units<true, false>(A, st);
    else if (weights) dg_launch_units<false, true>(A, st);
    else dg_launch_units<false, false>(A, st);
}

template <bool MIRROR, bool WEIGHTS>
void dg_launch_vjp(const DgVjpArgs& A, hipStream_t st) {
    const dim3 grid(dg_grid((A.units + DG_WAVES - 1) / DG_WAVES));
    if (A.flags & TLC_DG_PAIRED) hipLaunchKernelGGL((dg_vjp_paired_kernel<MIRROR, WEIGHTS>), grid, dim3(DG_BS), 0, st, A);
    else hipLaunchKernelGGL((dg_vjp_all_kernel<MIRROR, WEIGHTS>), grid, dim3(DG_BS), 0, st, A);
}

}  // namespace

extern "C" int64_t tlc_dgm_gram_work_bytes(int32_t nx, int32_t ny, int64_t max_nx_points, int64_t max_ny_points, uint32_t flags,
                                           int64_t* least) {
    if (least) *least = 0;
    if (dg_check_sizes(__func__, nx, ny, max_nx_points, max_ny_points, flags) != TLC_OK) return -1;
    const TlcDgmGramScratch S(nx, ny, max_nx_points, max_ny_points, (flags & TLC_DG_PAIRED) != 0, TlcCarver());
    if (S.least >= TlcDgmGramScratch::SAT) { tlc_set_error("%s: the workspace of these sizes is beyond int64", __func__); return -1; }
    if (least) *least = S.least;
    return S.total;
}

extern "C" int tlc_dgm_gram(int32_t nx, const int64_t* x_offs, const double* x_pts, const double* x_w, int32_t ny, const int64_t* y_offs,
                            const double* y_pts, const double* y_w, double gamma, double scale, uint32_t flags, int64_t max_nx_points,
                            int64_t max_ny_points, double* d_out, uint8_t* d_status_x, uint8_t* d_status_y, void* d_work,
                            int64_t work_bytes, void* stream) {
    const DgCall c{nx, ny, x_offs, y_offs, x_pts, x_w, y_pts, y_w, gamma, scale, flags, max_nx_points, max_ny_points, d_work, work_bytes};
    const bool paired = (flags & TLC_DG_PAIRED) != 0;
    const TlcDgmGramScratch S(nx, ny, max_nx_points, max_ny_points, paired, TlcCarver());
    bool done;
    const int rc = dg_check_call(__func__, c, S, S.wide ? S.least : 0, &done);       // (the chunk prefix in *least is the VJP's)
    if (rc != TLC_OK || done) return rc;
    TLC_REQUIRE(d_out && d_status_x && d_status_y, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    DgHost H;
    const int rb = dg_read_back(__func__, H, c, st);
    if (rb != TLC_OK) return rb;
    const int64_t *hx = H.offs, *hy = H.offs + nx + 1;
    const DgSide X{(const long long*)x_offs, x_pts, x_w}, Y{(const long long*)y_offs, y_pts, y_w};
    hipLaunchKernelGGL(dg_status_kernel, dim3(dg_grid(((long long)nx + DG_WAVES - 1) / DG_WAVES)), dim3(DG_BS), 0, st, nx, X, d_status_x);
    hipLaunchKernelGGL(dg_status_kernel, dim3(dg_grid(((long long)ny + DG_WAVES - 1) / DG_WAVES)), dim3(DG_BS), 0, st, ny, Y, d_status_y);
    DgArgs A{nx, ny, X, Y, -gamma, scale, flags, d_out, d_status_x, d_status_y, 1, nullptr, nullptr, 0, 0, 0, nullptr};
    const bool weights = x_w || y_w;
    if (!S.wide) {
        A.u1 = paired ? (long long)nx : (long long)nx * ny;
        dg_units(A, weights, st);
        TLC_HIP_CHECK(hipGetLastError());
        return TLC_OK;
    }
    // the unit prefixes: ALL the slices of X and the groups of Y, PAIRED the units of the pairs
    const size_t bx = (size_t)nx + 1, by = (size_t)ny + 1;
    H.pre = (int64_t*)malloc((bx + by) * sizeof(int64_t));
    if (!H.pre) { tlc_set_error("%s: out of host memory", __func__); return TLC_ERR_OUT_OF_MEMORY; }
    int64_t *px = H.pre, *py = H.pre + bx;
    px[0] = py[0] = 0;
    for (int32_t j = 0; j < ny; ++j) py[j + 1] = py[j] + TlcDgmGramScratch::groups_of(hy[j + 1] - hy[j]);
    for (int32_t i = 0; i < nx; ++i) {
        const int64_t s = TlcDgmGramScratch::slices_of(hx[i + 1] - hx[i]);
        px[i + 1] = px[i] + (paired ? s * (py[i + 1] - py[i]) : s);
    }
    char* w = tlc_align256(d_work);
    const int up = dg_upload(__func__, px, w, S.xpre, bx + by, st);      // (S.ypre lies right behind S.xpre's nx + 1 entries)
    if (up != TLC_OK) return up;
    A.simple = 0;
    A.xpre = (const long long*)(w + S.xpre);
    A.ypre = (const long long*)(w + S.ypre);
    A.gtot = py[ny];
    A.partial = (double*)(w + S.partial);
    const int64_t cap = S.slots_in(work_bytes);
    const int64_t per_row = paired ? 1 : A.gtot;                 // slots per unit of px
    for (int32_t i0 = 0; i0 < nx;) {
        int32_t i1 = i0 + 1;
        while (i1 < nx && (px[i1 + 1] - px[i0]) * per_row <= cap) ++i1;
        if ((px[i1] - px[i0]) * per_row > cap) { tlc_set_error("%s: d_work does not hold diagram %d of X", __func__, i0); return TLC_ERR_INVALID_ARG; }
        A.u0 = px[i0] * per_row;
        A.u1 = px[i1] * per_row;
        dg_units(A, weights, st);
        const long long pairs = paired ? (long long)(i1 - i0) : (long long)(i1 - i0) * ny;
        hipLaunchKernelGGL(dg_merge_kernel, dim3(dg_grid((pairs + DG_BS - 1) / DG_BS)), dim3(DG_BS), 0, st, A, i0, i1);
        i0 = i1;
    }
    TLC_HIP_CHECK(hipGetLastError());
    return TLC_OK;
}

extern "C" int tlc_dgm_gram_vjp(int32_t nx, const int64_t* x_offs, const double* x_pts, const double* x_w, int32_t ny,
                                const int64_t* y_offs, const double* y_pts, const double* y_w, double gamma, double scale, uint32_t flags,
                                int64_t max_nx_points, int64_t max_ny_points, const uint8_t* d_status_x, const uint8_t* d_status_y,
                                const double* d_grad_out, double* d_grad_pts_x, double* d_grad_w_x, void* d_work, int64_t work_bytes,
                                void* stream) {
    const DgCall c{nx, ny, x_offs, y_offs, x_pts, x_w, y_pts, y_w, gamma, scale, flags, max_nx_points, max_ny_points, d_work, work_bytes};
    const bool paired = (flags & TLC_DG_PAIRED) != 0;
    const TlcDgmGramScratch S(nx, ny, max_nx_points, max_ny_points, paired, TlcCarver());
    bool done;
    const int rc = dg_check_call(__func__, c, S, paired && max_nx_points > TlcDgmGramScratch::CHUNK ? S.least : 0, &done);
    if (rc != TLC_OK) return rc;
    TLC_REQUIRE((x_w == nullptr) == (d_grad_w_x == nullptr), "d_grad_w_x goes with x_w");
    if (nx == 0) return TLC_OK;
    TLC_REQUIRE(x_offs, "null pointer");
    TLC_REQUIRE(max_nx_points == 0 || (x_pts && d_grad_pts_x), "null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (done) {
        // ny == 0: every row is written, with zeros; the rows are X's, so its offsets alone are read
        int64_t ends[2];
        if (hipMemcpyAsync(&ends[0], x_offs, sizeof(int64_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipMemcpyAsync(&ends[1], x_offs + nx, sizeof(int64_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess) {
            tlc_set_error("%s: reading the offsets failed: %s", __func__, hipGetErrorString(hipGetLastError()));
            return TLC_ERR_HIP;
        }
        TLC_REQUIRE(ends[0] >= 0 && ends[1] >= ends[0], "the offsets of X decrease");
        const size_t rows = (size_t)(ends[1] - ends[0]);
        if (rows && d_grad_pts_x) TLC_HIP_CHECK(hipMemsetAsync(d_grad_pts_x + 2 * ends[0], 0, rows * 16, st));
        if (rows && d_grad_w_x) TLC_HIP_CHECK(hipMemsetAsync(d_grad_w_x + ends[0], 0, rows * 8, st));
        return TLC_OK;
    }
    TLC_REQUIRE(d_status_x && d_status_y && d_grad_out, "null pointer");
    DgHost H;
    const int rb = dg_read_back(__func__, H, c, st);
    if (rb != TLC_OK) return rb;
    const int64_t* hx = H.offs;
    const DgSide X{(const long long*)x_offs, x_pts, x_w}, Y{(const long long*)y_offs, y_pts, y_w};
    DgVjpArgs A{nx, ny, X, Y, -gamma, scale, 2.0 * gamma, flags, d_status_x, d_status_y, d_grad_out, d_grad_pts_x, d_grad_w_x,
                hx[0], hx[nx], 1, nullptr, 0};
    if (!paired) {
        A.units = (hx[nx] - hx[0] + 63) / 64;
    } else if (max_nx_points <= TlcDgmGramScratch::CHUNK) {
        A.units = nx;
    } else {
        const size_t bx = (size_t)nx + 1;
        H.pre = (int64_t*)malloc(bx * sizeof(int64_t));
        if (!H.pre) { tlc_set_error("%s: out of host memory", __func__); return TLC_ERR_OUT_OF_MEMORY; }
        H.pre[0] = 0;
        for (int32_t i = 0; i < nx; ++i) H.pre[i + 1] = H.pre[i] + TlcDgmGramScratch::chunks_of(hx[i + 1] - hx[i]);
        char* w = tlc_align256(d_work);
        const int up = dg_upload(__func__, H.pre, w, S.xpre, bx, st);
        if (up != TLC_OK) return up;
        A.simple = 0;
        A.cpre = (const long long*)(w + S.xpre);
        A.units = H.pre[nx];
    }
    if (A.units > 0) {
        const bool mirror = (flags & TLC_DG_MIRROR) != 0, weights = x_w || y_w;
        if (mirror && weights) dg_launch_vjp<true, true>(A, st);
        else if (mirror) dg_launch_vjp<true, false>(A, st);
        else if (weights) dg_launch_vjp<false, true>(A, st);
        else dg_launch_vjp<false, false>(A, st);
    }
    TLC_HIP_CHECK(hipGetLastError());
    return TLC_OK;
}

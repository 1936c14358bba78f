// dist_filt.hip -- the distance filtration of a packed batch (tlc_dist_filtration) and its vector-Jacobian product in the edge weights
// (tlc_dist_filtration_vjp).  gfx950, fp64, -ffp-contract=off: the path sums must not fuse.  The contract is in include/tlcgnn.h.
//
// Value: for node x and root r, D_r[x] = the minimum over paths x -> r of the left-to-right fp64 sum that starts at x.  The
// route is the tier kernels' (pd_pipeline.hip): a root-sourced Bellman-Ford on the u64 bit patterns (integer atomicMin: positive doubles
// order like their bits), the directed entries that are tight within 1e-10 (1 + d_max), one lane per x walking its tight chain and adding
// the weights in the reference's order, and a Bellman-Ford sourced at x for every x whose chain is not unique.  Every fixpoint is unique,
// so the bits depend neither on the class, nor on the order of the atomics, nor on the workspace.
//
// Launches: df_check_kernel (a wavefront per graph: offsets, roots, ids, loops, weights, repeated edges by a hash in d_work; bins the
// graph), df_group_kernel<64, 64> and <256, 2048> (a wavefront / a workgroup per graph, everything in LDS, weights streamed from L2),
// and for the whole-device class one launch per step and per Bellman-Ford round over all edges (nodes) of the batch, state in d_work.
// Every loop has a bound the graph fixes: n - 1 rounds, n chain steps, 2 m hash probes.
// The VJP (df_vjp_kernel<64> / <256>, a group per graph, state in d_work) rebuilds the raw values along the tree d_parent, puts the
// descriptor's and the normalisation's coefficients on the nodes, builds every node's child list in ascending id (a scan and a stable
// chunk-by-chunk fill) and pulls the subtree sums level by level from the deepest: fixed summation orders, no floating-point atomics.
#include "tlc_common.h"
#include "scratch_layouts.h"

#include <algorithm>

#define DF_WAVE_N TLC_DIST_WAVE_NMAX
#define DF_WG_N TLC_DIST_WG_NMAX
#define DF_WG_M TLC_DIST_WG_MMAX
#define DF_INF 0x7ff0000000000000ull
#define DF_FLAGS (TLC_DESC_MASK | TLC_INCLUDE_ROOTS | TLC_NORM_EPS | TLC_UNREACHABLE_100 | TLC_NO_NORM)
#define DF_CHECK_EVERY 8            // whole-device rounds between two reads of the "changed" words
// control words (int) at the head of d_work
#define DF_H_COUNT 0                // [3] graphs per class
#define DF_H_TICKET 3               // [3]
#define DF_H_CHANGED 6
#define DF_H_NAMB 7
#define DF_H_MAXN 8
#define DF_H_MAXM 9
#define DF_H_FALLBACKS 16           // u64 at byte TLC_DIST_WORK_FALLBACKS_OFF
#define DF_H_GCHANGED 256           // [MAX_GROUPS]
static_assert(DF_H_FALLBACKS * 4 == TLC_DIST_WORK_FALLBACKS_OFF, "the header names the byte offset of the fallback count");
static_assert((DF_H_GCHANGED + TlcDistFiltScratch::MAX_GROUPS) * 4 <= TlcDistFiltScratch::HEAD, "control words fit the head");

namespace {

typedef unsigned long long u64;

__device__ __forceinline__ double df_val(u64 b) { return __longlong_as_double((long long)b); }
__device__ __forceinline__ u64 df_bits(double v) { return (u64)__double_as_longlong(v); }
// the descriptor over the two distances (riccidist2dgm.py:47-49); one root: the first distance
__device__ __forceinline__ double df_desc(unsigned desc, bool single, double d1, double d2) {
    if (single) return d1;
    return desc == 0u ? d1 + d2 : (desc == TLC_DESC_MIN ? (d2 < d1 ? d2 : d1) : (d2 > d1 ? d2 : d1));
}

struct DfArgs {
    long long B, N, M;
    const long long* node_ptr;
    const long long* edge_ptr;
    const int* edges;
    const double* w;
    const int* roots;
    unsigned flags;
    double* f;
    unsigned char* status;
    int* parent;        // [2][N] or null
    int* head;
    int* lists;         // [3][B]
    u64* hash;          // [2 M]
    int* egraph;        // [M]
    int* ngraph;        // [N]: the owner graph of every node of the whole-device class, -1 elsewhere; null unless the batch can hold one
};

// ---- validation and binning: a wavefront per graph ------------------------------------------------------------------------------------
// vjp: two classes only (0: up to 64 nodes, 1: the rest)
__global__ __launch_bounds__(256) void df_check_kernel(DfArgs a, int vjp) {
    const int lane = tlc_lane();
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6, waves = ((long long)gridDim.x * blockDim.x) >> 6;
    for (long long g = wave; g < a.B; g += waves) {
        const long long n0 = a.node_ptr[g], n1 = a.node_ptr[g + 1], e0 = a.edge_ptr[g], e1 = a.edge_ptr[g + 1];
        const long long n = n1 - n0, m = e1 - e0;
        bool bad = n0 < 0 || n1 < n0 || n1 > a.N || e0 < 0 || e1 < e0 || e1 > a.M;
        if (!bad) bad = (n == 0 && m > 0) || (n > 0 && m > (n & 1 ? n * ((n - 1) >> 1) : (n >> 1) * (n - 1)));
        if (!bad && n > 0) {
            const int r0 = a.roots[2 * g], r1 = a.roots[2 * g + 1];
            bad = r0 < 0 || r0 >= n || r1 < -1 || r1 >= n;
        }
        if (bad || n == 0) {
            if (lane == 0) a.status[g] = bad ? TLC_ST_BAD_INPUT : TLC_ST_OK;
            continue;
        }
        u64* tab = a.hash + 2 * e0;
        const long long slots = 2 * m;
        for (long long e = lane; e < m; e += 64) {
            const int u = a.edges[2 * (e0 + e)], v = a.edges[2 * (e0 + e) + 1];
            const double w = a.w[e0 + e];
            if ((unsigned)u >= (unsigned)n || (unsigned)v >= (unsigned)n || u == v || !(w > 0.0) || !(w < __longlong_as_double((long long)DF_INF))) { bad = true; continue; }
            const u64 key = ((u64)(unsigned)(u < v ? u : v) << 32 | (u64)(unsigned)(u < v ? v : u)) + 1ull;
            long long s = (long long)((key * 0x9E3779B97F4A7C15ull) % (u64)slots);
            for (long long probe = 0; probe < slots; ++probe) {
                const u64 old = atomicCAS(&tab[s], 0ull, key);
                if (old == 0ull) break;
                if (old == key) { bad = true; break; }
                s = s + 1 == slots ? 0 : s + 1;
            }
        }
        bad = __any(bad);
        int cls = n <= DF_WAVE_N ? 0 : ((vjp || (n <= DF_WG_N && m <= DF_WG_M)) ? 1 : 2);
        if (!bad && cls == 2 && !vjp) {
            for (long long e = lane; e < m; e += 64) a.egraph[e0 + e] = (int)g;
            for (long long k = lane; k < n; k += 64) a.ngraph[n0 + k] = (int)g;
        }
        if (lane == 0) {
            a.status[g] = bad ? TLC_ST_BAD_INPUT : TLC_ST_OK;
            if (!bad) {
                a.lists[(long long)cls * a.B + atomicAdd(&a.head[DF_H_COUNT + cls], 1)] = (int)g;
                if (cls == 2) { atomicMax(&a.head[DF_H_MAXN], (int)n); atomicMax(&a.head[DF_H_MAXM], (int)m); }
            }
        }
    }
}

// ---- the wavefront and the workgroup class: a group of W threads per graph, state in LDS ---------------------------------------------
// du u64[NMAX] (later the raw values q) | dv u64[NMAX] (later the fallback's distances) | cntU, cntV, nxtU, nxtV u32[NMAX] | amb int[NMAX]
// | ctl int[4] | red u64[2]
constexpr size_t df_group_lds(int nmax) { return (size_t)nmax * (8 + 8 + 4 * 4 + 4) + 16 + 16; }

// rounds of relaxation over the undirected edges until nothing changes, n - 1 at the most (one more finds "nothing changed")
template <int W>
__device__ __forceinline__ void df_group_bf(u64* d0, u64* d1, bool two, int n, int m, const int* __restrict__ ed, const double* __restrict__ ew, int* ctl) {
    const int tid = (int)threadIdx.x;
    for (int round = 0; round < n; ++round) {
        if (tid == 0) ctl[0] = 0;
        __syncthreads();
        bool ch = false;
        for (int e = tid; e < m; e += W) {
            const int a = ed[2 * e], b = ed[2 * e + 1];
            const double w = ew[e];
            {
                const u64 xa = d0[a], xb = d0[b];
                if (xa != DF_INF) { const u64 s = df_bits(df_val(xa) + w); if (s < xb) ch |= atomicMin(&d0[b], s) > s; }
                if (xb != DF_INF) { const u64 s = df_bits(df_val(xb) + w); if (s < xa) ch |= atomicMin(&d0[a], s) > s; }
            }
            if (two) {
                const u64 xa = d1[a], xb = d1[b];
                if (xa != DF_INF) { const u64 s = df_bits(df_val(xa) + w); if (s < xb) ch |= atomicMin(&d1[b], s) > s; }
                if (xb != DF_INF) { const u64 s = df_bits(df_val(xb) + w); if (s < xa) ch |= atomicMin(&d1[a], s) > s; }
            }
        }
        if (ch) ctl[0] = 1;
        __syncthreads();
        const int any = ctl[0];
        __syncthreads();
        if (!any) break;
    }
}

template <int W>
__device__ __forceinline__ double df_group_max(double v, u64* red) {
    if (threadIdx.x == 0) red[0] = 0ull;
    __syncthreads();
    if (v > 0.0) atomicMax(&red[0], df_bits(v));
    __syncthreads();
    const double r = df_val(red[0]);
    __syncthreads();
    return r;
}

template <int W, int NMAX>
__global__ __launch_bounds__(W) void df_group_kernel(DfArgs a, int cls) {
    extern __shared__ __align__(16) unsigned char df_lds[];
    u64* du = (u64*)df_lds;
    u64* dv = du + NMAX;
    unsigned* cntU = (unsigned*)(dv + NMAX);
    unsigned* cntV = cntU + NMAX;
    unsigned* nxtU = cntV + NMAX;
    unsigned* nxtV = nxtU + NMAX;
    int* amb = (int*)(nxtV + NMAX);
    int* ctl = amb + NMAX;
    u64* red = (u64*)(ctl + 4);
    const int tid = (int)threadIdx.x;
    const int count = a.head[DF_H_COUNT + cls];
    const unsigned desc = a.flags & TLC_DESC_MASK;
    for (;;) {
        __syncthreads();
        if (tid == 0) ctl[2] = atomicAdd(&a.head[DF_H_TICKET + cls], 1);
        __syncthreads();
        const int i = ctl[2];
        if (i >= count) break;
        const int g = a.lists[(long long)cls * a.B + i];
        const long long n0 = a.node_ptr[g], e0 = a.edge_ptr[g];
        const int n = (int)(a.node_ptr[g + 1] - n0), m = (int)(a.edge_ptr[g + 1] - e0);
        const int* ed = a.edges + 2 * e0;
        const double* ew = a.w + e0;
        const int lu = a.roots[2 * g];
        const bool single = a.roots[2 * g + 1] < 0 || desc == TLC_DESC_ROOT1;
        const int lv = single ? lu : a.roots[2 * g + 1];
        for (int k = tid; k < n; k += W) { du[k] = DF_INF; dv[k] = DF_INF; cntU[k] = 0xffffffffu; cntV[k] = 0xffffffffu; }
        if (tid == 0) ctl[1] = 0;
        __syncthreads();
        if (tid == 0) { du[lu] = 0ull; if (!single) dv[lv] = 0ull; }
        __syncthreads();
        df_group_bf<W>(du, dv, !single, n, m, ed, ew, ctl);
        // the tree: the lowest neighbour y with R[y] < R[x] and fl(R[y] + w) == R[x]
        for (int e = tid; e < m; e += W) {
            const int p = ed[2 * e], q = ed[2 * e + 1];
            const double w = ew[e];
            const u64 up = du[p], uq = du[q], vp = dv[p], vq = dv[q];
            if (uq < up && up != DF_INF && df_bits(df_val(uq) + w) == up) atomicMin(&cntU[p], (unsigned)q);
            if (up < uq && uq != DF_INF && df_bits(df_val(up) + w) == uq) atomicMin(&cntU[q], (unsigned)p);
            if (vq < vp && vp != DF_INF && df_bits(df_val(vq) + w) == vp) atomicMin(&cntV[p], (unsigned)q);
            if (vp < vq && vq != DF_INF && df_bits(df_val(vp) + w) == vq) atomicMin(&cntV[q], (unsigned)p);
        }
        __syncthreads();
        double dmx = 0.0;
        int unreach = 0;
        for (int k = tid; k < n; k += W) {
            if (a.parent) { a.parent[n0 + k] = (int)cntU[k]; a.parent[a.N + n0 + k] = (int)cntV[k]; }     // 0xffffffff is -1
            cntU[k] = 0u; cntV[k] = 0u;
            const u64 x = du[k], y = dv[k];
            unreach |= (x == DF_INF);
            if (x != DF_INF && df_val(x) > dmx) dmx = df_val(x);
            if (y != DF_INF && df_val(y) > dmx) dmx = df_val(y);
        }
        dmx = df_group_max<W>(dmx, red);
        const bool un = df_group_max<W>(unreach ? 1.0 : 0.0, red) != 0.0;
        int status = TLC_ST_OK;
        if (un && !(a.flags & TLC_UNREACHABLE_100)) status = TLC_ST_DISCONNECTED;
        if (status == TLC_ST_OK) {
            // tight entries x -> y: on a (near-)shortest path from x to the root
            const double tol = 1e-10 * (1.0 + dmx);
            for (int j = tid; j < 2 * m; j += W) {
                const int e = j >> 1;
                const int x = ed[2 * e + (j & 1)], y = ed[2 * e + 1 - (j & 1)];
                const double w = ew[e];
                if (x != lu) { const double s = (w + df_val(du[y])) - df_val(du[x]); if (s <= tol) { atomicAdd(&cntU[x], 1u); nxtU[x] = (unsigned)j; } }
                if (!single && x != lv) { const double s = (w + df_val(dv[y])) - df_val(dv[x]); if (s <= tol) { atomicAdd(&cntV[x], 1u); nxtV[x] = (unsigned)j; } }
            }
            __syncthreads();
            // the chain walks: the weights from x towards the root, left to right.  q aliases du: a lane reads only its own du[x], dv[x]
            double* q = (double*)du;
            double nrm = 0.0;
            for (int x = tid; x < n; x += W) {
                double fr = 0.0, dm = 0.0;
                bool am = false;
                if (x != lu && x != lv) {
                    double d1 = 0.0, d2 = 0.0;
                    int c = x, steps = 0;
                    if (du[x] == DF_INF) { d1 = 100.0; c = lu; }
                    while (c != lu) {
                        if (cntU[c] != 1u || ++steps > n) { am = true; break; }
                        const int j = (int)nxtU[c];
                        d1 = d1 + ew[j >> 1];
                        c = ed[2 * (j >> 1) + 1 - (j & 1)];
                    }
                    c = x; steps = 0;
                    if (single) c = lv;
                    else if (dv[x] == DF_INF) { d2 = 100.0; c = lv; }
                    while (!am && c != lv) {
                        if (cntV[c] != 1u || ++steps > n) { am = true; break; }
                        const int j = (int)nxtV[c];
                        d2 = d2 + ew[j >> 1];
                        c = ed[2 * (j >> 1) + 1 - (j & 1)];
                    }
                    fr = df_desc(desc, single, d1, d2);
                    dm = (desc == TLC_DESC_MIN && !single) ? (d2 > d1 ? d2 : d1) : fr;       // 'min' is divided by the maximum of 'max' (:51)
                }
                if (am) amb[atomicAdd(&ctl[1], 1)] = x;
                else { q[x] = fr; nrm = dm > nrm ? dm : nrm; }
            }
            __syncthreads();
            // the exact fallback: a Bellman-Ford sourced at x itself
            const int namb = ctl[1];
            for (int t = 0; t < namb; ++t) {
                const int x = amb[t];
                for (int k = tid; k < n; k += W) dv[k] = DF_INF;
                __syncthreads();
                if (tid == 0) dv[x] = 0ull;
                __syncthreads();
                df_group_bf<W>(dv, dv, false, n, m, ed, ew, ctl);
                if (tid == 0) {
                    const double e1 = dv[lu] == DF_INF ? 100.0 : df_val(dv[lu]);
                    const double e2 = dv[lv] == DF_INF ? 100.0 : df_val(dv[lv]);
                    const double fr = df_desc(desc, single, e1, e2);
                    const double dm = (desc == TLC_DESC_MIN && !single) ? (e2 > e1 ? e2 : e1) : fr;
                    q[x] = fr;
                    nrm = dm > nrm ? dm : nrm;
                }
                __syncthreads();
            }
            if (namb && tid == 0) atomicAdd((u64*)(a.head + DF_H_FALLBACKS), (u64)namb);
            double den = df_group_max<W>(nrm, red);
            if (a.flags & TLC_NO_NORM) den = 1.0;
            else if (a.flags & TLC_NORM_EPS) den = den + 1e-10;
            else if (den == 0.0) status = TLC_ST_ZERO_RANGE;
            if (status == TLC_ST_OK)
                for (int k = tid; k < n; k += W) a.f[n0 + k] = (a.flags & TLC_NO_NORM) ? q[k] : q[k] / den;
        }
        if (tid == 0 && status != TLC_ST_OK) a.status[g] = (unsigned char)status;
    }
}

// ---- the whole-device class: state in d_work, indexed by the batch's node and edge numbers ---------------------------------------------
struct DfDev {
    u64* R0; u64* R1; double* q; unsigned* cnt0; unsigned* cnt1; unsigned* nxt0; unsigned* nxt1; int* amb;
    u64* gmax; u64* gden; int* gstat;
    u64* slices; long long slice_len; int groups;
};

__global__ __launch_bounds__(256) void df_dev_init_kernel(DfArgs a, DfDev d) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.N || a.ngraph[i] < 0) return;
    const int g = a.ngraph[i];
    const int x = (int)(i - a.node_ptr[g]);
    const unsigned desc = a.flags & TLC_DESC_MASK;
    const int lu = a.roots[2 * g], lv = a.roots[2 * g + 1];
    const bool single = lv < 0 || desc == TLC_DESC_ROOT1;
    d.R0[i] = x == lu ? 0ull : DF_INF;
    d.R1[i] = (!single && x == lv) ? 0ull : DF_INF;
    d.cnt0[i] = 0u; d.cnt1[i] = 0u; d.q[i] = 0.0;
    if (a.parent) { a.parent[i] = -1; a.parent[a.N + i] = -1; }
    if (x == 0) { d.gmax[g] = 0ull; d.gden[g] = 0ull; d.gstat[g] = TLC_ST_OK; }
}

__global__ __launch_bounds__(256) void df_dev_relax_kernel(DfArgs a, DfDev d) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= a.M || a.egraph[e] < 0) return;
    const long long n0 = a.node_ptr[a.egraph[e]];
    const long long p = n0 + a.edges[2 * e], q = n0 + a.edges[2 * e + 1];
    const double w = a.w[e];
    bool ch = false;
    for (int r = 0; r < 2; ++r) {
        u64* R = r ? d.R1 : d.R0;
        const u64 xa = R[p], xb = R[q];
        if (xa != DF_INF) { const u64 s = df_bits(df_val(xa) + w); if (s < xb) ch |= atomicMin(&R[q], s) > s; }
        if (xb != DF_INF) { const u64 s = df_bits(df_val(xb) + w); if (s < xa) ch |= atomicMin(&R[p], s) > s; }
    }
    if (ch) a.head[DF_H_CHANGED] = 1;
}

// the tree (integer atomicMin on the caller's d_parent, held as unsigned: -1 is the largest) and the largest distance per graph
__global__ __launch_bounds__(256) void df_dev_parent_kernel(DfArgs a, DfDev d) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= a.M || a.egraph[e] < 0 || !a.parent) return;
    const long long n0 = a.node_ptr[a.egraph[e]];
    const int lp = a.edges[2 * e], lq = a.edges[2 * e + 1];
    const long long p = n0 + lp, q = n0 + lq;
    const double w = a.w[e];
    for (int r = 0; r < 2; ++r) {
        const u64* R = r ? d.R1 : d.R0;
        unsigned* par = (unsigned*)(a.parent + (r ? a.N : 0));
        const u64 up = R[p], uq = R[q];
        if (uq < up && up != DF_INF && df_bits(df_val(uq) + w) == up) atomicMin(&par[p], (unsigned)lq);
        if (up < uq && uq != DF_INF && df_bits(df_val(up) + w) == uq) atomicMin(&par[q], (unsigned)lp);
    }
}

__global__ __launch_bounds__(256) void df_dev_dmax_kernel(DfArgs a, DfDev d) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.N || a.ngraph[i] < 0) return;
    const int g = a.ngraph[i];
    const u64 x = d.R0[i], y = d.R1[i];
    if (x == DF_INF && !(a.flags & TLC_UNREACHABLE_100)) d.gstat[g] = TLC_ST_DISCONNECTED;
    u64 mx = 0ull;
    if (x != DF_INF) mx = x;
    if (y != DF_INF && y > mx) mx = y;
    if (mx) atomicMax(&d.gmax[g], mx);
}

__global__ __launch_bounds__(256) void df_dev_tight_kernel(DfArgs a, DfDev d) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long e = j >> 1;
    if (e >= a.M || a.egraph[e] < 0) return;
    const int g = a.egraph[e];
    const long long n0 = a.node_ptr[g];
    const unsigned desc = a.flags & TLC_DESC_MASK;
    const int lu = a.roots[2 * g];
    const bool single = a.roots[2 * g + 1] < 0 || desc == TLC_DESC_ROOT1;
    const int lv = single ? lu : a.roots[2 * g + 1];
    const int lx = a.edges[2 * e + (j & 1)];
    const long long x = n0 + lx, y = n0 + a.edges[2 * e + 1 - (j & 1)];
    const double w = a.w[e];
    const double tol = 1e-10 * (1.0 + df_val(d.gmax[g]));
    const unsigned jl = (unsigned)(j - 2 * a.edge_ptr[g]);
    if (lx != lu) { const double s = (w + df_val(d.R0[y])) - df_val(d.R0[x]); if (s <= tol) { atomicAdd(&d.cnt0[x], 1u); d.nxt0[x] = jl; } }
    if (!single && lx != lv) { const double s = (w + df_val(d.R1[y])) - df_val(d.R1[x]); if (s <= tol) { atomicAdd(&d.cnt1[x], 1u); d.nxt1[x] = jl; } }
}

__global__ __launch_bounds__(256) void df_dev_walk_kernel(DfArgs a, DfDev d) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.N || a.ngraph[i] < 0) return;
    const int g = a.ngraph[i];
    if (d.gstat[g] != TLC_ST_OK) return;
    const long long n0 = a.node_ptr[g], e0 = a.edge_ptr[g];
    const int n = (int)(a.node_ptr[g + 1] - n0);
    const int* ed = a.edges + 2 * e0;
    const double* ew = a.w + e0;
    const unsigned desc = a.flags & TLC_DESC_MASK;
    const int lu = a.roots[2 * g];
    const bool single = a.roots[2 * g + 1] < 0 || desc == TLC_DESC_ROOT1;
    const int lv = single ? lu : a.roots[2 * g + 1];
    const int x = (int)(i - n0);
    double fr = 0.0, dm = 0.0;
    bool am = false;
    if (x != lu && x != lv) {
        double d1 = 0.0, d2 = 0.0;
        int c = x, steps = 0;
        if (d.R0[i] == DF_INF) { d1 = 100.0; c = lu; }
        while (c != lu) {
            if (d.cnt0[n0 + c] != 1u || ++steps > n) { am = true; break; }
            const int j = (int)d.nxt0[n0 + c];
            d1 = d1 + ew[j >> 1];
            c = ed[2 * (j >> 1) + 1 - (j & 1)];
        }
        c = x; steps = 0;
        if (single) c = lv;
        else if (d.R1[i] == DF_INF) { d2 = 100.0; c = lv; }
        while (!am && c != lv) {
            if (d.cnt1[n0 + c] != 1u || ++steps > n) { am = true; break; }
            const int j = (int)d.nxt1[n0 + c];
            d2 = d2 + ew[j >> 1];
            c = ed[2 * (j >> 1) + 1 - (j & 1)];
        }
        fr = df_desc(desc, single, d1, d2);
        dm = (desc == TLC_DESC_MIN && !single) ? (d2 > d1 ? d2 : d1) : fr;
    }
    if (am) { d.amb[atomicAdd(&a.head[DF_H_NAMB], 1)] = (int)i; atomicAdd((u64*)(a.head + DF_H_FALLBACKS), 1ull); }
    else { d.q[i] = fr; if (dm > 0.0) atomicMax(&d.gden[g], df_bits(dm)); }
}

// fallback work items base .. base + groups - 1 of the list: item k runs in slice k - base
__global__ __launch_bounds__(256) void df_dev_fb_init_kernel(DfArgs a, DfDev d, int base, int namb) {
    const int slot = (int)blockIdx.y, item = base + slot;
    if (item >= namb) return;
    const long long src = d.amb[item];
    const int g = a.ngraph[src];
    const long long n0 = a.node_ptr[g];
    const long long n = a.node_ptr[g + 1] - n0;
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k < n) d.slices[(long long)slot * d.slice_len + k] = (n0 + k == src) ? 0ull : DF_INF;
}

__global__ __launch_bounds__(256) void df_dev_fb_relax_kernel(DfArgs a, DfDev d, int base, int namb) {
    const int slot = (int)blockIdx.y, item = base + slot;
    if (item >= namb) return;
    const int g = a.ngraph[d.amb[item]];
    const long long e0 = a.edge_ptr[g];
    const long long m = a.edge_ptr[g + 1] - e0;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= m) return;
    u64* R = d.slices + (long long)slot * d.slice_len;
    const int p = a.edges[2 * (e0 + e)], q = a.edges[2 * (e0 + e) + 1];
    const double w = a.w[e0 + e];
    const u64 xa = R[p], xb = R[q];
    bool ch = false;
    if (xa != DF_INF) { const u64 s = df_bits(df_val(xa) + w); if (s < xb) ch |= atomicMin(&R[q], s) > s; }
    if (xb != DF_INF) { const u64 s = df_bits(df_val(xb) + w); if (s < xa) ch |= atomicMin(&R[p], s) > s; }
    if (ch) a.head[DF_H_GCHANGED + slot] = 1;
}

__global__ __launch_bounds__(256) void df_dev_fb_finish_kernel(DfArgs a, DfDev d, int base, int namb) {
    const int slot = (int)(blockIdx.x * 256 + threadIdx.x), item = base + slot;
    if (slot >= d.groups || item >= namb) return;
    const long long src = d.amb[item];
    const int g = a.ngraph[src];
    const unsigned desc = a.flags & TLC_DESC_MASK;
    const int lu = a.roots[2 * g];
    const bool single = a.roots[2 * g + 1] < 0 || desc == TLC_DESC_ROOT1;
    const int lv = single ? lu : a.roots[2 * g + 1];
    const u64* R = d.slices + (long long)slot * d.slice_len;
    const double e1 = R[lu] == DF_INF ? 100.0 : df_val(R[lu]);
    const double e2 = R[lv] == DF_INF ? 100.0 : df_val(R[lv]);
    const double fr = df_desc(desc, single, e1, e2);
    const double dm = (desc == TLC_DESC_MIN && !single) ? (e2 > e1 ? e2 : e1) : fr;
    d.q[src] = fr;
    if (dm > 0.0) atomicMax(&d.gden[g], df_bits(dm));
}

__global__ __launch_bounds__(256) void df_dev_norm_kernel(DfArgs a, DfDev d) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.N || a.ngraph[i] < 0) return;
    const int g = a.ngraph[i];
    int status = d.gstat[g];
    double den = df_val(d.gden[g]);
    if (status == TLC_ST_OK) {
        if (a.flags & TLC_NO_NORM) den = 1.0;
        else if (a.flags & TLC_NORM_EPS) den = den + 1e-10;
        else if (den == 0.0) status = TLC_ST_ZERO_RANGE;
    }
    if (status == TLC_ST_OK) a.f[i] = (a.flags & TLC_NO_NORM) ? d.q[i] : d.q[i] / den;
    else if (i == a.node_ptr[g]) a.status[g] = (unsigned char)status;
}

// ---- the VJP: a group of W threads per graph, state in d_work ----------------------------------------------------------------------------
struct DfVjp {
    const int* parent; const double* gf; double* gw;
    double* T0; double* T1; double* S0; double* S1;
    int* dep0; int* dep1; int* pe0; int* pe1; int* cc0; int* cc1; int* row0; int* row1; int* ch0; int* ch1;
};

template <int W>
__global__ __launch_bounds__(W) void df_vjp_kernel(DfArgs a, DfVjp v, int cls) {
    __shared__ int sh[W];
    __shared__ int ctl[4];
    __shared__ u64 red[2];
    __shared__ double corr_s;
    const int tid = (int)threadIdx.x;
    const int count = a.head[DF_H_COUNT + cls];
    const unsigned desc = a.flags & TLC_DESC_MASK;
    for (;;) {
        __syncthreads();
        if (tid == 0) ctl[2] = atomicAdd(&a.head[DF_H_TICKET + cls], 1);
        __syncthreads();
        const int i = ctl[2];
        if (i >= count) break;
        const int g = a.lists[(long long)cls * a.B + i];
        const long long n0 = a.node_ptr[g], e0 = a.edge_ptr[g];
        const int n = (int)(a.node_ptr[g + 1] - n0), m = (int)(a.edge_ptr[g + 1] - e0);
        const int* ed = a.edges + 2 * e0;
        const double* ew = a.w + e0;
        const int lu = a.roots[2 * g];
        const bool single = a.roots[2 * g + 1] < 0 || desc == TLC_DESC_ROOT1;
        const int lv = single ? lu : a.roots[2 * g + 1];
        const int nr = single ? 1 : 2;
        const int* P[2] = {v.parent + n0, v.parent + a.N + n0};
        double* T[2] = {v.T0 + n0, v.T1 + n0};
        double* S[2] = {v.S0 + n0, v.S1 + n0};
        int* dep[2] = {v.dep0 + n0, v.dep1 + n0};
        int* pe[2] = {v.pe0 + n0, v.pe1 + n0};
        int* cc[2] = {v.cc0 + n0, v.cc1 + n0};
        int* row[2] = {v.row0 + n0, v.row1 + n0};
        int* chl[2] = {v.ch0 + n0, v.ch1 + n0};
        const int root[2] = {lu, lv};
        for (int r = 0; r < nr; ++r)
            for (int k = tid; k < n; k += W) { pe[r][k] = -1; cc[r][k] = 0; }
        if (tid == 0) { ctl[0] = 0; ctl[1] = 0x7fffffff; red[0] = 0ull; }
        __syncthreads();
        // the tree edge of every node
        for (int e = tid; e < m; e += W) {
            const int p = ed[2 * e], q = ed[2 * e + 1];
            for (int r = 0; r < nr; ++r) {
                if (P[r][p] == q) pe[r][p] = e;
                else if (P[r][q] == p) pe[r][q] = e;
            }
        }
        __syncthreads();
        // T_r[x]: the weights along x's tree path, left to right; 100 where the path does not arrive.  depth: the steps until a node
        // without a tree edge
        int mydepth = 0;
        for (int x = tid; x < n; x += W) {
            double t[2] = {0.0, 0.0};
            for (int r = 0; r < nr; ++r) {
                int c = x, steps = 0;
                double s = 0.0;
                while (pe[r][c] >= 0 && steps < n) { s = s + ew[pe[r][c]]; c = P[r][c]; ++steps; }
                t[r] = c == root[r] ? s : 100.0;
                row[r][x] = c == root[r];                     // (until the scan below: does the path arrive)
                T[r][x] = t[r];
                dep[r][x] = steps;
                mydepth = steps > mydepth ? steps : mydepth;
                if (pe[r][x] >= 0) atomicAdd(&cc[r][P[r][x]], 1);
            }
            const bool isroot = x == lu || x == lv;
            const double q = isroot ? 0.0 : df_desc(desc, single, t[0], t[1]);
            const double dm = isroot ? 0.0 : ((desc == TLC_DESC_MIN && !single) ? (t[1] > t[0] ? t[1] : t[0]) : q);
            if (dm > 0.0) atomicMax(&red[0], df_bits(dm));
        }
        atomicMax(&ctl[0], mydepth);
        __syncthreads();
        const double den0 = df_val(red[0]);
        const int maxdepth = ctl[0];
        int status = TLC_ST_OK;
        double den = den0;
        const bool normed = !(a.flags & TLC_NO_NORM);
        if (!normed) den = 1.0;
        else if (a.flags & TLC_NORM_EPS) den = den0 + 1e-10;
        else if (den0 == 0.0) status = TLC_ST_ZERO_RANGE;
        if (status != TLC_ST_OK) {                        // (uniform over the group)
            if (tid == 0) a.status[g] = (unsigned char)status;
            continue;
        }
        // x*: the lowest index of the maximum
        for (int x = tid; x < n; x += W) {
            const bool isroot = x == lu || x == lv;
            const double t0 = T[0][x], t1 = single ? 0.0 : T[1][x];
            const double q = isroot ? 0.0 : df_desc(desc, single, t0, t1);
            const double dm = isroot ? 0.0 : ((desc == TLC_DESC_MIN && !single) ? (t1 > t0 ? t1 : t0) : q);
            if (dm == den0) atomicMin(&ctl[1], x);
        }
        // sum over x ascending, from +0.0, of g[x] q[x]
        if (tid == 0) {
            double s = 0.0;
            if (normed)
                for (int x = 0; x < n; ++x) {
                    const bool isroot = x == lu || x == lv;
                    const double q = isroot ? 0.0 : df_desc(desc, single, T[0][x], single ? 0.0 : T[1][x]);
                    s = s + v.gf[n0 + x] * q;
                }
            corr_s = s / (den * den);
        }
        __syncthreads();
        const int xstar = ctl[1];
        const double corr = corr_s;
        // c_r[x] into S_r[x]
        for (int x = tid; x < n; x += W) {
            const bool isroot = x == lu || x == lv;
            const double t0 = T[0][x], t1 = single ? 0.0 : T[1][x];
            const double av = v.gf[n0 + x] / den;
            for (int r = 0; r < nr; ++r) {
                const bool arrives = !isroot && row[r][x] != 0;
                bool sel, dsel;
                if (single || desc == 0u) { sel = true; dsel = true; }
                else if (desc == TLC_DESC_MIN) { sel = r == (t1 < t0 ? 1 : 0); dsel = r == (t1 > t0 ? 1 : 0); }
                else { sel = r == (t1 > t0 ? 1 : 0); dsel = sel; }
                double c = (arrives && sel) ? av : 0.0;
                if (normed && x == xstar && arrives && dsel) c = c - corr;
                S[r][x] = c;
            }
        }
        __syncthreads();
        // the children of every node in ascending id: row starts by a scan, then a stable fill chunk by chunk
        for (int r = 0; r < nr; ++r) {
            int base = 0;
            for (int x0 = 0; x0 < n; x0 += W) {
                const int x = x0 + tid;
                const int c = x < n ? cc[r][x] : 0;
                sh[tid] = c;
                __syncthreads();
                for (int off = 1; off < W; off <<= 1) {
                    const int t = tid >= off ? sh[tid - off] : 0;
                    __syncthreads();
                    sh[tid] += t;
                    __syncthreads();
                }
                if (x < n) { row[r][x] = base + sh[tid] - c; cc[r][x] = 0; }
                base += sh[W - 1];
                __syncthreads();
            }
            for (int x0 = 0; x0 < n; x0 += W) {
                const int x = x0 + tid;
                const int p = (x < n && pe[r][x] >= 0) ? P[r][x] : -1;
                sh[tid] = p;
                __syncthreads();
                int before = 0, after = 0;
                if (p >= 0) {
                    for (int t = 0; t < tid; ++t) before += sh[t] == p;
                    for (int t = tid + 1; t < W; ++t) after += sh[t] == p;
                    chl[r][row[r][p] + cc[r][p] + before] = x;
                }
                __syncthreads();
                if (p >= 0 && after == 0) cc[r][p] += before + 1;
                __syncthreads();
            }
        }
        // S_r[x] = c_r[x] + the children's S_r in ascending id, level by level from the deepest
        for (int lev = maxdepth; lev >= 0; --lev) {
            for (int r = 0; r < nr; ++r)
                for (int x = tid; x < n; x += W) {
                    if (dep[r][x] != lev) continue;
                    double s = S[r][x];
                    const int k0 = row[r][x], k1 = k0 + cc[r][x];
                    for (int k = k0; k < k1; ++k) s = s + S[r][chl[r][k]];
                    S[r][x] = s;
                }
            __syncthreads();
        }
        for (int e = tid; e < m; e += W) {
            const int p = ed[2 * e], q = ed[2 * e + 1];
            double gw = 0.0;
            for (int r = 0; r < nr; ++r) {
                if (pe[r][p] == e) gw = gw + S[r][p];
                else if (pe[r][q] == e) gw = gw + S[r][q];
            }
            v.gw[e0 + e] = gw;
        }
    }
}

int df_common_checks(int64_t n_graphs, int64_t total_nodes, int64_t total_edges) {
    TLC_REQUIRE(n_graphs >= 0 && n_graphs < (1ll << 31) && total_nodes >= 0 && total_edges >= 0, "bad sizes");
    if (total_nodes >= (1ll << 30) || total_edges >= (1ll << 30)) {
        tlc_set_error("tlc_dist_filtration: a batch of 2^30 nodes or edges and more is not supported");
        return TLC_ERR_UNSUPPORTED;
    }
    return TLC_OK;
}

}  // namespace

extern "C" int tlc_dist_filtration_work_bytes(int64_t n_graphs, int64_t total_nodes, int64_t total_edges, int64_t* bytes) {
    TLC_REQUIRE(bytes, "null pointer");
    const int rc = df_common_checks(n_graphs, total_nodes, total_edges);
    if (rc != TLC_OK) return rc;
    *bytes = TlcDistFiltScratch(n_graphs, total_nodes, total_edges, DF_WG_N, DF_WG_M, false).least;
    return TLC_OK;
}

extern "C" int tlc_dist_filtration_vjp_work_bytes(int64_t n_graphs, int64_t total_nodes, int64_t total_edges, int64_t* bytes) {
    TLC_REQUIRE(bytes, "null pointer");
    const int rc = df_common_checks(n_graphs, total_nodes, total_edges);
    if (rc != TLC_OK) return rc;
    *bytes = TlcDistFiltScratch(n_graphs, total_nodes, total_edges, DF_WG_N, DF_WG_M, true).least;
    return TLC_OK;
}

namespace {
// the shared front of both entries: the control words, the hash, validation and binning
int df_front(DfArgs& a, const TlcDistFiltScratch& L, unsigned char* w, bool vjp, hipStream_t s) {
    a.head = (int*)w;
    a.lists = (int*)(w + L.lists);
    a.hash = (u64*)(w + L.hash);
    a.egraph = (int*)(w + L.egraph);
    TLC_HIP_CHECK(hipMemsetAsync(w, 0, (size_t)L.egraph, s));                        // head, lists, hash
    if (a.M) TLC_HIP_CHECK(hipMemsetAsync(a.egraph, 0xff, (size_t)a.M * 4, s));
    if (a.ngraph) TLC_HIP_CHECK(hipMemsetAsync(a.ngraph, 0xff, (size_t)a.N * 4, s));
    hipLaunchKernelGGL(df_check_kernel, dim3(tlc_grid_for(a.B, 4, 2048)), dim3(256), 0, s, a, vjp ? 1 : 0);
    TLC_HIP_CHECK(hipGetLastError());
    return TLC_OK;
}
}  // namespace

extern "C" int tlc_dist_filtration(int64_t n_graphs, const int64_t* d_node_ptr, const int64_t* d_edge_ptr, const int32_t* d_edges,
                                   const double* d_w, const int32_t* d_roots, int64_t total_nodes, int64_t total_edges, uint32_t flags,
                                   double* d_f, uint8_t* d_status, int32_t* d_parent, void* d_work, int64_t work_bytes, void* stream) {
    int rc = df_common_checks(n_graphs, total_nodes, total_edges);
    if (rc != TLC_OK) return rc;
    TLC_REQUIRE((flags & ~DF_FLAGS) == 0, "unknown flag");
    if (n_graphs == 0) return TLC_OK;
    TLC_REQUIRE(d_node_ptr && d_edge_ptr && d_roots && d_status && d_work && (total_nodes == 0 || d_f) && (total_edges == 0 || (d_edges && d_w)),
                "null pointer");
    const TlcDistFiltScratch L(n_graphs, total_nodes, total_edges, DF_WG_N, DF_WG_M, false);
    TLC_REQUIRE(work_bytes >= L.least, "d_work is smaller than tlc_dist_filtration_work_bytes()");
    TLC_REQUIRE((reinterpret_cast<uintptr_t>(d_work) & 255) == 0, "d_work must be 256-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    unsigned char* w = (unsigned char*)d_work;
    DfArgs a{};
    a.B = n_graphs; a.N = total_nodes; a.M = total_edges;
    a.node_ptr = (const long long*)d_node_ptr; a.edge_ptr = (const long long*)d_edge_ptr;
    a.edges = d_edges; a.w = d_w; a.roots = d_roots; a.flags = flags; a.f = d_f; a.status = d_status; a.parent = d_parent;
    DfDev d{};
    if (L.wide) {
        int64_t o = L.node;
        auto take = [&](int64_t count, int64_t size) { const int64_t at = o; o += TlcDistFiltScratch::up256(count * size); return (void*)(w + at); };
        d.R0 = (u64*)take(a.N, 8); d.R1 = (u64*)take(a.N, 8); d.q = (double*)take(a.N, 8);
        d.cnt0 = (unsigned*)take(a.N, 4); d.cnt1 = (unsigned*)take(a.N, 4); d.nxt0 = (unsigned*)take(a.N, 4); d.nxt1 = (unsigned*)take(a.N, 4);
        d.amb = (int*)take(a.N, 4); a.ngraph = (int*)take(a.N, 4);
        o = L.graph;
        d.gmax = (u64*)take(a.B, 8); d.gden = (u64*)take(a.B, 8); d.gstat = (int*)take(a.B, 4);
        d.slices = (u64*)(w + L.slices); d.slice_len = L.slice_bytes / 8; d.groups = (int)L.groups_in(work_bytes);
    }
    rc = df_front(a, L, w, false, s);
    if (rc != TLC_OK) return rc;
    constexpr size_t lds_w = df_group_lds(DF_WAVE_N), lds_g = df_group_lds(DF_WG_N);
    static_assert(2 * lds_g <= 160 * 1024, "two workgroups of the workgroup class per CU");
    TLC_HIP_CHECK(hipFuncSetAttribute((const void*)df_group_kernel<256, DF_WG_N>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_g));
    hipLaunchKernelGGL((df_group_kernel<64, DF_WAVE_N>), dim3(tlc_grid_for(a.B, 1, 8192)), dim3(64), lds_w, s, a, 0);
    TLC_HIP_CHECK(hipGetLastError());
    if (a.N > DF_WAVE_N) {
        hipLaunchKernelGGL((df_group_kernel<256, DF_WG_N>), dim3(tlc_grid_for(std::min<long long>(a.B, a.N / (DF_WAVE_N + 1)), 1, 512)), dim3(256), lds_g, s, a, 1);
        TLC_HIP_CHECK(hipGetLastError());
    }
    if (!L.wide) return TLC_OK;
    // the whole-device class: its size and its largest graph, read back once
    int head[16];
    TLC_HIP_CHECK(hipMemcpyAsync(head, a.head, sizeof(head), hipMemcpyDeviceToHost, s));
    TLC_HIP_CHECK(hipStreamSynchronize(s));
    if (head[DF_H_COUNT + 2] == 0) return TLC_OK;
    const int maxn = head[DF_H_MAXN], maxm = head[DF_H_MAXM];
    const unsigned gn = (unsigned)((a.N + 255) / 256), gm = (unsigned)((a.M + 255) / 256), gm2 = (unsigned)((2 * a.M + 255) / 256);
    hipLaunchKernelGGL(df_dev_init_kernel, dim3(gn), dim3(256), 0, s, a, d);
    TLC_HIP_CHECK(hipGetLastError());
    for (int round = 0; round < maxn; ++round) {
        hipLaunchKernelGGL(df_dev_relax_kernel, dim3(gm), dim3(256), 0, s, a, d);
        TLC_HIP_CHECK(hipGetLastError());
        if ((round + 1) % DF_CHECK_EVERY == 0) {
            int changed = 0;
            TLC_HIP_CHECK(hipMemcpyAsync(&changed, a.head + DF_H_CHANGED, 4, hipMemcpyDeviceToHost, s));
            TLC_HIP_CHECK(hipMemsetAsync(a.head + DF_H_CHANGED, 0, 4, s));
            TLC_HIP_CHECK(hipStreamSynchronize(s));
            if (!changed) break;
        }
    }
    hipLaunchKernelGGL(df_dev_parent_kernel, dim3(gm), dim3(256), 0, s, a, d);
    hipLaunchKernelGGL(df_dev_dmax_kernel, dim3(gn), dim3(256), 0, s, a, d);
    hipLaunchKernelGGL(df_dev_tight_kernel, dim3(gm2), dim3(256), 0, s, a, d);
    hipLaunchKernelGGL(df_dev_walk_kernel, dim3(gn), dim3(256), 0, s, a, d);
    TLC_HIP_CHECK(hipGetLastError());
    int namb = 0;
    TLC_HIP_CHECK(hipMemcpyAsync(&namb, a.head + DF_H_NAMB, 4, hipMemcpyDeviceToHost, s));
    TLC_HIP_CHECK(hipStreamSynchronize(s));
    const int G = d.groups;
    int gch[TlcDistFiltScratch::MAX_GROUPS];
    for (int base = 0; base < namb; base += G) {
        TLC_HIP_CHECK(hipMemsetAsync(a.head + DF_H_GCHANGED, 0, (size_t)G * 4, s));
        hipLaunchKernelGGL(df_dev_fb_init_kernel, dim3((unsigned)((maxn + 255) / 256), (unsigned)G), dim3(256), 0, s, a, d, base, namb);
        TLC_HIP_CHECK(hipGetLastError());
        for (int round = 0; round < maxn; ++round) {
            hipLaunchKernelGGL(df_dev_fb_relax_kernel, dim3((unsigned)((maxm + 255) / 256), (unsigned)G), dim3(256), 0, s, a, d, base, namb);
            TLC_HIP_CHECK(hipGetLastError());
            if ((round + 1) % DF_CHECK_EVERY == 0) {
                TLC_HIP_CHECK(hipMemcpyAsync(gch, a.head + DF_H_GCHANGED, (size_t)G * 4, hipMemcpyDeviceToHost, s));
                TLC_HIP_CHECK(hipMemsetAsync(a.head + DF_H_GCHANGED, 0, (size_t)G * 4, s));
                TLC_HIP_CHECK(hipStreamSynchronize(s));
                int any = 0;
                for (int k = 0; k < G; ++k) any |= gch[k];
                if (!any) break;
            }
        }
        hipLaunchKernelGGL(df_dev_fb_finish_kernel, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, s, a, d, base, namb);
        TLC_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(df_dev_norm_kernel, dim3(gn), dim3(256), 0, s, a, d);
    TLC_HIP_CHECK(hipGetLastError());
    return TLC_OK;
}

extern "C" int tlc_dist_filtration_vjp(int64_t n_graphs, const int64_t* d_node_ptr, const int64_t* d_edge_ptr, const int32_t* d_edges,
                                       const double* d_w, const int32_t* d_roots, int64_t total_nodes, int64_t total_edges, uint32_t flags,
                                       const double* d_f, const int32_t* d_parent, const double* d_grad_f, double* d_grad_w,
                                       uint8_t* d_status, void* d_work, int64_t work_bytes, void* stream) {
    (void)d_f;
    int rc = df_common_checks(n_graphs, total_nodes, total_edges);
    if (rc != TLC_OK) return rc;
    TLC_REQUIRE((flags & ~DF_FLAGS) == 0, "unknown flag");
    if (n_graphs == 0) return TLC_OK;
    TLC_REQUIRE(d_node_ptr && d_edge_ptr && d_roots && d_status && d_work && (total_nodes == 0 || (d_parent && d_grad_f)) &&
                    (total_edges == 0 || (d_edges && d_w && d_grad_w)), "null pointer");
    const TlcDistFiltScratch L(n_graphs, total_nodes, total_edges, DF_WG_N, DF_WG_M, true);
    TLC_REQUIRE(work_bytes >= L.least, "d_work is smaller than tlc_dist_filtration_vjp_work_bytes()");
    TLC_REQUIRE((reinterpret_cast<uintptr_t>(d_work) & 255) == 0, "d_work must be 256-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    unsigned char* w = (unsigned char*)d_work;
    DfArgs a{};
    a.B = n_graphs; a.N = total_nodes; a.M = total_edges;
    a.node_ptr = (const long long*)d_node_ptr; a.edge_ptr = (const long long*)d_edge_ptr;
    a.edges = d_edges; a.w = d_w; a.roots = d_roots; a.flags = flags; a.status = d_status;
    DfVjp v{};
    v.parent = d_parent; v.gf = d_grad_f; v.gw = d_grad_w;
    int64_t o = L.node;
    auto take = [&](int64_t count, int64_t size) { const int64_t at = o; o += TlcDistFiltScratch::up256(count * size); return (void*)(w + at); };
    v.T0 = (double*)take(a.N, 8); v.T1 = (double*)take(a.N, 8); v.S0 = (double*)take(a.N, 8); v.S1 = (double*)take(a.N, 8);
    v.dep0 = (int*)take(a.N, 4); v.dep1 = (int*)take(a.N, 4); v.pe0 = (int*)take(a.N, 4); v.pe1 = (int*)take(a.N, 4);
    v.cc0 = (int*)take(a.N, 4); v.cc1 = (int*)take(a.N, 4); v.row0 = (int*)take(a.N, 4); v.row1 = (int*)take(a.N, 4);
    v.ch0 = (int*)take(a.N, 4); v.ch1 = (int*)take(a.N, 4);
    rc = df_front(a, L, w, true, s);
    if (rc != TLC_OK) return rc;
    hipLaunchKernelGGL((df_vjp_kernel<64>), dim3(tlc_grid_for(a.B, 1, 8192)), dim3(64), 0, s, a, v, 0);
    TLC_HIP_CHECK(hipGetLastError());
    if (a.N > DF_WAVE_N) {
        hipLaunchKernelGGL((df_vjp_kernel<256>), dim3(tlc_grid_for(std::min<long long>(a.B, a.N / (DF_WAVE_N + 1)), 1, 2048)), dim3(256), 0, s, a, v, 1);
        TLC_HIP_CHECK(hipGetLastError());
    }
    return TLC_OK;
}

// hks_sparse.hip -- tlc_hks_sparse_batch / _dt: heat-kernel signatures of sparse graphs of any size, without eigenpairs and without a
// dense matrix.  With M = D^-1/2 A D^-1/2, L = I - M, tau = t / 2, column v of exp(-tau L) is y_v = exp(-tau) sum_k z_k, z_0 = e_v,
// z_k = (tau / k) M z_{k-1}, and hks_t(v) = |y_v|^2, d/dt hks_t(v) = y_v^T M y_v - |y_v|^2  (include/tlcgnn.h states the operation
// sequence).  Kernels:
//   once per call   setup (descriptors from launch arguments), head (offsets and declared counts), emit (two sort keys per edge), the
//                   shared radix passes, rowptr (a binary search per row), cols (columns; adjacent equal keys = a repeat), rows (r_u and
//                   the chunk slots of the split rows), status;
//   per group, time init, then per Taylor step part (a wavefront per chunk of a split row; only where the declared sizes of a graph of
//                   the group allow a row above TLC_HKS_SPARSE_LONG_ROW neighbours) and step (a wavefront per four rows of a
//                   panel, lane = column: a neighbour costs one coalesced 512-byte row load), then scale, for the derivative part and
//                   step again on q, red1 (a wavefront per block of 64 rows), red2 (a wavefront per panel: the values);
//   per time        norm / norm_dt (a workgroup per graph), after the last group.
// A group is a run of consecutive panels (graph after graph, panel after panel) whose vectors fit d_work; a column's bits depend on its
// graph and the time alone, so the groups' cuts change nothing.
#include "radix_passes.h"
#include "scratch_layouts.h"

#include <math.h>

#define HKSS_P TLC_HKS_SPARSE_PANEL
#define HKSS_LONG TLC_HKS_SPARSE_LONG_ROW
#define HKSS_ROWS_PER_WG 16       // step / init / scale: four rows per wavefront
static_assert(HKSS_P == 64 && TlcHksSparseScratch::PANEL == HKSS_P && TlcHksSparseScratch::LONG_ROW == HKSS_LONG, "one panel width");

namespace {

struct HkssDesc {               // one selected graph (64 bytes)
    long long panel_base;       // index of its first panel among the selection's
    long long buf_cum;          // doubles of all panels before its first
    int g, n, m;                // index in the batch; nodes and edges as the caller declared them
    int row_base, ent_base;     // its first row; its first entry as declared (2 x the edges before it)
    int slot_base, nslots;      // its chunk slots in slotrow
    int pad[5];
};
static_assert(sizeof(HkssDesc) == TlcHksSparseScratch::DESC, "HkssDesc is 64 bytes");

enum { HKSS_EMPTY = 0, HKSS_RUN = 1, HKSS_BAD = 2 };

struct HkssCtx {
    const HkssDesc* descs;
    int* state;
    const int* rowptr;
    const int* col;
    const double* rinv;
    const int* slotrow;
    double* bufs;               // the group's panels
    long long first_panel, buf0;   // the group's first panel and the doubles of all panels before it
    int n_sel, n_panels;
};

struct HkssPanel {              // a panel of the group, located
    int gi, pl, n, nslots, nb;  // graph of the selection, panel of the graph, its nodes, chunk slots, row blocks
    int row_base;
    double *S, *A, *B, *part, *red;
};

__host__ __device__ inline int hkss_slot0(int p_local) { return p_local / HKSS_P + p_local / HKSS_LONG; }

// the last graph whose `key` (panel_base, row_base or ent_base: ascending, equal for graphs that own nothing) is <= v
template <typename F>
__device__ __forceinline__ int hkss_find(const HkssDesc* descs, int n_sel, long long v, F key) {
    int lo = 0, hi = n_sel - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (key(descs[mid]) <= v) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ bool hkss_locate(const HkssCtx& C, int y, HkssPanel& P) {
    const long long p = C.first_panel + y;
    const int gi = hkss_find(C.descs, C.n_sel, p, [](const HkssDesc& d) { return d.panel_base; });
    if (C.state[gi] != HKSS_RUN) return false;
    const HkssDesc d = C.descs[gi];
    P.gi = gi; P.pl = (int)(p - d.panel_base); P.n = d.n; P.nslots = d.nslots; P.nb = (d.n + HKSS_P - 1) / HKSS_P; P.row_base = d.row_base;
    const long long pd = (long long)HKSS_P * (3ll * d.n + d.nslots + 2ll * P.nb);
    double* b = C.bufs + (d.buf_cum + (long long)P.pl * pd - C.buf0);
    P.S = b; P.A = b + (size_t)HKSS_P * d.n; P.B = P.A + (size_t)HKSS_P * d.n; P.part = P.B + (size_t)HKSS_P * d.n;
    P.red = P.part + (size_t)HKSS_P * d.nslots;
    return true;
}

// ---- setup: descriptors from launch arguments (nothing is copied from host memory) ------------------------------------------------------
#define HKSS_CHUNK 128
struct HkssChunk {
    long long panel_base, buf_cum;
    int count, first, row_base, ent_base, slot_base;
    int g[HKSS_CHUNK], n[HKSS_CHUNK], m[HKSS_CHUNK];
};

__global__ __launch_bounds__(HKSS_CHUNK) void hkss_setup_kernel(HkssChunk C, HkssDesc* __restrict__ descs) {
    const int k = threadIdx.x;
    if (k >= C.count) return;
    HkssDesc d;
    d.panel_base = C.panel_base; d.buf_cum = C.buf_cum; d.row_base = C.row_base; d.ent_base = C.ent_base; d.slot_base = C.slot_base;
    for (int j = 0; j < k; ++j) {
        const long long n = C.n[j], e = 2ll * C.m[j];
        const long long nb = TlcHksSparseScratch::blocks_of(n);
        d.panel_base += nb;
        d.buf_cum += nb * TlcHksSparseScratch::panel_doubles(n, e);
        d.row_base += (int)n; d.ent_base += (int)e; d.slot_base += (int)TlcHksSparseScratch::slots_of(e);
    }
    d.g = C.g[k]; d.n = C.n[k]; d.m = C.m[k];
    d.nslots = (int)TlcHksSparseScratch::slots_of(2ll * C.m[k]);
    for (int i = 0; i < 5; ++i) d.pad[i] = 0;
    descs[C.first + k] = d;
}

// ---- head: a thread per selected graph -- its offsets and the declared counts, before anything is indexed with them -------------------
__global__ __launch_bounds__(256) void hkss_head_kernel(const HkssDesc* __restrict__ descs, int n_sel, long long total_nodes, long long total_edges,
                                                        const long long* __restrict__ node_ptr, const long long* __restrict__ edge_ptr,
                                                        int* __restrict__ state) {
    const int gi = blockIdx.x * 256 + threadIdx.x;
    if (gi >= n_sel) return;
    const HkssDesc d = descs[gi];
    const long long n0 = node_ptr[d.g], n1 = node_ptr[d.g + 1], e0 = edge_ptr[d.g], e1 = edge_ptr[d.g + 1];
    bool ok = !(n0 < 0 || n1 < n0 || n1 > total_nodes || e0 < 0 || e1 < e0 || e1 > total_edges);
    ok = ok && n1 - n0 == (long long)d.n && e1 - e0 == (long long)d.m;
    // a simple graph has at most n (n - 1) / 2 edges: more of them hold a repeat
    ok = ok && (long long)d.m <= (long long)d.n * (d.n - 1) / 2;
    state[gi] = !ok ? HKSS_BAD : d.n == 0 ? HKSS_EMPTY : HKSS_RUN;
}

// ---- emit: a thread per declared edge -- the keys (row << 32 | column) of its two entries; ~0 for what is not computed ----------------
__global__ __launch_bounds__(256) void hkss_emit_kernel(const HkssDesc* __restrict__ descs, int n_sel, long long sel_edges,
                                                        const long long* __restrict__ edge_ptr, const int* __restrict__ edges,
                                                        int* __restrict__ state, unsigned long long* __restrict__ keys) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= sel_edges) return;
    const int gi = hkss_find(descs, n_sel, 2 * i, [](const HkssDesc& d) { return (long long)d.ent_base; });
    const HkssDesc d = descs[gi];
    unsigned long long ka = ~0ull, kb = ~0ull;
    // (another thread may set HKSS_BAD meanwhile: this edge then gets a key or not, and the graph is not computed either way)
    if (state[gi] == HKSS_RUN) {                               // its offsets are in range and hold d.m edges
        const long long e = edge_ptr[d.g] + (i - d.ent_base / 2);
        const int a = edges[2 * e], b = edges[2 * e + 1];
        if ((unsigned)a >= (unsigned)d.n || (unsigned)b >= (unsigned)d.n || a == b) state[gi] = HKSS_BAD;
        else {
            ka = ((unsigned long long)(unsigned)(d.row_base + a) << 32) | (unsigned)b;
            kb = ((unsigned long long)(unsigned)(d.row_base + b) << 32) | (unsigned)a;
        }
    }
    keys[2 * i] = ka;
    keys[2 * i + 1] = kb;
}

// ---- rowptr: a thread per row (and one for the end) -- the first sorted key >= row << 32 ---------------------------------------------------
__global__ __launch_bounds__(256) void hkss_rowptr_kernel(const unsigned long long* __restrict__ keys, int n_ent, int rows, int* __restrict__ rowptr) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r > rows) return;
    const unsigned long long want = (unsigned long long)(unsigned)r << 32;
    int lo = 0, hi = n_ent;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < want) lo = mid + 1; else hi = mid;
    }
    rowptr[r] = lo;
}

// ---- cols: a thread per sorted entry -- its column; two adjacent equal keys are a repeated edge, in either orientation ----------------
__global__ __launch_bounds__(256) void hkss_cols_kernel(const HkssDesc* __restrict__ descs, int n_sel, const unsigned long long* __restrict__ keys, int n_ent,
                                                        int* __restrict__ col, int* __restrict__ state) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_ent) return;
    const unsigned long long k = keys[i];
    col[i] = (int)(unsigned)k;
    if (k != ~0ull && i + 1 < n_ent && keys[i + 1] == k)
        state[hkss_find(descs, n_sel, (long long)(k >> 32), [](const HkssDesc& d) { return (long long)d.row_base; })] = HKSS_BAD;
}

// ---- rows: a thread per row -- r_u, and for a split row the slots of its chunks -------------------------------------------------------
__global__ __launch_bounds__(256) void hkss_rows_kernel(const HkssDesc* __restrict__ descs, int n_sel, int rows, const int* __restrict__ rowptr,
                                                        const int* __restrict__ state, double* __restrict__ rinv, int* __restrict__ slotrow) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const int p0 = rowptr[r], deg = rowptr[r + 1] - p0;
    rinv[r] = deg > 0 ? 1.0 / sqrt((double)deg) : 0.0;
    if (deg <= HKSS_LONG) return;
    const int gi = hkss_find(descs, n_sel, (long long)r, [](const HkssDesc& d) { return (long long)d.row_base; });
    if (state[gi] != HKSS_RUN) return;                         // (a graph that runs owns exactly its 2 m declared entries)
    const HkssDesc d = descs[gi];
    const int s0 = hkss_slot0(p0 - rowptr[d.row_base]), nch = (deg + HKSS_P - 1) / HKSS_P;
    for (int j = 0; j < nch && s0 + j < d.nslots; ++j) slotrow[d.slot_base + s0 + j] = r - d.row_base;
}

__global__ __launch_bounds__(256) void hkss_status_kernel(const HkssDesc* __restrict__ descs, int n_sel, const int* __restrict__ state,
                                                          unsigned char* __restrict__ status) {
    const int gi = blockIdx.x * 256 + threadIdx.x;
    if (gi < n_sel) status[descs[gi].g] = (unsigned char)(state[gi] == HKSS_BAD ? TLC_ST_BAD_INPUT : TLC_ST_OK);
}

// ---- the ordered sums -------------------------------------------------------------------------------------------------------------------
// entries [c0, c1) (at most a chunk) of x, ascending from +0.0; eight loads travel at once, the additions keep their order
__device__ __forceinline__ double hkss_chunk_sum(const double* __restrict__ x, const int* __restrict__ col, int c0, int c1, int lane) {
    double part = 0.0;
    int i = c0;
    for (; i + 8 <= c1; i += 8) {
        double v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = x[(size_t)col[i + j] * HKSS_P + lane];
#pragma unroll
        for (int j = 0; j < 8; ++j) part += v[j];
    }
    for (; i < c1; ++i) part += x[(size_t)col[i] * HKSS_P + lane];
    return part;
}

// R_u(x) for the rows up to HKSS_LONG neighbours; above, the chunks' partial sums from hkss_part_kernel
__device__ __forceinline__ double hkss_row_sum(const HkssCtx& C, const HkssPanel& P, const double* __restrict__ x, int u, int gstart, int lane) {
    const int p0 = C.rowptr[P.row_base + u], p1 = C.rowptr[P.row_base + u + 1];
    double tot = 0.0;
    if (p1 - p0 <= HKSS_LONG) {
        for (int c0 = p0; c0 < p1; c0 += HKSS_P) tot += hkss_chunk_sum(x, C.col, c0, c0 + HKSS_P < p1 ? c0 + HKSS_P : p1, lane);
    } else {
        const int s0 = hkss_slot0(p0 - gstart), nch = (p1 - p0 + HKSS_P - 1) / HKSS_P;
        for (int j = 0; j < nch; ++j) tot += P.part[(size_t)(s0 + j) * HKSS_P + lane];
    }
    return tot;
}

__device__ __forceinline__ double* hkss_vec(const HkssPanel& P, int sel) { return sel == 1 ? P.A : P.B; }

// ---- init: S = e_v, s = r_v e_v ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hkss_init_kernel(HkssCtx C, int dst) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (int y = blockIdx.y; y < C.n_panels; y += gridDim.y) {
        HkssPanel P;
        if (!hkss_locate(C, y, P)) continue;
        double* s = hkss_vec(P, dst);
        for (int rr = 0; rr < 4; ++rr) {
            const int u = blockIdx.x * HKSS_ROWS_PER_WG + wave * 4 + rr;
            if (u >= P.n) break;
            const bool diag = u == P.pl * HKSS_P + lane;
            P.S[(size_t)u * HKSS_P + lane] = diag ? 1.0 : 0.0;
            s[(size_t)u * HKSS_P + lane] = diag ? C.rinv[P.row_base + u] : 0.0;
        }
    }
}

// ---- part: a wavefront per chunk slot of a panel -- the partial sum of one chunk of a split row ------------------------------------------
__global__ __launch_bounds__(256) void hkss_part_kernel(HkssCtx C, int src) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (int y = blockIdx.y; y < C.n_panels; y += gridDim.y) {
        HkssPanel P;
        if (!hkss_locate(C, y, P)) continue;
        const int sl = blockIdx.x * 4 + wave;
        if (sl >= P.nslots) continue;
        const int u = C.slotrow[C.descs[P.gi].slot_base + sl];
        if (u < 0 || u >= P.n) continue;
        const int gstart = C.rowptr[P.row_base], p0 = C.rowptr[P.row_base + u], p1 = C.rowptr[P.row_base + u + 1];
        const int j = sl - hkss_slot0(p0 - gstart), c0 = p0 + j * HKSS_P;
        if (j < 0 || c0 >= p1) continue;
        P.part[(size_t)sl * HKSS_P + lane] = hkss_chunk_sum(hkss_vec(P, src), C.col, c0, c0 + HKSS_P < p1 ? c0 + HKSS_P : p1, lane);
    }
}

// ---- step: a wavefront per four rows of a panel.  QUAD false: z = (ck r_u) R_u(s), S += z, s' = r_u z.  QUAD true: g = q[u] R_u(q) ----------
template <bool QUAD>
__global__ __launch_bounds__(256) void hkss_step_kernel(HkssCtx C, int src, int dst, double ck) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (int y = blockIdx.y; y < C.n_panels; y += gridDim.y) {
        HkssPanel P;
        if (!hkss_locate(C, y, P)) continue;
        const double* x = hkss_vec(P, src);
        double* o = hkss_vec(P, dst);
        const int gstart = C.rowptr[P.row_base];
        for (int rr = 0; rr < 4; ++rr) {
            const int u = blockIdx.x * HKSS_ROWS_PER_WG + wave * 4 + rr;
            if (u >= P.n) break;
            const double tot = hkss_row_sum(C, P, x, u, gstart, lane);
            const size_t at = (size_t)u * HKSS_P + lane;
            if (QUAD) o[at] = x[at] * tot;
            else {
                const double r = C.rinv[P.row_base + u];
                const double z = (ck * r) * tot;
                P.S[at] = P.S[at] + z;
                o[at] = r * z;
            }
        }
    }
}

// ---- scale: y = exp(-tau) S (into S), q = r y ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hkss_scale_kernel(HkssCtx C, int dst, double factor) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (int y = blockIdx.y; y < C.n_panels; y += gridDim.y) {
        HkssPanel P;
        if (!hkss_locate(C, y, P)) continue;
        double* q = hkss_vec(P, dst);
        for (int rr = 0; rr < 4; ++rr) {
            const int u = blockIdx.x * HKSS_ROWS_PER_WG + wave * 4 + rr;
            if (u >= P.n) break;
            const size_t at = (size_t)u * HKSS_P + lane;
            const double v = factor * P.S[at];
            P.S[at] = v;
            q[at] = C.rinv[P.row_base + u] * v;
        }
    }
}

// ---- red1: a wavefront per block of 64 rows -- the block's partial sums of y^2 and (DT) of g ----------------------------------------------
template <bool DT>
__global__ __launch_bounds__(256) void hkss_red1_kernel(HkssCtx C, int g_sel) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (int y = blockIdx.y; y < C.n_panels; y += gridDim.y) {
        HkssPanel P;
        if (!hkss_locate(C, y, P)) continue;
        const int b = blockIdx.x * 4 + wave;
        if (b >= P.nb) continue;
        const double* g = hkss_vec(P, g_sel);
        const int u1 = (b + 1) * HKSS_P < P.n ? (b + 1) * HKSS_P : P.n;
        double pv = 0.0, pq = 0.0;
        for (int u = b * HKSS_P; u < u1; ++u) {
            const double v = P.S[(size_t)u * HKSS_P + lane];
            pv += v * v;
            if (DT) pq += g[(size_t)u * HKSS_P + lane];
        }
        P.red[(size_t)(2 * b) * HKSS_P + lane] = pv;
        if (DT) P.red[(size_t)(2 * b + 1) * HKSS_P + lane] = pq;
    }
}

// ---- red2: a wavefront per panel -- the blocks' partial sums ascending; the value and the derivative of column v ----------------------------
template <bool DT>
__global__ __launch_bounds__(256) void hkss_red2_kernel(HkssCtx C, const long long* __restrict__ node_ptr, double* __restrict__ out, double* __restrict__ dout) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long y = (long long)blockIdx.x * 4 + wave;
    if (y >= C.n_panels) return;
    HkssPanel P;
    if (!hkss_locate(C, (int)y, P)) return;
    double val = 0.0, quad = 0.0;
    for (int b = 0; b < P.nb; ++b) {
        val += P.red[(size_t)(2 * b) * HKSS_P + lane];
        if (DT) quad += P.red[(size_t)(2 * b + 1) * HKSS_P + lane];
    }
    const int v = P.pl * HKSS_P + lane;
    if (v >= P.n) return;
    const bool isolated = C.rowptr[P.row_base + v + 1] == C.rowptr[P.row_base + v];
    const long long at = node_ptr[C.descs[P.gi].g] + v;
    out[at] = isolated ? 1.0 : val;
    if (DT) dout[at] = isolated ? 0.0 : quad - val;
}

// ---- norm: a workgroup per selected graph.  f = hks / (mx + 1e-10), mx = hks(a) at the LOWEST index a of the maximum;
// DT: f'(x) = (hks'(x) - f(x) hks'(a)) / (mx + 1e-10) -----------------------------------------------------------------------------------
template <bool DT>
__global__ __launch_bounds__(256) void hkss_norm_kernel(const HkssDesc* __restrict__ descs, const int* __restrict__ state, const long long* __restrict__ node_ptr,
                                                        double* __restrict__ out, double* __restrict__ dout) {
    __shared__ double smax[256];
    __shared__ int sarg[256];
    const int gi = blockIdx.x, tid = threadIdx.x;
    if (state[gi] != HKSS_RUN) return;
    const HkssDesc d = descs[gi];
    double* o = out + node_ptr[d.g];
    double* dd = DT ? dout + node_ptr[d.g] : nullptr;
    double mx = o[0];
    int a = 0;
    for (int x = tid; x < d.n; x += 256)                       // x ascending: the first of equal values stays
        if (o[x] > mx) { mx = o[x]; a = x; }
    smax[tid] = mx;
    sarg[tid] = a;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) {
            const double m2 = smax[tid + h];
            const int a2 = sarg[tid + h];
            if (m2 > smax[tid] || (m2 == smax[tid] && a2 < sarg[tid])) { smax[tid] = m2; sarg[tid] = a2; }
        }
        __syncthreads();
    }
    mx = smax[0];
    const double da = DT ? dd[sarg[0]] : 0.0;
    __syncthreads();                                           // every thread holds hks'(a) before its owner overwrites it
    for (int x = tid; x < d.n; x += 256) {
        const double f = o[x] / (mx + 1e-10);
        o[x] = f;
        if (DT) dd[x] = (dd[x] - f * da) / (mx + 1e-10);
    }
}

inline unsigned hkss_grid_y(long long n) { return (unsigned)(n < 65535 ? n : 65535); }

}  // namespace

extern "C" int32_t tlc_hks_sparse_terms(double t) {
    if (!(t >= 0.0 && t <= TLC_HKS_SPARSE_TIME_MAX)) return -1;
    const double tau = t * 0.5;
    if (tau == 0.0) return 0;
    double E = 1.0, term = 1.0;
    for (int j = 1; j <= 400; ++j) {
        term = term * tau / (double)j;
        E = E + term;
    }
    const double bound = 1.0 / 18446744073709551616.0, slack = 1.0 + 1.0 / 1099511627776.0;   // 2^-64; 1 + 2^-40
    term = 1.0;
    for (int k = 0; k < 1000; ++k) {
        term = term * tau / (double)(k + 1);
        if ((double)(k + 2) > tau && term / (1.0 - tau / (double)(k + 2)) / E * slack <= bound) return k;
    }
    return -1;
}

namespace {

#define HKSS_REQUIRE(cond, msg)                                                                                                                \
    do {                                                                                                                                       \
        if (!(cond)) { tlc_set_error("%s: %s", fn, msg); return TLC_ERR_INVALID_ARG; }                                                         \
    } while (0)

// the checks on a selection's declared sizes that the layout and the 32-bit ids need
int hkss_check_sizes(const char* fn, const int64_t* h_sel_nodes, const int64_t* h_sel_edges, int64_t n_sel) {
    HKSS_REQUIRE(n_sel >= 0 && n_sel < (1ll << 31), "bad sizes");
    HKSS_REQUIRE(n_sel == 0 || (h_sel_nodes && h_sel_edges), "null pointer");
    int64_t rows = 0, edges = 0;
    for (int64_t i = 0; i < n_sel; ++i) {
        HKSS_REQUIRE(h_sel_nodes[i] >= 0, "negative node count");
        HKSS_REQUIRE(h_sel_edges[i] >= 0, "negative edge count");
        HKSS_REQUIRE(h_sel_nodes[i] < (1ll << 31) - 1 && h_sel_edges[i] < (1ll << 30), "the selection exceeds 2^31 - 2 nodes or 2^30 - 1 edges");
        rows += h_sel_nodes[i];
        edges += h_sel_edges[i];
        HKSS_REQUIRE(rows < (1ll << 31) - 1 && edges < (1ll << 30), "the selection exceeds 2^31 - 2 nodes or 2^30 - 1 edges");
    }
    return TLC_OK;
}

template <bool DT>
int hkss_run(const char* fn, const int64_t* d_node_ptr, const int64_t* d_edge_ptr, const int32_t* d_edges, int64_t n_graphs, int64_t total_nodes,
             int64_t total_edges, const int64_t* h_sel, const int64_t* h_sel_nodes, const int64_t* h_sel_edges, int64_t n_sel, const double* h_times,
             int32_t n_times, uint32_t flags, double* d_out, double* d_dout, uint8_t* d_status, void* d_work, int64_t work_bytes, void* stream) {
    HKSS_REQUIRE(n_graphs >= 0 && n_graphs < (1ll << 31) && total_nodes >= 0 && total_edges >= 0, "bad sizes");
    HKSS_REQUIRE(n_sel >= 0 && n_sel <= n_graphs, "n_sel outside 0 .. n_graphs");
    HKSS_REQUIRE(h_times && n_times >= 1 && n_times <= TLC_HKS_TMAX, "n_times outside 1 .. TLC_HKS_TMAX");
    HKSS_REQUIRE((flags & ~TLC_HKS_NORMALISE) == 0, "unknown flag");
    for (int i = 0; i < n_times; ++i)
        HKSS_REQUIRE(isfinite(h_times[i]) && h_times[i] >= 0.0 && h_times[i] <= TLC_HKS_SPARSE_TIME_MAX, "a time outside [0, TLC_HKS_SPARSE_TIME_MAX]");
    if (DT) HKSS_REQUIRE(d_dout || total_nodes == 0, "null d_dout");
    HKSS_REQUIRE(n_sel == 0 || (h_sel && h_sel_nodes && h_sel_edges), "null pointer");
    for (int64_t i = 0; i < n_sel; ++i)
        HKSS_REQUIRE(h_sel[i] >= 0 && h_sel[i] < n_graphs && (i == 0 || h_sel[i] > h_sel[i - 1]), "h_sel is not strictly ascending inside 0 .. n_graphs-1");
    const int rc = hkss_check_sizes(fn, h_sel_nodes, h_sel_edges, n_sel);
    if (rc != TLC_OK) return rc;
    if (n_sel == 0) return TLC_OK;
    HKSS_REQUIRE(d_node_ptr && d_edge_ptr && d_status && d_work && (total_nodes == 0 || d_out) && (total_edges == 0 || d_edges), "null pointer");
    const TlcHksSparseScratch L(h_sel_nodes, h_sel_edges, n_sel, rk_hist_ints(TlcHksSparseScratch::entries_of(h_sel_edges, n_sel)), RK_TOT_INTS);
    HKSS_REQUIRE(work_bytes >= L.least + 256, "d_work is smaller than tlc_hks_sparse_work_bytes()'s min_bytes");
    HKSS_REQUIRE((reinterpret_cast<uintptr_t>(d_work) & 15) == 0, "d_work must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    char* w = tlc_align256(d_work);
    const int64_t avail = work_bytes - 256 - L.panels;         // bytes of panels that fit (>= the largest panel)
    HkssDesc* descs = reinterpret_cast<HkssDesc*>(w + L.descs);
    int* state = reinterpret_cast<int*>(w + L.state);
    unsigned long long *ka = reinterpret_cast<unsigned long long*>(w + L.key_a), *kb = reinterpret_cast<unsigned long long*>(w + L.key_b);
    unsigned char *la = reinterpret_cast<unsigned char*>(w + L.lab_a), *lb = reinterpret_cast<unsigned char*>(w + L.lab_b);
    int* col = reinterpret_cast<int*>(w + L.col);
    int* rowptr = reinterpret_cast<int*>(w + L.rowptr);
    double* rinv = reinterpret_cast<double*>(w + L.rinv);
    int* slotrow = reinterpret_cast<int*>(w + L.slotrow);
    int* hist = reinterpret_cast<int*>(w + L.hist);
    int* tot = reinterpret_cast<int*>(w + L.tot);
    const int S = (int)n_sel, rows = (int)L.rows, n_ent = (int)L.entries;
    const long long* np = (const long long*)d_node_ptr;
    const long long* ep = (const long long*)d_edge_ptr;

    // ---- once per call: descriptors, checks, the CSR of the selection ----
    {
        HkssChunk C;
        int64_t pb = 0, bc = 0, rb = 0, eb = 0, sb = 0;
        for (int64_t k0 = 0; k0 < n_sel; k0 += HKSS_CHUNK) {
            C.panel_base = pb; C.buf_cum = bc; C.row_base = (int)rb; C.ent_base = (int)eb; C.slot_base = (int)sb;
            C.count = (int)(n_sel - k0 < HKSS_CHUNK ? n_sel - k0 : HKSS_CHUNK);
            C.first = (int)k0;
            for (int k = 0; k < HKSS_CHUNK; ++k) {
                const int64_t n = k < C.count ? h_sel_nodes[k0 + k] : 0, m = k < C.count ? h_sel_edges[k0 + k] : 0;
                C.g[k] = k < C.count ? (int)h_sel[k0 + k] : 0;
                C.n[k] = (int)n; C.m[k] = (int)m;
                const int64_t nb = TlcHksSparseScratch::blocks_of(n);
                pb += nb; bc += nb * TlcHksSparseScratch::panel_doubles(n, 2 * m);
                rb += n; eb += 2 * m; sb += TlcHksSparseScratch::slots_of(2 * m);
            }
            hipLaunchKernelGGL(hkss_setup_kernel, dim3(1), dim3(HKSS_CHUNK), 0, s, C, descs);
            TLC_HIP_CHECK(hipGetLastError());
        }
    }
    const unsigned gsel = (unsigned)((S + 255) / 256);
    hipLaunchKernelGGL(hkss_head_kernel, dim3(gsel), dim3(256), 0, s, (const HkssDesc*)descs, S, (long long)total_nodes, (long long)total_edges, np, ep, state);
    TLC_HIP_CHECK(hipGetLastError());
    const unsigned long long* keys = ka;
    if (n_ent > 0) {
        hipLaunchKernelGGL(hkss_emit_kernel, dim3((unsigned)((n_ent / 2 + 255) / 256)), dim3(256), 0, s, (const HkssDesc*)descs, S, (long long)(n_ent / 2), ep,
                           (const int*)d_edges, state, ka);
        TLC_HIP_CHECK(hipGetLastError());
        // the digits that can differ: the column's bytes up to the largest graph's, the row's up to `rows` (<= 256^nh - 1, so that no
        // row's digits are all ones and the ~0 keys of what is not computed sort behind every entry); every other digit of an entry is 0
        int nl = 1, nh = 1;
        while (nl < 4 && (L.max_n - 1) >> (8 * nl)) ++nl;
        while (nh < 4 && (int64_t)rows > (1ll << (8 * nh)) - 1) ++nh;
        if (n_ent > 1) {
            unsigned long long *kin = ka, *kout = kb;
            unsigned char *lin = la, *lout = lb;
            for (int p = 0; p < nl + nh; ++p) {
                rk_pass(s, (long long)n_ent, p < nl ? 8 * p : 32 + 8 * (p - nl), kin, lin, kout, lout, hist, tot);
                TLC_HIP_CHECK(hipGetLastError());
                std::swap(kin, kout);
                std::swap(lin, lout);
            }
            keys = kin;
        }
        hipLaunchKernelGGL(hkss_cols_kernel, dim3((unsigned)((n_ent + 255) / 256)), dim3(256), 0, s, (const HkssDesc*)descs, S, keys, n_ent, col, state);
        TLC_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(hkss_rowptr_kernel, dim3((unsigned)(((int64_t)rows + 1 + 255) / 256)), dim3(256), 0, s, keys, n_ent, rows, rowptr);
    TLC_HIP_CHECK(hipGetLastError());
    TLC_HIP_CHECK(hipMemsetAsync(slotrow, 0xFF, (size_t)L.slots * sizeof(int), s));
    if (rows > 0) {
        hipLaunchKernelGGL(hkss_rows_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, (const HkssDesc*)descs, S, rows, (const int*)rowptr,
                           (const int*)state, rinv, slotrow);
        TLC_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(hkss_status_kernel, dim3(gsel), dim3(256), 0, s, (const HkssDesc*)descs, S, (const int*)state, d_status);
    TLC_HIP_CHECK(hipGetLastError());

    // ---- the groups of panels ----
    HkssCtx C;
    C.descs = descs; C.state = state; C.rowptr = rowptr; C.col = col; C.rinv = rinv; C.slotrow = slotrow;
    C.bufs = reinterpret_cast<double*>(w + L.panels);
    C.n_sel = S;
    int64_t gi = 0, pj = 0, panel_cum = 0, buf_cum = 0;          // the next panel: panel pj of graph gi; what lies before graph gi
    while (gi < n_sel) {
        const int64_t nb_g = TlcHksSparseScratch::blocks_of(h_sel_nodes[gi]);
        if (pj >= nb_g) {
            panel_cum += nb_g;
            buf_cum += nb_g * TlcHksSparseScratch::panel_doubles(h_sel_nodes[gi], 2 * h_sel_edges[gi]);
            ++gi; pj = 0;
            continue;
        }
        C.first_panel = panel_cum + pj;
        C.buf0 = buf_cum + pj * TlcHksSparseScratch::panel_doubles(h_sel_nodes[gi], 2 * h_sel_edges[gi]);
        int64_t used = 0, count = 0, max_n = 0, max_slots = 0;
        bool may_split = false;                                // a graph that is computed is simple: no row is longer than min(n - 1, m)
        int64_t gj = gi, pk = pj, pc = panel_cum, bc = buf_cum;
        while (gj < n_sel && count < (1ll << 30)) {             // panels from (gj, pk) on, as many as fit
            const int64_t n = h_sel_nodes[gj], nb = TlcHksSparseScratch::blocks_of(n), pd = TlcHksSparseScratch::panel_doubles(n, 2 * h_sel_edges[gj]);
            if (pk >= nb) { pc += nb; bc += nb * pd; ++gj; pk = 0; continue; }
            int64_t take = (avail - used) / (pd * 8);
            if (take > nb - pk) take = nb - pk;
            if (take > (1ll << 30) - count) take = (1ll << 30) - count;
            if (take <= 0) break;
            used += take * pd * 8; count += take; pk += take;
            if (n > max_n) max_n = n;
            if (n - 1 > HKSS_LONG && h_sel_edges[gj] > HKSS_LONG) may_split = true;
            if (TlcHksSparseScratch::slots_of(2 * h_sel_edges[gj]) > max_slots) max_slots = TlcHksSparseScratch::slots_of(2 * h_sel_edges[gj]);
        }
        if (count <= 0) {
            tlc_set_error("%s: internal: a panel does not fit its workspace", fn);
            return TLC_ERR_INVALID_ARG;
        }
        C.n_panels = (int)count;
        const dim3 grid_rows((unsigned)((max_n + HKSS_ROWS_PER_WG - 1) / HKSS_ROWS_PER_WG), hkss_grid_y(count));
        const dim3 grid_slots((unsigned)((max_slots + 3) / 4), hkss_grid_y(count));
        const dim3 grid_blocks((unsigned)((TlcHksSparseScratch::blocks_of(max_n) + 3) / 4), hkss_grid_y(count));
        for (int t = 0; t < n_times; ++t) {
            const double tau = h_times[t] * 0.5, factor = exp(-tau);
            const int K = tlc_hks_sparse_terms(h_times[t]);
            int cur = 1;                                       // which of s (1) / s' (2) holds the step's input
            hipLaunchKernelGGL(hkss_init_kernel, grid_rows, dim3(256), 0, s, C, cur);
            TLC_HIP_CHECK(hipGetLastError());
            for (int k = 1; k <= K; ++k) {
                if (may_split) hipLaunchKernelGGL(hkss_part_kernel, grid_slots, dim3(256), 0, s, C, cur);
                hipLaunchKernelGGL(hkss_step_kernel<false>, grid_rows, dim3(256), 0, s, C, cur, 3 - cur, tau / (double)k);
                TLC_HIP_CHECK(hipGetLastError());
                cur = 3 - cur;
            }
            hipLaunchKernelGGL(hkss_scale_kernel, grid_rows, dim3(256), 0, s, C, cur, factor);
            TLC_HIP_CHECK(hipGetLastError());
            double* out_t = d_out + (size_t)t * (size_t)total_nodes;
            double* dout_t = DT ? d_dout + (size_t)t * (size_t)total_nodes : nullptr;
            if (DT) {
                if (may_split) hipLaunchKernelGGL(hkss_part_kernel, grid_slots, dim3(256), 0, s, C, cur);
                hipLaunchKernelGGL(hkss_step_kernel<true>, grid_rows, dim3(256), 0, s, C, cur, 3 - cur, 0.0);
                TLC_HIP_CHECK(hipGetLastError());
            }
            hipLaunchKernelGGL(hkss_red1_kernel<DT>, grid_blocks, dim3(256), 0, s, C, 3 - cur);
            hipLaunchKernelGGL(hkss_red2_kernel<DT>, dim3((unsigned)((count + 3) / 4)), dim3(256), 0, s, C, np, out_t, dout_t);
            TLC_HIP_CHECK(hipGetLastError());
        }
        gi = gj; pj = pk; panel_cum = pc; buf_cum = bc;
    }
    if (flags & TLC_HKS_NORMALISE)
        for (int t = 0; t < n_times; ++t) {
            hipLaunchKernelGGL(hkss_norm_kernel<DT>, dim3((unsigned)S), dim3(256), 0, s, (const HkssDesc*)descs, (const int*)state, np,
                               d_out + (size_t)t * (size_t)total_nodes, DT ? d_dout + (size_t)t * (size_t)total_nodes : nullptr);
            TLC_HIP_CHECK(hipGetLastError());
        }
    return TLC_OK;
}
#undef HKSS_REQUIRE

}  // namespace

extern "C" int tlc_hks_sparse_work_bytes(const int64_t* h_sel_nodes, const int64_t* h_sel_edges, int64_t n_sel, int32_t n_times, int64_t* min_bytes,
                                         int64_t* all_bytes) {
    TLC_REQUIRE(min_bytes && all_bytes, "null pointer");
    TLC_REQUIRE(n_times >= 1 && n_times <= TLC_HKS_TMAX, "n_times outside 1 .. TLC_HKS_TMAX");
    const int rc = hkss_check_sizes(__func__, h_sel_nodes, h_sel_edges, n_sel);
    if (rc != TLC_OK) return rc;
    const TlcHksSparseScratch L(h_sel_nodes, h_sel_edges, n_sel, rk_hist_ints(TlcHksSparseScratch::entries_of(h_sel_edges, n_sel)), RK_TOT_INTS);
    *min_bytes = n_sel ? L.least + 256 : 0;                    // (256: the alignment of the caller's pointer)
    *all_bytes = n_sel ? L.total + 256 : 0;
    return TLC_OK;
}

extern "C" int tlc_hks_sparse_batch(const int64_t* d_node_ptr, const int64_t* d_edge_ptr, const int32_t* d_edges, int64_t n_graphs, int64_t total_nodes,
                                    int64_t total_edges, const int64_t* h_sel, const int64_t* h_sel_nodes, const int64_t* h_sel_edges, int64_t n_sel,
                                    const double* h_times, int32_t n_times, uint32_t flags, double* d_out, uint8_t* d_status, void* d_work,
                                    int64_t work_bytes, void* stream) {
    return hkss_run<false>(__func__, d_node_ptr, d_edge_ptr, d_edges, n_graphs, total_nodes, total_edges, h_sel, h_sel_nodes, h_sel_edges, n_sel, h_times,
                           n_times, flags, d_out, nullptr, d_status, d_work, work_bytes, stream);
}

extern "C" int tlc_hks_sparse_batch_dt(const int64_t* d_node_ptr, const int64_t* d_edge_ptr, const int32_t* d_edges, int64_t n_graphs,
                                       int64_t total_nodes, int64_t total_edges, const int64_t* h_sel, const int64_t* h_sel_nodes,
                                       const int64_t* h_sel_edges, int64_t n_sel, const double* h_times, int32_t n_times, uint32_t flags,
                                       double* d_out, double* d_dout, uint8_t* d_status, void* d_work, int64_t work_bytes, void* stream) {
    return hkss_run<true>(__func__, d_node_ptr, d_edge_ptr, d_edges, n_graphs, total_nodes, total_edges, h_sel, h_sel_nodes, h_sel_edges, n_sel, h_times,
                          n_times, flags, d_out, d_dout, d_status, d_work, work_bytes, stream);
}

// pd_grad.hip -- d diagram / d filtration of the exact extended persistence (tlc_pd_point_vertices, tlc_pd_filtration_grad;
// DESIGN.md 6.6).  Every coordinate of every point tlc_pd_from_filtration / tlc_pd_wide write is a copy of one f[v], so the
// Jacobian is a 0/1 selection matrix; the forward kernels return the values only, and this file recovers the vertices from them:
//
//     the vertex of a coordinate c of graph g is the LOWEST local id v in 0 .. n_g-1 with f[node_offs[g] + v] == c  (IEEE ==:
//     -0.0 matches +0.0, a NaN matches nothing).
//
// With pairwise distinct values that is the critical vertex of the pairing; under ties (where the diagram is not differentiable
// in f) it is a fixed convention, the same in every class below and for both forward entries.  The backward sums, per vertex, the
// gradients of the coordinates it owns in fp64 from +0.0 in one fixed order -- up rows ascending (birth, death), down rows, one
// rows, ext0 (birth, death) -- without a floating-point atomic, so a graph's bits depend on nothing but its own inputs.
//
// Classes by node count, cut on the device from the offsets (every kernel skips the graphs of the other classes):
//   n <= TLC_PD_VERT_WAVE_NMAX   one wavefront per graph, PDG_BS / 64 graphs per workgroup, grid-stride over the batch.  Lane v holds
//                                f[v]; a coordinate's vertex is the lowest set bit of the ballot of f == c.  Backward: the coordinates
//                                are walked in the fixed order and lane v adds where the id is v.
//   n <= TLC_PD_VERT_LDS_NMAX    one workgroup per graph: (order-preserving key, id) sorted in LDS by a bitonic network (12 B per
//                                node), one lane per coordinate searches the lower bound -- the first equal entry has the lowest id.
//                                Backward: the grad slice in LDS, thread t owns the vertices v = t (mod PDG_BS) and the coordinates
//                                pass by in the fixed order, a chunk of PDG_BS at a time.
//   above                        the whole device, one graph after the other: radix_passes.h sorts (key, id) in the workspace, a
//                                grid-stride kernel searches from global memory.  Backward: the coordinates' slot positions are
//                                radix-sorted stably by vertex -- a CSR by vertex in the fixed order -- and one thread per vertex sums
//                                its run.
// The entries read the batch's offsets back once (to find the graphs of the third class and to size their launches) before they
// launch anything.
#include "radix_passes.h"

#include <stdlib.h>

namespace {

#define PDG_BS 256
#define PDG_WAVES (PDG_BS / 64)
#define PDG_MAX_GRID 2048
#define PDG_WAVE_N TLC_PD_VERT_WAVE_NMAX
#define PDG_LDS_N TLC_PD_VERT_LDS_NMAX
#define PDG_NOID 0xffffffffu
static_assert(PDG_BS == RK_BS, "the radix passes and the kernels here share one workgroup width");
static_assert(PDG_WAVE_N == 64, "one lane per node");
static_assert((PDG_LDS_N & (PDG_LDS_N - 1)) == 0, "the bitonic network sorts a power of two");

// what the offsets and the counts row say about graph g
struct Shape {
    long long no, eo, n, m;
    int cu, cd, c1;        // points of the three slots
    int status;            // TLC_ST_*
    bool run;              // status OK and n > 0: there is something to compute
};
__device__ __forceinline__ Shape graph_shape(const int64_t* __restrict__ node_offs, const int64_t* __restrict__ edge_offs,
                                             const int32_t* __restrict__ counts, long long g) {
    Shape s;
    s.no = node_offs[g];
    s.eo = edge_offs[g];
    s.n = node_offs[g + 1] - s.no;
    s.m = edge_offs[g + 1] - s.eo;
    s.cu = s.cd = s.c1 = 0;
    s.run = false;
    s.status = TLC_ST_OK;
    if (s.no < 0 || s.eo < 0 || s.n < 0 || s.m < 0) { s.status = TLC_ST_BAD_INPUT; return s; }
    if (s.n == 0) return s;
    const int cu = counts[4 * g], cd = counts[4 * g + 1], c1 = counts[4 * g + 2];
    if (cu == -1 && cd == -1 && c1 == -1) { s.status = TLC_ST_TOO_LARGE; return s; }
    if (cu < 0 || cd < 0 || c1 < 0 || cu > s.n || cd > s.n || c1 > s.m) { s.status = TLC_ST_BAD_INPUT; return s; }
    if (s.n + s.m > TLC_PD_WIDE_MAX_ITEMS) { s.status = TLC_ST_TOO_LARGE; return s; }
    s.cu = cu; s.cd = cd; s.c1 = c1;
    s.run = true;
    return s;
}

struct VertArgs {
    long long n_graphs;
    const int64_t *node_offs, *edge_offs;
    const double *f, *pd_up, *pd_down, *pd_one, *ext0;
    const int32_t* counts;
    int32_t *v_up, *v_down, *v_one, *v_ext0;
    uint8_t* status;
};
struct GradArgs {
    long long n_graphs;
    const int64_t *node_offs, *edge_offs;
    const int32_t* counts;
    const int32_t *v_up, *v_down, *v_one, *v_ext0;
    const double *g_up, *g_down, *g_one, *g_ext0;     // each may be NULL: zeros
    const uint8_t* status;
    double* grad_f;
};

// ---- n <= 64: one wavefront per graph ----------------------------------------------------------------------------------------
// ids of the coordinates src[0 .. valid), -1 into dst[valid .. total); true if a coordinate matched no lane.  All arguments but fv /
// has are uniform over the wavefront.
__device__ __forceinline__ bool wave_slot_ids(double fv, bool has, const double* __restrict__ src, int valid, int total,
                                              int32_t* __restrict__ dst, int lane) {
    bool bad = false;
    for (int base = 0; base < total; base += 64) {
        const int j = base + lane;
        const double c = j < valid ? src[j] : 0.0;
        int id = -1;
        const int lim = valid - base < 64 ? valid - base : 64;
        for (int k = 0; k < lim; ++k) {
            const double ck = __shfl(c, k);
            const unsigned long long b = __ballot(has && fv == ck);
            if (lane == k) id = b ? __ffsll((unsigned long long)b) - 1 : -1;
        }
        if (j < valid && id < 0) bad = true;
        if (j < total) dst[j] = id;
    }
    return bad;
}
__global__ __launch_bounds__(PDG_BS) void pdg_wave_vertices_kernel(VertArgs A) {
    const int lane = (int)(threadIdx.x & 63);
    const long long w0 = (long long)blockIdx.x * PDG_WAVES + (threadIdx.x >> 6), stride = (long long)gridDim.x * PDG_WAVES;
    for (long long g = w0; g < A.n_graphs; g += stride) {
        const Shape s = graph_shape(A.node_offs, A.edge_offs, A.counts, g);
        if (!s.run) {                                      // this kernel writes the status of every graph nothing is computed for
            if (lane == 0) A.status[g] = (uint8_t)s.status;
            continue;
        }
        if (s.n > PDG_WAVE_N) continue;
        const int n = (int)s.n, m = (int)s.m;
        const bool has = lane < n;
        const double fv = has ? A.f[s.no + lane] : 0.0;
        bool bad = wave_slot_ids(fv, has, A.pd_up + 2 * s.no, 2 * s.cu, 2 * n, A.v_up + 2 * s.no, lane);
        bad |= wave_slot_ids(fv, has, A.pd_down + 2 * s.no, 2 * s.cd, 2 * n, A.v_down + 2 * s.no, lane);
        bad |= wave_slot_ids(fv, has, A.pd_one + 2 * s.eo, 2 * s.c1, 2 * m, A.v_one + 2 * s.eo, lane);
        bad |= wave_slot_ids(fv, has, A.ext0 + 2 * g, 2, 2, A.v_ext0 + 2 * g, lane);
        const bool any_bad = __any(bad);
        if (lane == 0) A.status[g] = (uint8_t)(any_bad ? TLC_ST_BAD_INPUT : TLC_ST_OK);
    }
}
__device__ __forceinline__ double wave_slot_sum(double acc, const int32_t* __restrict__ ids, const double* __restrict__ gr, int valid,
                                                int lane) {
    for (int base = 0; base < valid; base += 64) {
        const int j = base + lane;
        int id = -1;
        double gv = 0.0;
        if (j < valid) {
            id = ids[j];
            if (gr) gv = gr[j];
        }
        const int lim = valid - base < 64 ? valid - base : 64;
        for (int k = 0; k < lim; ++k) {
            const int idk = __shfl(id, k);
            const double gk = __shfl(gv, k);
            if (lane == idk) acc += gk;
        }
    }
    return acc;
}
__global__ __launch_bounds__(PDG_BS) void pdg_wave_grad_kernel(GradArgs A) {
    const int lane = (int)(threadIdx.x & 63);
    const long long w0 = (long long)blockIdx.x * PDG_WAVES + (threadIdx.x >> 6), stride = (long long)gridDim.x * PDG_WAVES;
    for (long long g = w0; g < A.n_graphs; g += stride) {
        if (A.status[g] != TLC_ST_OK) continue;
        const Shape s = graph_shape(A.node_offs, A.edge_offs, A.counts, g);
        if (!s.run || s.n > PDG_WAVE_N) continue;
        double acc = 0.0;
        acc = wave_slot_sum(acc, A.v_up + 2 * s.no, A.g_up ? A.g_up + 2 * s.no : nullptr, 2 * s.cu, lane);
        acc = wave_slot_sum(acc, A.v_down + 2 * s.no, A.g_down ? A.g_down + 2 * s.no : nullptr, 2 * s.cd, lane);
        acc = wave_slot_sum(acc, A.v_one + 2 * s.eo, A.g_one ? A.g_one + 2 * s.eo : nullptr, 2 * s.c1, lane);
        acc = wave_slot_sum(acc, A.v_ext0 + 2 * g, A.g_ext0 ? A.g_ext0 + 2 * g : nullptr, 2, lane);
        if (lane < (int)s.n) A.grad_f[s.no + lane] = acc;
    }
}

// ---- 65 .. 2048 nodes: one workgroup per graph --------------------------------------------------------------------------------
// first position in key[0 .. n) that is not below kc
template <typename KeyPtr>
__device__ __forceinline__ int lower_bound_u64(KeyPtr key, int n, unsigned long long kc) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (key[mid] < kc) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
// the id of coordinate c from the sorted (key, id) pairs, -1 if no vertex holds it
template <typename KeyPtr, typename IdPtr>
__device__ __forceinline__ int find_vertex(KeyPtr key, IdPtr vid, int n, double c) {
    if (c != c) return -1;
    const unsigned long long kc = tlc_ord_f64(c);
    const int p = lower_bound_u64(key, n, kc);
    return (p < n && key[p] == kc) ? (int)vid[p] : -1;
}
__device__ __forceinline__ bool lds_slot_ids(const unsigned long long* key, const unsigned* vid, int n, const double* __restrict__ src,
                                             int valid, int total, int32_t* __restrict__ dst) {
    bool bad = false;
    for (int j = threadIdx.x; j < total; j += PDG_BS) {
        int id = -1;
        if (j < valid) {
            id = find_vertex(key, vid, n, src[j]);
            bad |= id < 0;
        }
        dst[j] = id;
    }
    return bad;
}
__global__ __launch_bounds__(PDG_BS) void pdg_lds_vertices_kernel(VertArgs A) {
    __shared__ unsigned long long key[PDG_LDS_N];
    __shared__ unsigned vid[PDG_LDS_N];
    __shared__ int sbad;
    const int tid = (int)threadIdx.x;
    for (long long g = blockIdx.x; g < A.n_graphs; g += gridDim.x) {
        const Shape s = graph_shape(A.node_offs, A.edge_offs, A.counts, g);
        if (!s.run || s.n <= PDG_WAVE_N || s.n > PDG_LDS_N) continue;        // uniform over the workgroup
        const int n = (int)s.n, m = (int)s.m;
        int P = 128;
        while (P < n) P <<= 1;
        for (int i = tid; i < P; i += PDG_BS) {
            key[i] = i < n ? tlc_ord_f64(A.f[s.no + i]) : ~0ull;
            vid[i] = i < n ? (unsigned)i : PDG_NOID;
        }
        if (tid == 0) sbad = 0;
        __syncthreads();
        for (int k = 2; k <= P; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int t = tid; t < (P >> 1); t += PDG_BS) {
                    const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                    const unsigned long long ki = key[i], kl = key[l];
                    const unsigned vi = vid[i], vl = vid[l];
                    const bool gt = ki > kl || (ki == kl && vi > vl);
                    if (gt == ((i & k) == 0)) {
                        key[i] = kl; key[l] = ki;
                        vid[i] = vl; vid[l] = vi;
                    }
                }
                __syncthreads();
            }
        bool bad = lds_slot_ids(key, vid, n, A.pd_up + 2 * s.no, 2 * s.cu, 2 * n, A.v_up + 2 * s.no);
        bad |= lds_slot_ids(key, vid, n, A.pd_down + 2 * s.no, 2 * s.cd, 2 * n, A.v_down + 2 * s.no);
        bad |= lds_slot_ids(key, vid, n, A.pd_one + 2 * s.eo, 2 * s.c1, 2 * m, A.v_one + 2 * s.eo);
        bad |= lds_slot_ids(key, vid, n, A.ext0 + 2 * g, 2, 2, A.v_ext0 + 2 * g);
        if (bad) sbad = 1;
        __syncthreads();
        if (tid == 0) A.status[g] = (uint8_t)(sbad ? TLC_ST_BAD_INPUT : TLC_ST_OK);
        __syncthreads();                                    // key / vid / sbad are the next graph's
    }
}
// the coordinates of one slot pass by in order, PDG_BS at a time; thread t adds those whose vertex is t (mod PDG_BS)
__device__ __forceinline__ void lds_slot_sum(double* sg, int* cid, double* cg, int n, const int32_t* __restrict__ ids,
                                             const double* __restrict__ gr, int valid) {
    const int tid = (int)threadIdx.x;
    for (int base = 0; base < valid; base += PDG_BS) {
        const int j = base + tid;
        cid[tid] = j < valid ? ids[j] : -1;
        cg[tid] = (j < valid && gr) ? gr[j] : 0.0;
        __syncthreads();
        const int lim = valid - base < PDG_BS ? valid - base : PDG_BS;
        for (int k = 0; k < lim; ++k) {
            const int id = cid[k];
            if (id >= 0 && id < n && (id & (PDG_BS - 1)) == tid) sg[id] += cg[k];
        }
        __syncthreads();
    }
}
__global__ __launch_bounds__(PDG_BS) void pdg_lds_grad_kernel(GradArgs A) {
    __shared__ double sg[PDG_LDS_N];
    __shared__ double cg[PDG_BS];
    __shared__ int cid[PDG_BS];
    const int tid = (int)threadIdx.x;
    for (long long g = blockIdx.x; g < A.n_graphs; g += gridDim.x) {
        if (A.status[g] != TLC_ST_OK) continue;
        const Shape s = graph_shape(A.node_offs, A.edge_offs, A.counts, g);
        if (!s.run || s.n <= PDG_WAVE_N || s.n > PDG_LDS_N) continue;
        const int n = (int)s.n;
        for (int i = tid; i < n; i += PDG_BS) sg[i] = 0.0;
        __syncthreads();
        lds_slot_sum(sg, cid, cg, n, A.v_up + 2 * s.no, A.g_up ? A.g_up + 2 * s.no : nullptr, 2 * s.cu);
        lds_slot_sum(sg, cid, cg, n, A.v_down + 2 * s.no, A.g_down ? A.g_down + 2 * s.no : nullptr, 2 * s.cd);
        lds_slot_sum(sg, cid, cg, n, A.v_one + 2 * s.eo, A.g_one ? A.g_one + 2 * s.eo : nullptr, 2 * s.c1);
        lds_slot_sum(sg, cid, cg, n, A.v_ext0 + 2 * g, A.g_ext0 ? A.g_ext0 + 2 * g : nullptr, 2);
        for (int i = tid; i < n; i += PDG_BS) A.grad_f[s.no + i] = sg[i];
        __syncthreads();
    }
}

// ---- above 2048 nodes: the whole device, one graph at a time -----------------------------------------------------------------
// The coordinates of a graph in slot positions p = 0 .. 4 n + 2 m + 1: up [0, 2n), down [2n, 4n), one [4n, 4n + 2m), ext0 the last two.
// Ascending p among the point rows is the fixed summation order.
enum { W_STATUS = 0, W_BAD, W_CU, W_CD, W_C1, W_INTS = 8 };
struct Slot {
    int which;             // 0 up, 1 down, 2 one, 3 ext0
    long long j;           // coordinate inside the slot
    bool valid;            // inside the slot's point rows
};
__device__ __forceinline__ Slot slot_of(long long p, long long n, long long m, const int* ctl) {
    Slot s;
    if (p < 2 * n) { s.which = 0; s.j = p; s.valid = p < 2ll * ctl[W_CU]; }
    else if (p < 4 * n) { s.which = 1; s.j = p - 2 * n; s.valid = s.j < 2ll * ctl[W_CD]; }
    else if (p < 4 * n + 2 * m) { s.which = 2; s.j = p - 4 * n; s.valid = s.j < 2ll * ctl[W_C1]; }
    else { s.which = 3; s.j = p - 4 * n - 2 * m; s.valid = true; }
    return s;
}
#define PDG_FOR(i, count) \
    for (long long i = (long long)blockIdx.x * PDG_BS + threadIdx.x; i < (count); i += (long long)gridDim.x * PDG_BS)

__global__ void pdgw_ctl_kernel(int* __restrict__ ctl, const int64_t* __restrict__ node_offs, const int64_t* __restrict__ edge_offs,
                                const int32_t* __restrict__ counts, const uint8_t* __restrict__ status_in, long long g) {
    if (threadIdx.x != 0) return;
    const Shape s = graph_shape(node_offs, edge_offs, counts, g);
    int st = s.status;
    if (status_in && status_in[g] != TLC_ST_OK) st = status_in[g];
    ctl[W_STATUS] = st;
    ctl[W_BAD] = 0;
    ctl[W_CU] = s.cu; ctl[W_CD] = s.cd; ctl[W_C1] = s.c1;
}
__global__ __launch_bounds__(PDG_BS) void pdgw_keys_kernel(const int* __restrict__ ctl, long long n, const double* __restrict__ f,
                                                           unsigned long long* __restrict__ key, unsigned* __restrict__ val) {
    if (ctl[W_STATUS] != TLC_ST_OK) return;
    PDG_FOR(v, n) {
        key[v] = tlc_ord_f64(f[v]);
        val[v] = (unsigned)v;
    }
}
__global__ __launch_bounds__(PDG_BS) void pdgw_search_kernel(int* __restrict__ ctl, long long n, long long m, const unsigned long long* __restrict__ key,
                                                             const unsigned* __restrict__ val, const double* __restrict__ pd_up,
                                                             const double* __restrict__ pd_down, const double* __restrict__ pd_one,
                                                             const double* __restrict__ ext0, int32_t* __restrict__ v_up,
                                                             int32_t* __restrict__ v_down, int32_t* __restrict__ v_one,
                                                             int32_t* __restrict__ v_ext0) {
    if (ctl[W_STATUS] != TLC_ST_OK) return;
    PDG_FOR(p, 4 * n + 2 * m + 2) {
        const Slot s = slot_of(p, n, m, ctl);
        const double* src = s.which == 0 ? pd_up : s.which == 1 ? pd_down : s.which == 2 ? pd_one : ext0;
        int32_t* dst = s.which == 0 ? v_up : s.which == 1 ? v_down : s.which == 2 ? v_one : v_ext0;
        int id = -1;
        if (s.valid) {
            id = find_vertex(key, val, (int)n, src[s.j]);
            if (id < 0) ctl[W_BAD] = 1;
        }
        dst[s.j] = id;
    }
}
__global__ void pdgw_status_kernel(const int* __restrict__ ctl, uint8_t* __restrict__ status) {
    if (threadIdx.x == 0) *status = (uint8_t)(ctl[W_STATUS] != TLC_ST_OK ? ctl[W_STATUS] : ctl[W_BAD] ? TLC_ST_BAD_INPUT : TLC_ST_OK);
}
// sort items of the backward: key = the vertex of the coordinate at slot position p (PDG_NOID behind the points), payload = p
__global__ __launch_bounds__(PDG_BS) void pdgw_items_kernel(const int* __restrict__ ctl, long long n, long long m, const int32_t* __restrict__ v_up,
                                                            const int32_t* __restrict__ v_down, const int32_t* __restrict__ v_one,
                                                            const int32_t* __restrict__ v_ext0, unsigned* __restrict__ key,
                                                            unsigned* __restrict__ val) {
    if (ctl[W_STATUS] != TLC_ST_OK) return;
    PDG_FOR(p, 4 * n + 2 * m + 2) {
        const Slot s = slot_of(p, n, m, ctl);
        const int32_t* src = s.which == 0 ? v_up : s.which == 1 ? v_down : s.which == 2 ? v_one : v_ext0;
        unsigned k = PDG_NOID;
        if (s.valid) {
            const int id = src[s.j];
            if (id >= 0 && id < n) k = (unsigned)id;
        }
        key[p] = k;
        val[p] = (unsigned)p;
    }
}
__global__ __launch_bounds__(PDG_BS) void pdgw_sum_kernel(const int* __restrict__ ctl, long long n, long long m, const unsigned* __restrict__ key,
                                                          const unsigned* __restrict__ val, const double* __restrict__ g_up,
                                                          const double* __restrict__ g_down, const double* __restrict__ g_one,
                                                          const double* __restrict__ g_ext0, double* __restrict__ grad_f) {
    if (ctl[W_STATUS] != TLC_ST_OK) return;
    const long long T = 4 * n + 2 * m + 2;
    PDG_FOR(v, n) {
        long long lo = 0, hi = T;
        while (lo < hi) {
            const long long mid = (lo + hi) >> 1;
            if (key[mid] < (unsigned)v) lo = mid + 1;
            else hi = mid;
        }
        double acc = 0.0;
        for (; lo < T && key[lo] == (unsigned)v; ++lo) {
            const Slot s = slot_of((long long)val[lo], n, m, ctl);
            const double* src = s.which == 0 ? g_up : s.which == 1 ? g_down : s.which == 2 ? g_one : g_ext0;
            acc += src ? src[s.j] : 0.0;
        }
        grad_f[v] = acc;
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------
struct WLay {
    size_t ctl, key_a, key_b, val_a, val_b, hist, tot, bytes;
};
// workspace of one graph of the third class: the forward sorts n (u64 key, u32 id) pairs, the backward T = 4 n + 2 m + 2 (u32, u32)
WLay wlayout(long long n, long long m) {
    WLay L;
    TlcCarver W;
    const long long T = 4 * n + 2 * m + 2;
    L.ctl = W.take(W_INTS, 4);
    L.key_a = W.take(T, 4); L.key_b = W.take(T, 4);      // 4 T >= 8 n bytes: room for the forward's u64 keys
    L.val_a = W.take(T, 4); L.val_b = W.take(T, 4);
    L.hist = W.take(rk_hist_ints(T), 4); L.tot = W.take(RK_TOT_INTS, 4);
    L.bytes = W.bytes();
    return L;
}
long long work_need(long long max_nodes, long long max_edges) {
    if (max_nodes <= PDG_LDS_N) return 0;
    // a graph beyond n + m <= TLC_PD_WIDE_MAX_ITEMS is not computed (TLC_ST_TOO_LARGE): the largest T = 2 n + 2 (n + m) among the others
    const long long n = max_nodes < TLC_PD_WIDE_MAX_ITEMS ? max_nodes : TLC_PD_WIDE_MAX_ITEMS;
    const long long m = max_edges < TLC_PD_WIDE_MAX_ITEMS - n ? max_edges : TLC_PD_WIDE_MAX_ITEMS - n;
    return (long long)wlayout(n, m).bytes;
}
unsigned pdg_grid(long long count) { return tlc_grid_for(count, PDG_BS, PDG_MAX_GRID); }

// The offsets of the batch on the host, and what they say about the classes.  large[]: the graphs of the third class that the device
// may compute (offsets in order, n + m within the limit); the device decides on the counts.
struct HostBatch {
    int64_t* offs = nullptr;       // node offsets [B + 1], then edge offsets [B + 1]
    int64_t* large = nullptr;
    long long n_large = 0, n_lds = 0, need = 0, need_graph = -1;
    ~HostBatch() { free(offs); free(large); }
};
int read_batch(const char* who, HostBatch& H, long long B, const int64_t* d_node_offs, const int64_t* d_edge_offs, hipStream_t st) {
    H.offs = (int64_t*)malloc((size_t)(B + 1) * 2 * sizeof(int64_t));
    H.large = (int64_t*)malloc((size_t)B * sizeof(int64_t));
    if (!H.offs || !H.large) { tlc_set_error("%s: out of host memory", who); return TLC_ERR_OUT_OF_MEMORY; }
    if (hipMemcpyAsync(H.offs, d_node_offs, (size_t)(B + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(H.offs + B + 1, d_edge_offs, (size_t)(B + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) {
        tlc_set_error("%s: reading the offsets failed: %s", who, hipGetErrorString(hipGetLastError()));
        return TLC_ERR_HIP;
    }
    const int64_t *no = H.offs, *eo = H.offs + B + 1;
    for (long long g = 0; g < B; ++g) {
        const long long n = no[g + 1] - no[g], m = eo[g + 1] - eo[g];
        if (no[g] < 0 || eo[g] < 0 || n < 0 || m < 0 || n <= PDG_WAVE_N) continue;
        if (n <= PDG_LDS_N) { H.n_lds += 1; continue; }
        if (n + m > TLC_PD_WIDE_MAX_ITEMS) continue;
        H.large[H.n_large++] = g;
        const long long b = (long long)wlayout(n, m).bytes;
        if (b > H.need) { H.need = b; H.need_graph = g; }
    }
    return TLC_OK;
}
int check_work(const char* who, const HostBatch& H, long long B, int64_t work_bytes) {
    if (work_bytes >= H.need) return TLC_OK;
    const long long g = H.need_graph;
    tlc_set_error("%s: d_work holds %lld bytes; graph %lld (%lld nodes, %lld edges) needs %lld (tlc_pd_grad_work_bytes)", who,
                  (long long)work_bytes, g, (long long)(H.offs[g + 1] - H.offs[g]), (long long)(H.offs[B + 1 + g + 1] - H.offs[B + 1 + g]),
                  H.need);
    return TLC_ERR_INVALID_ARG;
}
// what both entries refuse from their scalar arguments alone
int check_sizes(const char* who, int64_t n_graphs, const void* d_work, int64_t work_bytes) {
    if (n_graphs < 0 || n_graphs >= (1ll << 31) || work_bytes < 0) { tlc_set_error("%s: bad sizes", who); return TLC_ERR_INVALID_ARG; }
    if (n_graphs == 0) return TLC_OK;
    const long long least = work_need(PDG_LDS_N + 1, 0);
    if (work_bytes > 0 && (work_bytes < least || !d_work)) {
        if (!d_work) tlc_set_error("%s: null pointer", who);
        else tlc_set_error("%s: d_work holds %lld bytes; the smallest graph above TLC_PD_VERT_LDS_NMAX nodes needs %lld (a batch without "
                           "one needs none: tlc_pd_grad_work_bytes)", who, (long long)work_bytes, least);
        return TLC_ERR_INVALID_ARG;
    }
    return TLC_OK;
}

}  // namespace

extern "C" int tlc_pd_grad_work_bytes(int64_t max_nodes, int64_t max_edges, int64_t* bytes) {
    TLC_REQUIRE(bytes, "null pointer");
    TLC_REQUIRE(max_nodes >= 0 && max_edges >= 0, "negative size");
    *bytes = work_need(max_nodes, max_edges);
    return TLC_OK;
}

extern "C" int tlc_pd_point_vertices(int64_t n_graphs, const int64_t* d_node_offs, const int64_t* d_edge_offs, const double* d_f,
                                     const double* d_pd_up, const double* d_pd_down, const double* d_pd_one, const double* d_ext0,
                                     const int32_t* d_counts, int32_t* d_vert_up, int32_t* d_vert_down, int32_t* d_vert_one,
                                     int32_t* d_vert_ext0, uint8_t* d_status, void* d_work, int64_t work_bytes, void* stream) {
    int rc = check_sizes(__func__, n_graphs, d_work, work_bytes);
    if (rc != TLC_OK || n_graphs == 0) return rc;
    TLC_REQUIRE(d_node_offs && d_edge_offs && d_f && d_pd_up && d_pd_down && d_pd_one && d_ext0 && d_counts && d_vert_up && d_vert_down &&
                    d_vert_one && d_vert_ext0 && d_status, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    HostBatch H;
    if ((rc = read_batch(__func__, H, n_graphs, d_node_offs, d_edge_offs, st)) != TLC_OK) return rc;
    if ((rc = check_work(__func__, H, n_graphs, work_bytes)) != TLC_OK) return rc;
    const VertArgs A{n_graphs, d_node_offs, d_edge_offs, d_f, d_pd_up, d_pd_down, d_pd_one, d_ext0, d_counts,
                     d_vert_up, d_vert_down, d_vert_one, d_vert_ext0, d_status};
    hipLaunchKernelGGL(pdg_wave_vertices_kernel, dim3(pdg_grid(n_graphs * 64)), dim3(PDG_BS), 0, st, A);
    if (H.n_lds) hipLaunchKernelGGL(pdg_lds_vertices_kernel, dim3((unsigned)(n_graphs < PDG_MAX_GRID ? n_graphs : PDG_MAX_GRID)), dim3(PDG_BS), 0, st, A);
    char* w = H.n_large ? tlc_align256(d_work) : nullptr;
    for (long long i = 0; i < H.n_large; ++i) {
        const long long g = H.large[i], no = H.offs[g], eo = H.offs[n_graphs + 1 + g];
        const long long n = H.offs[g + 1] - no, m = H.offs[n_graphs + 1 + g + 1] - eo;
        const WLay L = wlayout(n, m);
        int* ctl = (int*)(w + L.ctl);
        unsigned long long *key_a = (unsigned long long*)(w + L.key_a), *key_b = (unsigned long long*)(w + L.key_b);
        unsigned *val_a = (unsigned*)(w + L.val_a), *val_b = (unsigned*)(w + L.val_b);
        hipLaunchKernelGGL(pdgw_ctl_kernel, dim3(1), dim3(64), 0, st, ctl, d_node_offs, d_edge_offs, d_counts, (const uint8_t*)nullptr, g);
        hipLaunchKernelGGL(pdgw_keys_kernel, dim3(pdg_grid(n)), dim3(PDG_BS), 0, st, ctl, n, d_f + no, key_a, val_a);
        rk_sort<64>(st, n, key_a, key_b, val_a, val_b, (int*)(w + L.hist), (int*)(w + L.tot));
        hipLaunchKernelGGL(pdgw_search_kernel, dim3(pdg_grid(4 * n + 2 * m + 2)), dim3(PDG_BS), 0, st, ctl, n, m, key_a, val_a, d_pd_up + 2 * no,
                           d_pd_down + 2 * no, d_pd_one + 2 * eo, d_ext0 + 2 * g, d_vert_up + 2 * no, d_vert_down + 2 * no,
                           d_vert_one + 2 * eo, d_vert_ext0 + 2 * g);
        hipLaunchKernelGGL(pdgw_status_kernel, dim3(1), dim3(64), 0, st, ctl, d_status + g);
    }
    TLC_HIP_CHECK(hipGetLastError());
    return TLC_OK;
}

extern "C" int tlc_pd_filtration_grad(int64_t n_graphs, const int64_t* d_node_offs, const int64_t* d_edge_offs, const int32_t* d_counts,
                                      const int32_t* d_vert_up, const int32_t* d_vert_down, const int32_t* d_vert_one,
                                      const int32_t* d_vert_ext0, const double* d_g_up, const double* d_g_down, const double* d_g_one,
                                      const double* d_g_ext0, const uint8_t* d_status, double* d_grad_f, void* d_work, int64_t work_bytes,
                                      void* stream) {
    int rc = check_sizes(__func__, n_graphs, d_work, work_bytes);
    if (rc != TLC_OK || n_graphs == 0) return rc;
    TLC_REQUIRE(d_node_offs && d_edge_offs && d_counts && d_vert_up && d_vert_down && d_vert_one && d_vert_ext0 && d_status && d_grad_f,
                "null pointer");
    hipStream_t st = (hipStream_t)stream;
    HostBatch H;
    if ((rc = read_batch(__func__, H, n_graphs, d_node_offs, d_edge_offs, st)) != TLC_OK) return rc;
    if ((rc = check_work(__func__, H, n_graphs, work_bytes)) != TLC_OK) return rc;
    const GradArgs A{n_graphs, d_node_offs, d_edge_offs, d_counts, d_vert_up, d_vert_down, d_vert_one, d_vert_ext0,
                     d_g_up, d_g_down, d_g_one, d_g_ext0, d_status, d_grad_f};
    hipLaunchKernelGGL(pdg_wave_grad_kernel, dim3(pdg_grid(n_graphs * 64)), dim3(PDG_BS), 0, st, A);
    if (H.n_lds) hipLaunchKernelGGL(pdg_lds_grad_kernel, dim3((unsigned)(n_graphs < PDG_MAX_GRID ? n_graphs : PDG_MAX_GRID)), dim3(PDG_BS), 0, st, A);
    char* w = H.n_large ? tlc_align256(d_work) : nullptr;
    for (long long i = 0; i < H.n_large; ++i) {
        const long long g = H.large[i], no = H.offs[g], eo = H.offs[n_graphs + 1 + g];
        const long long n = H.offs[g + 1] - no, m = H.offs[n_graphs + 1 + g + 1] - eo, T = 4 * n + 2 * m + 2;
        const WLay L = wlayout(n, m);
        int* ctl = (int*)(w + L.ctl);
        unsigned *key_a = (unsigned*)(w + L.key_a), *key_b = (unsigned*)(w + L.key_b);
        unsigned *val_a = (unsigned*)(w + L.val_a), *val_b = (unsigned*)(w + L.val_b);
        hipLaunchKernelGGL(pdgw_ctl_kernel, dim3(1), dim3(64), 0, st, ctl, d_node_offs, d_edge_offs, d_counts, d_status, g);
        hipLaunchKernelGGL(pdgw_items_kernel, dim3(pdg_grid(T)), dim3(PDG_BS), 0, st, ctl, n, m, d_vert_up + 2 * no, d_vert_down + 2 * no,
                           d_vert_one + 2 * eo, d_vert_ext0 + 2 * g, key_a, val_a);
        rk_sort<32>(st, T, key_a, key_b, val_a, val_b, (int*)(w + L.hist), (int*)(w + L.tot));
        hipLaunchKernelGGL(pdgw_sum_kernel, dim3(pdg_grid(n)), dim3(PDG_BS), 0, st, ctl, n, m, key_a, val_a, d_g_up ? d_g_up + 2 * no : nullptr,
                           d_g_down ? d_g_down + 2 * no : nullptr, d_g_one ? d_g_one + 2 * eo : nullptr,
                           d_g_ext0 ? d_g_ext0 + 2 * g : nullptr, d_grad_f + no);
    }
    TLC_HIP_CHECK(hipGetLastError());
    return TLC_OK;
}

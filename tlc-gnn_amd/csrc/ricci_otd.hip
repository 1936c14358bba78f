// ricci_otd.hip -- Ollivier-Ricci curvature with the EXACT transport distance: GraphRicciCurvature's OllivierRicci(G, alpha,
// method="OTD") (POT's emd2), which the reference's node-classification pipeline uses for its curvature files (pipelines_GIN.py:79).
//
// The optimum is a number, not an algorithm, and on this path (unit weights, alpha = p / q) it is an integer: for an edge (s, t)
// scale the two measures by D = q * deg(s) * deg(t):
//     source: p * deg(s) * deg(t) at s, (q - p) * deg(t) on each neighbour of s;   sink: the same with s and t exchanged;
// the cost of a pair is its hop distance, 0..3 (the 2-bit codes ricci.hip stages, ricci_codes.h).  W = the integer minimum cost,
// kappa = 1.0 - (double)W / (double)D: one fp64 division and one subtraction, nothing floating before them.
//
// Mass on a node of both supports (s, t, the common neighbours) is cancelled in place first -- the cost is a metric, so some
// optimum leaves it where it is -- and the rest is solved by the primal-dual method of ricci_otd_solve.h.
//
// Tiers, as for Sinkhorn: one wavefront per edge with everything in LDS (u16 flow cells: D <= 65 535, which at alpha = 1/2 is every
// edge with na * nb <= 8 192), else one 1 024-thread workgroup per edge with the per-node state in LDS, the codes in LDS when they
// fit and the flow cells (u32, or u64 when q * (max_support / 2)^2 could pass 2^32) in the block's workspace slot.
#include "tlc_common.h"
#include "ricci_codes.h"
#include "ricci_otd_solve.h"

namespace {

struct OtdParams {
    int n_nodes;
    const int* rowptr;
    const int* col;
    long long n_edges;
    const int* edges;            // [n_edges, 2]
    int num, den;                // alpha = num / den
    double* kappa;               // [n_edges]
    long long* cost;             // [n_edges] or null: W
    long long* denom;            // [n_edges] or null: D
    int* big_count;              // device counter + list of the edges left to the workgroup kernel
    int* big_list;
    unsigned char* slots;        // [n_slots][slot_bytes]: codes (code_bytes), then the flow cells
    long long slot_bytes, code_bytes, max_product;
    int max_support;
};

template <int W>
struct OtdSync { __device__ __forceinline__ void operator()() const { group_sync<W>(); } };
struct OtdAtomicMin { __device__ __forceinline__ void operator()(int* p, int v) const { atomicMin(p, v); } };

__device__ __forceinline__ void otd_write(const OtdParams& p, long long e, long long w, long long d) {
    p.kappa[e] = w < 0 ? __longlong_as_double(0x7ff8000000000000LL) : (d > 0 ? 1.0 - (double)w / (double)d : 0.0);
    if (p.cost) p.cost[e] = w < 0 ? -1 : w;
    if (p.denom) p.denom[e] = d;
}

// One edge by one group of W threads.  ex: na + nb entries of Ex, and room for the na + nb + 1 ints of the staging (which it
// overlays: the ids are dead once the twins are known); par / st / pot: na + nb entries each; sh: otd::SH_INTS ints.
template <int W, class Cell, class Ex>
__device__ void otd_edge(const OtdParams& p, long long e, unsigned int* codes, Cell* x, Ex* ex, unsigned short* par, unsigned char* st,
                         signed char* pot, int* sh, int tid) {
    const int s = p.edges[2 * e], t = p.edges[2 * e + 1];
    const int sl = p.rowptr[s], tl = p.rowptr[t];
    const int ds = p.rowptr[s + 1] - sl, dt = p.rowptr[t + 1] - tl;
    const int na = ds + 1, nb = dt + 1;
    int* const idx = reinterpret_cast<int*>(ex);
    ricci_stage_codes<W>(p.rowptr, p.col, s, t, codes, idx, tid);
    // the twin of source i: the index of the same node in the sink support (idx[0 .. dt) = the neighbours of t, ascending)
    for (int i = tid; i < na; i += W) {
        const int z = i < ds ? p.col[sl + i] : s;
        int tw = otd::ROOT;
        if (z == t) tw = dt;
        else {
            int lo = 0, hi = dt;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                const int c = idx[mid];
                if (c == z) { tw = mid; break; }
                if (c < z) lo = mid + 1; else hi = mid;
            }
        }
        par[i] = (unsigned short)tw;
    }
    group_sync<W>();
    const Ex own = (Ex)((long long)p.num * ds * dt);
    const Ex ma = (Ex)((long long)(p.den - p.num) * dt), mb = (Ex)((long long)(p.den - p.num) * ds);
    Ex* const exA = ex;
    Ex* const exB = ex + na;
    for (int i = tid; i < na; i += W) exA[i] = i < ds ? ma : own;
    for (int j = tid; j < nb; j += W) exB[j] = j < dt ? mb : own;
    group_sync<W>();
    for (int i = tid; i < na; i += W) {                   // a sink has one twin at most: no two threads meet
        const int tw = par[i];
        if (tw != otd::ROOT) {
            const Ex a = exA[i], b = exB[tw], c = a < b ? a : b;
            exA[i] = a - c;
            exB[tw] = b - c;
        }
    }
    group_sync<W>();
    const long long w = otd::solve<W, Cell, Ex>(codes, na, nb, x, exA, exB, par, par + na, st, st + na, pot, pot + na, sh, tid, OtdSync<W>(),
                                                OtdAtomicMin());
    if (tid == 0) otd_write(p, e, w, (long long)p.den * ds * dt);
    group_sync<W>();
}

#define OTD_SMALL_CELLS 8192            /* TLC_OTD_WAVE_PRODUCT: flow cells (u16) and hop codes per wavefront: 16 KB + 2 KB */
#define OTD_SMALL_SUPPORT 256           /* TLC_OTD_WAVE_SUPPORT: na + nb limit of the wavefront kernel */
#define OTD_SMALL_DENOM 65535           /* TLC_OTD_WAVE_DENOM: D limit of the u16 cells */
#define OTD_SMALL_WAVES 2

// one wavefront per edge, two per workgroup (20.5 KB of LDS each), everything in LDS; the rest goes to the workgroup kernel's list
__global__ __launch_bounds__(64 * OTD_SMALL_WAVES) void otd_small_kernel(OtdParams p) {
    __shared__ __attribute__((aligned(16))) unsigned int s_codes[OTD_SMALL_WAVES][OTD_SMALL_CELLS / 16];
    __shared__ __attribute__((aligned(16))) unsigned short s_x[OTD_SMALL_WAVES][OTD_SMALL_CELLS];
    __shared__ __attribute__((aligned(16))) int s_ex[OTD_SMALL_WAVES][OTD_SMALL_SUPPORT + 4];
    __shared__ unsigned short s_par[OTD_SMALL_WAVES][OTD_SMALL_SUPPORT];
    __shared__ unsigned char s_st[OTD_SMALL_WAVES][OTD_SMALL_SUPPORT];
    __shared__ signed char s_pot[OTD_SMALL_WAVES][OTD_SMALL_SUPPORT];
    __shared__ int s_sh[OTD_SMALL_WAVES][otd::SH_INTS];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long n_waves = (long long)gridDim.x * OTD_SMALL_WAVES;
    for (long long e = (long long)blockIdx.x * OTD_SMALL_WAVES + wv; e < p.n_edges; e += n_waves) {
        const int s = p.edges[2 * e], t = p.edges[2 * e + 1];
        const bool bad = s < 0 || t < 0 || s >= p.n_nodes || t >= p.n_nodes || s == t;
        if (bad) {
            if (lane == 0) otd_write(p, e, 0, 0);                    // self pair: curvature 0 (the library's convention), W 0, D 0
            continue;
        }
        const int ds = p.rowptr[s + 1] - p.rowptr[s], dt = p.rowptr[t + 1] - p.rowptr[t];
        const long long na = ds + 1, nb = dt + 1;
        if (na * nb > OTD_SMALL_CELLS || na + nb > OTD_SMALL_SUPPORT || (long long)p.den * ds * dt > OTD_SMALL_DENOM) {
            if (lane == 0) p.big_list[atomicAdd(p.big_count, 1)] = (int)e;
            continue;
        }
        otd_edge<64, unsigned short, int>(p, e, s_codes[wv], s_x[wv], s_ex[wv], s_par[wv], s_st[wv], s_pot[wv], s_sh[wv], lane);
    }
}

// hub edges: one workgroup per edge; ex / par / st / pot (12 bytes per support entry) and, when they fit (lds_codes bytes), the
// codes in LDS; the flow cells in the block's slot, which a few hub edges keep L2-resident
#define OTD_BIG_THREADS 1024
template <class Cell>
__global__ __launch_bounds__(OTD_BIG_THREADS) void otd_big_kernel(OtdParams p, int lds_codes) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_big[];
    const size_t ms = (size_t)p.max_support;
    long long* const ex = reinterpret_cast<long long*>(s_big);                               // [max_support] (>= the staging's ints)
    unsigned short* const par = reinterpret_cast<unsigned short*>(s_big + ms * 8);
    unsigned char* const st = s_big + ms * 10;
    signed char* const pot = reinterpret_cast<signed char*>(s_big + ms * 11);
    int* const sh = reinterpret_cast<int*>(s_big + ((ms * 12 + 15) & ~(size_t)15));
    unsigned int* const lds_code_base = reinterpret_cast<unsigned int*>(sh + otd::SH_INTS);
    unsigned char* const slot = p.slots + (size_t)blockIdx.x * (size_t)p.slot_bytes;
    const int n_big = *p.big_count;
    for (int k = blockIdx.x; k < n_big; k += gridDim.x) {
        const long long e = p.big_list[k];
        const int s = p.edges[2 * e], t = p.edges[2 * e + 1];
        const int ds = p.rowptr[s + 1] - p.rowptr[s], dt = p.rowptr[t + 1] - p.rowptr[t];
        const long long na = ds + 1, nb = dt + 1;
        const long long d = (long long)p.den * ds * dt;
        // beyond the caller's workspace, or a mass beyond the cell: loud
        if (na + nb > p.max_support || na * nb > p.max_product || (sizeof(Cell) == 4 && d > 0xffffffffLL)) {
            if (threadIdx.x == 0) otd_write(p, e, -1, d);
            continue;
        }
        const bool in_lds = na * nb <= (long long)lds_codes * 4;                               // four codes per byte
        otd_edge<OTD_BIG_THREADS, Cell, long long>(p, e, in_lds ? lds_code_base : reinterpret_cast<unsigned int*>(slot),
                                                   reinterpret_cast<Cell*>(slot + p.code_bytes), ex, par, st, pot, sh, threadIdx.x);
    }
}

constexpr int64_t OTD_LDS_BUDGET = 150 * 1024;

struct OtdLayout { int64_t list_bytes, code_bytes, cell_size, slot_bytes; };

// u32 cells hold every mass while alpha_den * deg(s) * deg(t) <= 1024 * (max_support / 2)^2 < 2^32
int otd_layout(int64_t n_edges, int32_t max_support, int64_t max_product, OtdLayout* L) {
    TLC_REQUIRE(n_edges >= 0 && n_edges < (1ll << 31), "n_edges: 0 .. 2^31 - 1");
    TLC_REQUIRE(max_support >= 2 && (int64_t)max_support * 12 + 64 <= OTD_LDS_BUDGET, "max_support beyond the LDS of a workgroup (12 800 entries)");
    TLC_REQUIRE(max_product >= 1 && max_product < (1ll << 31), "max_product: 1 .. 2^31 - 1");
    const int64_t half = (int64_t)max_support / 2 + 1;
    L->list_bytes = (n_edges * 4 + 15) & ~15ll;
    L->code_bytes = (((max_product + 3) / 4) + 15) & ~15ll;                 // 2 bits per hop code
    L->cell_size = 1024 * half * half < (1ll << 32) ? 4 : 8;
    L->slot_bytes = L->code_bytes + ((max_product * L->cell_size + 15) & ~15ll);
    return TLC_OK;
}

}  // namespace

extern "C" int tlc_ollivier_ricci_otd_work_bytes(int64_t n_edges, int32_t max_support, int64_t max_product, int64_t* bytes) {
    TLC_REQUIRE(bytes, "null pointer");
    OtdLayout L;
    const int rc = otd_layout(n_edges, max_support, max_product, &L);
    if (rc != TLC_OK) return rc;
    const int64_t slots = n_edges < 1 ? 1 : (n_edges < 32 ? n_edges : 32);
    *bytes = 16 + L.list_bytes + slots * L.slot_bytes;
    return TLC_OK;
}

extern "C" int tlc_ollivier_ricci_otd(int32_t n_nodes, const int32_t* d_rowptr, const int32_t* d_col, int64_t n_edges, const int32_t* d_edges,
                                      int32_t alpha_num, int32_t alpha_den, double* d_kappa, int64_t* d_cost, int64_t* d_denom, void* d_work,
                                      int64_t work_bytes, int32_t max_support, int64_t max_product, void* stream) {
    TLC_REQUIRE(n_nodes >= 0 && n_edges >= 0, "negative size");
    TLC_REQUIRE(alpha_den >= 1 && alpha_den <= 1024, "alpha_den: 1 .. 1024");
    TLC_REQUIRE(alpha_num >= 0 && alpha_num <= alpha_den, "alpha_num: 0 .. alpha_den");
    if (n_edges == 0) return TLC_OK;
    TLC_REQUIRE(d_rowptr && d_col && d_edges && d_kappa, "null pointer");
    OtdLayout L;
    const int rc = otd_layout(n_edges, max_support, max_product, &L);
    if (rc != TLC_OK) return rc;
    // workspace: [counter 16 B][big list int32[n_edges]][slots x (codes, flow cells)]
    TLC_REQUIRE(d_work && work_bytes >= 16 + L.list_bytes + L.slot_bytes, "workspace too small: see tlc_ollivier_ricci_otd_work_bytes()");
    TLC_REQUIRE((reinterpret_cast<uintptr_t>(d_work) & 15) == 0, "d_work must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    OtdParams p;
    p.n_nodes = n_nodes; p.rowptr = d_rowptr; p.col = d_col; p.n_edges = n_edges; p.edges = d_edges;
    p.num = alpha_num; p.den = alpha_den; p.kappa = d_kappa; p.cost = (long long*)d_cost; p.denom = (long long*)d_denom;
    p.big_count = (int*)d_work;
    p.big_list = (int*)((char*)d_work + 16);
    p.slots = (unsigned char*)d_work + 16 + L.list_bytes;
    p.slot_bytes = L.slot_bytes; p.code_bytes = L.code_bytes; p.max_product = max_product;
    p.max_support = max_support;
    int64_t slots = (work_bytes - 16 - L.list_bytes) / L.slot_bytes;
    if (slots > 1024) slots = 1024;
    if (slots > n_edges) slots = n_edges;
    TLC_HIP_CHECK(hipMemsetAsync(d_work, 0, 16, s));
    long long blocks = (n_edges + OTD_SMALL_WAVES - 1) / OTD_SMALL_WAVES;
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(otd_small_kernel, dim3((unsigned)blocks), dim3(64 * OTD_SMALL_WAVES), 0, s, p);
    // LDS of the workgroup kernel: 12 bytes per support entry, the control block, and as many code bytes as the largest product needs
    const int64_t state_bytes = (((int64_t)max_support * 12 + 15) & ~15ll) + otd::SH_INTS * 4;
    int64_t lds_codes = OTD_LDS_BUDGET - state_bytes;
    if (lds_codes > L.code_bytes) lds_codes = L.code_bytes;
    if (lds_codes < 0) lds_codes = 0;
    const size_t lds = (size_t)(state_bytes + lds_codes);
    if (L.cell_size == 4) {
        if (lds > 64 * 1024) TLC_HIP_CHECK(hipFuncSetAttribute((const void*)otd_big_kernel<unsigned int>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(otd_big_kernel<unsigned int>, dim3((unsigned)slots), dim3(OTD_BIG_THREADS), lds, s, p, (int)lds_codes);
    } else {
        if (lds > 64 * 1024) TLC_HIP_CHECK(hipFuncSetAttribute((const void*)otd_big_kernel<unsigned long long>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(otd_big_kernel<unsigned long long>, dim3((unsigned)slots), dim3(OTD_BIG_THREADS), lds, s, p, (int)lds_codes);
    }
    TLC_HIP_CHECK(hipGetLastError());
    return TLC_OK;
}

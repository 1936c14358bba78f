// gc_prep.hip -- tlc_graph_components: the connected components of a packed batch of RAW edge lists (both orientations, repeats and self
// loops allowed and dropped), the largest component of every graph extracted, renumbered and deduplicated -- the per-graph host step of
// the reference's graph-classification ground truth (Knowledge_Distillation/data_utils_GC.py:240-248), whose restatement in this project
// is `data_utils_GC.largest_component` (numpy unique + scipy connected_components); that function is the specification, integer for integer.
// The contract is the comment of include/tlcgnn.h; the algorithm of both classes is DESIGN.md 6.9.
//
// Everything is an integer.  The only atomics are integer (LDS atomicOr; global atomicMin on labels, atomicAdd on counts, atomicMax on the
// packed winner, one atomicAdd per wavefront on an append cursor whose order the sort removes), and every one of them is commutative with a
// unique end state, so the outputs do not depend on the scheduling, on the batch around a graph or on the number of rounds run.
//
// Classes by node count, binned ON THE DEVICE from node_ptr:
//   WAVE  n <= 64   one wavefront per graph, four per workgroup, a persistent loop that draws graphs from the list by a ticket.  Lane v
//                   owns row v of the adjacency matrix as one u64 in LDS; the component masks are closed in REGISTERS by one Warshall
//                   sweep: for pivot k = 0 .. n-1 every lane whose mask holds k ORs in lane k's mask (two readlanes of a uniform k).  One
//                   sweep is the whole transitive closure, its trip count n is uniform, and there is no per-lane `while` whose longest
//                   lane the wavefront waits for (README, round 6); the only per-lane loop writes a lane's own upper neighbours, at most
//                   its degree (three or four on molecules).
//   WIDE  larger    all such graphs TOGETHER, one item after the other over the whole device: keys (lo, hi) in global ids from a
//                   wavefront-aggregated append, two stable radix sorts (by hi, then by lo: `rk_sort` of radix_passes.h on u32 halves, 16
//                   or 32 bits by total_nodes), FastSV labelling rounds (hook the parents and the ends onto the lower grandparent with
//                   atomicMin, then jump), component sizes, the per-graph winner, two exclusive scans, the outputs.
#include "tlc_common.h"

#include <algorithm>

#include "radix_passes.h"
#include "scratch_layouts.h"

#define CC_WAVE_N TLC_CC_WAVE_NMAX
#define CC_BS 256
#define CC_SCAN_IPT 8
#define CC_ROUND_GROUP 4            // labelling rounds per read-back of the "changed" word
#define CC_FLAG_SLOTS 32            // "changed" words in the head: one per round, zeroed again when the rounds wrap
#define CC_JUMPS 4                  // pointer jumps of a node per round (it stops at a root)

static_assert(CC_WAVE_N == 64, "a u64 adjacency row per lane");
static_assert(CC_BS * CC_SCAN_IPT == TlcGraphComponentsScratch::SCAN_CHUNK, "scan chunk");
static_assert(CC_FLAG_SLOTS % CC_ROUND_GROUP == 0, "a group of rounds does not straddle the wrap");

namespace {

typedef unsigned long long u64;
typedef unsigned int u32;

// the head's ints: the WAVE list's length and ticket, the WIDE class's graphs and keys (read back together), the rounds' "changed" words
enum { H_WAVE_COUNT = 0, H_WAVE_TICKET = 1, H_WIDE_GRAPHS = 2, H_WIDE_ITEMS = 3, H_FLAGS = 8 };
static_assert((H_FLAGS + CC_FLAG_SLOTS) * 4 <= TlcGraphComponentsScratch::HEAD, "head");
enum { CLS_NONE = 0, CLS_WIDE = 2 };

__device__ __forceinline__ void cc_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// ---- binning: one thread per graph ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CC_BS) void cc_bin_kernel(long long B, long long total_nodes, long long total_edges, long long max_nodes,
                                                       const long long* __restrict__ node_ptr, const long long* __restrict__ edge_ptr,
                                                       int* __restrict__ head, int* __restrict__ list, unsigned char* __restrict__ cls,
                                                       u64* __restrict__ best, int* __restrict__ comps, int* __restrict__ info,
                                                       unsigned char* __restrict__ status) {
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    bool wave = false, wide = false;
    if (g < B) {
        const long long n0 = node_ptr[g], n1 = node_ptr[g + 1], e0 = edge_ptr[g], e1 = edge_ptr[g + 1];
        const long long n = n1 - n0, m = e1 - e0;
        bool ok = !(n0 < 0 || n1 < n0 || n1 > total_nodes || e0 < 0 || e1 < e0 || e1 > total_edges);
        ok = ok && !(max_nodes >= 0 && n > max_nodes) && !(n == 0 && m > 0);      // an edge of a graph without nodes names an id outside it
        status[g] = ok ? TLC_ST_OK : TLC_ST_BAD_INPUT;
        if (ok && n == 0) reinterpret_cast<int4*>(info)[g] = make_int4(0, 0, 0, 0);
        wave = ok && n > 0 && n <= CC_WAVE_N;
        wide = ok && n > CC_WAVE_N;
        if (cls) cls[g] = wide ? CLS_WIDE : CLS_NONE;     // cls == nullptr: the workspace has no WIDE part, and no graph can be WIDE
        if (wide) { best[g] = 0; comps[g] = 0; }
    }
    // one atomic per wavefront and class
    const u64 mw = __ballot(wave), md = __ballot(wide);
    if (mw) {
        const int leader = __ffsll((long long)mw) - 1;
        int base = 0;
        if (tlc_lane() == leader) base = atomicAdd(&head[H_WAVE_COUNT], __popcll(mw));
        base = __shfl(base, leader);
        if (wave) list[base + __popcll(mw & tlc_lanemask_lt())] = (int)g;
    }
    if (md && tlc_lane() == __ffsll((long long)md) - 1) atomicAdd(&head[H_WIDE_GRAPHS], __popcll(md));
}

// ---- WAVE: n <= 64 ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ u64 cc_readlane_u64(u64 v, int l) {
    return ((u64)(u32)__builtin_amdgcn_readlane((int)(v >> 32), l) << 32) | (u64)(u32)__builtin_amdgcn_readlane((int)(u32)v, l);
}
__device__ __forceinline__ u32 cc_wave_max_u32(u32 v) {
    v = max(v, tlc_lane_xor_u32<1>(v));
    v = max(v, tlc_lane_xor_u32<2>(v));
    v = max(v, tlc_lane_xor_u32<4>(v));
    v = max(v, tlc_lane_xor_u32<8>(v));
    v = max(v, tlc_lane_xor_u32<16>(v));
    v = max(v, tlc_lane_xor_u32<32>(v));
    return v;
}

__device__ __forceinline__ int cc_wave_graph(u64* row, int* flag, int lane, int n, int m, const int2* __restrict__ edges, int4* __restrict__ info,
                                             int* __restrict__ new_id, int2* __restrict__ out_edges) {
    row[lane] = 0;
    if (lane == 0) flag[0] = 0;
    cc_wave_sync();
    for (int e = lane; e < m; e += 64) {
        const int2 ab = edges[e];
        if ((unsigned)ab.x >= (unsigned)n || (unsigned)ab.y >= (unsigned)n) flag[0] = 1;
        else if (ab.x != ab.y) {
            atomicOr(&row[ab.x], 1ull << ab.y);
            atomicOr(&row[ab.y], 1ull << ab.x);
        }
    }
    cc_wave_sync();
    if (flag[0]) return TLC_ST_BAD_INPUT;
    const u64 mine = row[lane];                                  // lanes n .. 63: 0, no id in range names them
    const u64 above = ~((2ull << lane) - 1ull);                  // the bits above the lane's own (lane 63: none)
    // one Warshall sweep: after pivot k a mask holds everything it reaches through pivots 0 .. k
    u64 comp = lane < n ? (mine | (1ull << lane)) : 0ull;
    for (int k = 0; k < n; ++k) {
        const u64 rk = cc_readlane_u64(comp, k);
        if ((comp >> k) & 1ull) comp |= rk;
    }
    const int label = __ffsll((long long)comp) - 1;              // the component's lowest id (-1 on the lanes behind n)
    // the winner: most nodes, then the lower label -- every lane of a component holds the same key
    const u32 key = lane < n ? ((u32)__popcll(comp) << 6) | (u32)(63 - label) : 0u;
    const int wl = 63 - (int)(__builtin_amdgcn_readfirstlane((int)cc_wave_max_u32(key)) & 63);
    const u64 W = cc_readlane_u64(comp, wl);
    const bool in = (W >> lane) & 1ull;
    const int nid = __popcll(W & tlc_lanemask_lt());
    if (lane < n) new_id[lane] = in ? nid : -1;
    // the edges in (lo, hi) order: lane lo writes its neighbours above it, ascending, behind those of the lanes below
    const u64 upper = mine & above;
    const int cnt = in ? __popcll(upper) : 0;
    const int incl = tlc_wave_iscan_i32(cnt);
    int off = incl - cnt;
    if (in)
        for (u64 r = upper; r; r &= r - 1) {
            const int hi = __ffsll((long long)r) - 1;
            out_edges[off++] = make_int2(nid, __popcll(W & ((1ull << hi) - 1ull)));
        }
    const int c = __popcll(__ballot(lane < n && label == lane));
    const int s = tlc_wave_sum_i32(__popcll(upper));
    if (lane == 0) info[0] = make_int4(__popcll(W), __builtin_amdgcn_readlane(incl, 63), c, s);
    return TLC_ST_OK;
}

__global__ __launch_bounds__(CC_BS) void cc_wave_kernel(const long long* __restrict__ node_ptr, const long long* __restrict__ edge_ptr,
                                                        const int* __restrict__ edges, int* __restrict__ info, int* __restrict__ new_id,
                                                        int* __restrict__ out_edges, unsigned char* __restrict__ status, int* __restrict__ head,
                                                        const int* __restrict__ list) {
    __shared__ u64 rows[CC_BS / 64][64];
    __shared__ int flags_s[CC_BS / 64][2];
    const int lane = tlc_lane(), wv = (int)(threadIdx.x >> 6);
    const int count = head[H_WAVE_COUNT];
    for (;;) {
        int i = lane == 0 ? atomicAdd(&head[H_WAVE_TICKET], 1) : 0;
        i = __builtin_amdgcn_readfirstlane(i);
        if (i >= count) break;
        const int g = __builtin_amdgcn_readfirstlane(list[i]);
        const long long n0 = node_ptr[g], e0 = edge_ptr[g];
        const int n = __builtin_amdgcn_readfirstlane((int)(node_ptr[g + 1] - n0)), m = __builtin_amdgcn_readfirstlane((int)(edge_ptr[g + 1] - e0));
        const int st = cc_wave_graph(rows[wv], flags_s[wv], lane, n, m, reinterpret_cast<const int2*>(edges) + e0, reinterpret_cast<int4*>(info) + g,
                                     new_id + n0, reinterpret_cast<int2*>(out_edges) + e0);
        if (lane == 0 && st != TLC_ST_OK) status[g] = (unsigned char)st;
        cc_wave_sync();
    }
}

// ---- WIDE: every larger graph, together ---------------------------------------------------------------------------------------------
struct CcWide {
    long long B, N, M;                       // graphs, nodes and raw edges of the whole batch
    const long long *node_ptr, *edge_ptr;
    const int* edges;
    int* head;
    unsigned char* cls;
    u64* best;                               // per graph: size << 32 | ~label (local) of the winner so far
    int *comps, *first;                      // per graph: components; index of its first sorted key
    u32* parent;                             // per node (global id): the label tree
    int* size;                               // per node: nodes labelled by it
    u64* nscan;                              // keep flags, then their exclusive scan, [N + 1]
    u32 *klo, *khi;                          // the sorted keys' halves
    u64* escan;                              // distinct | kept << 32 per key, then the exclusive scan, [items + 1]
    int *info, *new_id, *out_edges;
    unsigned char* status;
};

// the largest g in [0, B) with ptr[g] <= x (ptr ascending: the graph whose slice holds x; the callers check that it does)
__device__ __forceinline__ long long cc_owner(const long long* __restrict__ ptr, long long B, long long x) {
    long long lo = 0, hi = B;
    while (hi - lo > 1) {
        const long long mid = (lo + hi) >> 1;
        if (ptr[mid] <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}
// the WIDE graph that holds node x, or -1 (another class, a refused graph, or offsets out of order around x)
__device__ __forceinline__ long long cc_wide_graph(const CcWide& P, long long x) {
    const long long g = cc_owner(P.node_ptr, P.B, x);
    return (P.cls[g] == CLS_WIDE && x >= P.node_ptr[g] && x < P.node_ptr[g + 1]) ? g : -1;
}
__device__ __forceinline__ long long cc_tid() { return (long long)blockIdx.x * blockDim.x + threadIdx.x; }
__device__ __forceinline__ u32 cc_load(const u32* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// raw edge i of a WIDE graph -> the key (global lo, global hi), appended; an id out of range refuses the graph before it indexes anything
__global__ __launch_bounds__(CC_BS) void cc_keys_kernel(CcWide P) {
    const long long i = cc_tid();
    bool emit = false;
    u32 lo = 0, hi = 0;
    if (i < P.M) {
        const long long g = cc_owner(P.edge_ptr, P.B, i);
        if (P.cls[g] == CLS_WIDE && i >= P.edge_ptr[g] && i < P.edge_ptr[g + 1]) {
            const long long n0 = P.node_ptr[g], n = P.node_ptr[g + 1] - n0;
            const int a = P.edges[2 * i], b = P.edges[2 * i + 1];
            if ((unsigned)a >= (u64)n || (unsigned)b >= (u64)n) P.status[g] = TLC_ST_BAD_INPUT;
            else if (a != b) {
                emit = true;
                lo = (u32)(n0 + std::min(a, b));
                hi = (u32)(n0 + std::max(a, b));
            }
        }
    }
    const u64 mask = __ballot(emit);
    if (!mask) return;
    const int leader = __ffsll((long long)mask) - 1;
    int base = 0;
    if (tlc_lane() == leader) base = atomicAdd(&P.head[H_WIDE_ITEMS], __popcll(mask));
    base = __shfl(base, leader);
    if (emit) {
        const int pos = base + __popcll(mask & tlc_lanemask_lt());
        P.klo[pos] = lo;
        P.khi[pos] = hi;
    }
}

__global__ __launch_bounds__(CC_BS) void cc_init_kernel(CcWide P) {
    const long long v = cc_tid();
    if (v < P.N) { P.parent[v] = (u32)v; P.size[v] = 0; }
}

// one labelling round.  Invariant: parent[x] <= x and in x's component; every write lowers a parent to such a node, so the rounds end, and
// they end only where every parent is a root and the two ends of every key share it: the component's lowest id, whatever the order was.
__global__ __launch_bounds__(CC_BS) void cc_round_kernel(CcWide P, long long items, const int* __restrict__ prev, int* __restrict__ cur) {
    if (prev && *prev == 0) return;              // the round before changed nothing: neither does this one
    const long long i = cc_tid();
    bool changed = false;
    if (i < items) {
        const u32 u = P.klo[i], v = P.khi[i];
        const u32 fu = cc_load(&P.parent[u]), fv = cc_load(&P.parent[v]);
        if (fu != fv) {
            const u32 gu = cc_load(&P.parent[fu]), gv = cc_load(&P.parent[fv]);
            const u32 lo = std::min(gu, gv);
            if (gu > lo) changed |= atomicMin(&P.parent[fu], lo) > lo;     // the parents onto the lower grandparent
            if (gv > lo) changed |= atomicMin(&P.parent[fv], lo) > lo;
            if (fu > lo) changed |= atomicMin(&P.parent[u], lo) > lo;      // and the ends themselves
            if (fv > lo) changed |= atomicMin(&P.parent[v], lo) > lo;
        }
    }
    if (i < P.N) {
        const u32 p0 = cc_load(&P.parent[i]);
        u32 p = p0;
        for (int j = 0; j < CC_JUMPS; ++j) {
            const u32 q = cc_load(&P.parent[p]);
            if (q == p) break;
            p = q;
        }
        if (p < p0) changed |= atomicMin(&P.parent[i], p) > p;
    }
    if (__ballot(changed) && tlc_lane() == 0) atomicOr(cur, 1);
}

__global__ __launch_bounds__(CC_BS) void cc_count_kernel(CcWide P) {
    const long long v = cc_tid();
    if (v < P.N) atomicAdd(&P.size[P.parent[v]], 1);
}

// every root of a computed WIDE graph: one more component, and a candidate for the winner (most nodes, then the lower label)
__global__ __launch_bounds__(CC_BS) void cc_winner_kernel(CcWide P) {
    const long long v = cc_tid();
    if (v >= P.N || P.parent[v] != (u32)v) return;
    const long long g = cc_wide_graph(P, v);
    if (g < 0 || P.status[g] != TLC_ST_OK) return;
    atomicAdd(&P.comps[g], 1);
    atomicMax(&P.best[g], ((u64)(u32)P.size[v] << 32) | (u64)(u32)~(u32)(v - P.node_ptr[g]));
}

// what the two scans add up: per node "kept", per sorted key "distinct" (low half) and "distinct and kept" (high half)
__global__ __launch_bounds__(CC_BS) void cc_flags_kernel(CcWide P, long long items) {
    const long long i = cc_tid();
    if (i <= P.N) {
        u64 keep = 0;
        if (i < P.N) {
            const long long g = cc_wide_graph(P, i);
            if (g >= 0 && P.status[g] == TLC_ST_OK) keep = (u32)(P.parent[i] - (u32)P.node_ptr[g]) == ~(u32)P.best[g];
        }
        P.nscan[i] = keep;
    }
    if (i <= items) {
        u64 fl = 0;
        if (i < items) {
            const u32 u = P.klo[i], v = P.khi[i];
            const long long g = cc_wide_graph(P, u);
            if ((i == 0 || u != P.klo[i - 1] || v != P.khi[i - 1]) && g >= 0 && P.status[g] == TLC_ST_OK)
                fl = 1ull | ((u64)((u32)(P.parent[u] - (u32)P.node_ptr[g]) == ~(u32)P.best[g]) << 32);
        }
        P.escan[i] = fl;
    }
}

// in-place exclusive scan of v[0 .. count) in chunks of CC_BS * CC_SCAN_IPT: chunk sums, their scan by one workgroup, the chunks again
__global__ __launch_bounds__(CC_BS) void cc_scan_sums_kernel(const u64* __restrict__ v, long long count, u64* __restrict__ sums) {
    __shared__ BlockScratch<CC_BS> sh;
    const long long base = ((long long)blockIdx.x * CC_BS + threadIdx.x) * CC_SCAN_IPT;
    long long local = 0;
    for (int j = 0; j < CC_SCAN_IPT; ++j)
        if (base + j < count) local += (long long)v[base + j];
    long long total;
    block_excl_sum<CC_BS>(local, sh, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = (u64)total;
}
__global__ __launch_bounds__(CC_BS) void cc_scan_top_kernel(u64* __restrict__ sums, long long chunks) {
    __shared__ BlockScratch<CC_BS> sh;
    long long carry = 0;
    for (long long b0 = 0; b0 < chunks; b0 += CC_BS) {
        const long long b = b0 + threadIdx.x;
        const long long x = b < chunks ? (long long)sums[b] : 0;
        long long total;
        const long long ex = block_excl_sum<CC_BS>(x, sh, &total);
        if (b < chunks) sums[b] = (u64)(carry + ex);
        carry += total;
    }
}
__global__ __launch_bounds__(CC_BS) void cc_scan_apply_kernel(u64* __restrict__ v, long long count, const u64* __restrict__ sums) {
    __shared__ BlockScratch<CC_BS> sh;
    const long long base = ((long long)blockIdx.x * CC_BS + threadIdx.x) * CC_SCAN_IPT;
    long long x[CC_SCAN_IPT], local = 0;
    for (int j = 0; j < CC_SCAN_IPT; ++j) {
        x[j] = base + j < count ? (long long)v[base + j] : 0;
        local += x[j];
    }
    long long total;
    long long run = block_excl_sum<CC_BS>(local, sh, &total) + (long long)sums[blockIdx.x];
    for (int j = 0; j < CC_SCAN_IPT; ++j)
        if (base + j < count) {
            v[base + j] = (u64)run;
            run += x[j];
        }
}

__device__ __forceinline__ long long cc_lower_bound(const u32* __restrict__ k, long long count, long long x) {
    long long lo = 0, hi = count;                 // the first index whose key is >= x
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if ((long long)k[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// per computed WIDE graph: its stretch of the sorted keys, and its row of d_info
__global__ __launch_bounds__(CC_BS) void cc_graph_kernel(CcWide P, long long items) {
    const long long g = cc_tid();
    if (g >= P.B || P.cls[g] != CLS_WIDE || P.status[g] != TLC_ST_OK) return;
    const long long k0 = cc_lower_bound(P.klo, items, P.node_ptr[g]), k1 = cc_lower_bound(P.klo, items, P.node_ptr[g + 1]);
    const u64 d = P.escan[k1] - P.escan[k0];      // both halves at once: neither difference is negative
    P.first[g] = (int)k0;
    reinterpret_cast<int4*>(P.info)[g] = make_int4((int)(P.best[g] >> 32), (int)(d >> 32), P.comps[g], (int)(u32)d);
}

__global__ __launch_bounds__(CC_BS) void cc_output_kernel(CcWide P, long long items) {
    const long long i = cc_tid();
    if (i < P.N) {
        const long long g = cc_wide_graph(P, i);
        if (g >= 0 && P.status[g] == TLC_ST_OK)
            P.new_id[i] = P.nscan[i + 1] != P.nscan[i] ? (int)(P.nscan[i] - P.nscan[P.node_ptr[g]]) : -1;
    }
    if (i < items && (P.escan[i + 1] >> 32) != (P.escan[i] >> 32)) {
        const u32 u = P.klo[i], v = P.khi[i];
        const long long g = cc_wide_graph(P, u);          // a flagged key belongs to a computed WIDE graph
        const u64 nb = P.nscan[P.node_ptr[g]];
        const long long row = P.edge_ptr[g] + (long long)((P.escan[i] >> 32) - (P.escan[P.first[g]] >> 32));
        if (row < P.edge_ptr[g + 1])                      // always, unless offsets out of order made two graphs share a stretch of keys
            reinterpret_cast<int2*>(P.out_edges)[row] = make_int2((int)(P.nscan[u] - nb), (int)(P.nscan[v] - nb));
    }
}

inline unsigned cc_blocks(long long count) { return (unsigned)std::max<long long>(1, (count + CC_BS - 1) / CC_BS); }

int cc_scan(hipStream_t s, u64* v, long long count, u64* sums) {
    const long long chunks = (count + TlcGraphComponentsScratch::SCAN_CHUNK - 1) / TlcGraphComponentsScratch::SCAN_CHUNK;
    hipLaunchKernelGGL(cc_scan_sums_kernel, dim3((unsigned)chunks), dim3(CC_BS), 0, s, v, count, sums);
    hipLaunchKernelGGL(cc_scan_top_kernel, dim3(1), dim3(CC_BS), 0, s, sums, chunks);
    hipLaunchKernelGGL(cc_scan_apply_kernel, dim3((unsigned)chunks), dim3(CC_BS), 0, s, v, count, sums);
    TLC_HIP_CHECK(hipGetLastError());
    return TLC_OK;
}

// the two stable sorts that order the keys by (lo, hi): by hi, then by lo; the result is back in (klo_a, khi_a)
template <int BITS>
void cc_sort(hipStream_t s, long long items, u32* klo_a, u32* klo_b, u32* khi_a, u32* khi_b, int* hist, int* tot) {
    rk_sort<BITS>(s, items, khi_a, khi_b, klo_a, klo_b, hist, tot);
    rk_sort<BITS>(s, items, klo_a, klo_b, khi_a, khi_b, hist, tot);
}

int cc_wide(hipStream_t s, CcWide P, unsigned char* w, const TlcGraphComponentsScratch& L) {
    hipLaunchKernelGGL(cc_keys_kernel, dim3(cc_blocks(P.M)), dim3(CC_BS), 0, s, P);
    TLC_HIP_CHECK(hipGetLastError());
    int census[2] = {0, 0};                       // the class's graphs and keys: what the passes below are sized by
    TLC_HIP_CHECK(hipMemcpyAsync(census, P.head + H_WIDE_GRAPHS, sizeof(census), hipMemcpyDeviceToHost, s));
    TLC_HIP_CHECK(hipStreamSynchronize(s));
    if (census[0] == 0) return TLC_OK;
    const long long items = census[1], span = std::max(P.N, items);
    u32 *klo_b = (u32*)(w + L.klo_b), *khi_b = (u32*)(w + L.khi_b);
    int *hist = (int*)(w + L.hist), *tot = (int*)(w + L.tot);
    if (P.N > 65536) cc_sort<32>(s, items, P.klo, klo_b, P.khi, khi_b, hist, tot);
    else cc_sort<16>(s, items, P.klo, klo_b, P.khi, khi_b, hist, tot);
    hipLaunchKernelGGL(cc_init_kernel, dim3(cc_blocks(P.N)), dim3(CC_BS), 0, s, P);
    TLC_HIP_CHECK(hipGetLastError());
    int* flags = P.head + H_FLAGS;
    for (int r = 0; items > 0; ++r) {
        const int slot = r % CC_FLAG_SLOTS;
        if (slot == 0) TLC_HIP_CHECK(hipMemsetAsync(flags, 0, CC_FLAG_SLOTS * sizeof(int), s));
        hipLaunchKernelGGL(cc_round_kernel, dim3(cc_blocks(span)), dim3(CC_BS), 0, s, P, items, slot ? flags + slot - 1 : (const int*)nullptr, flags + slot);
        TLC_HIP_CHECK(hipGetLastError());
        if ((r + 1) % CC_ROUND_GROUP) continue;
        int changed = 0;                          // of the group's last round: zero as soon as one round of the group changed nothing
        TLC_HIP_CHECK(hipMemcpyAsync(&changed, flags + slot, sizeof(int), hipMemcpyDeviceToHost, s));
        TLC_HIP_CHECK(hipStreamSynchronize(s));
        if (!changed) break;
    }
    hipLaunchKernelGGL(cc_count_kernel, dim3(cc_blocks(P.N)), dim3(CC_BS), 0, s, P);
    hipLaunchKernelGGL(cc_winner_kernel, dim3(cc_blocks(P.N)), dim3(CC_BS), 0, s, P);
    hipLaunchKernelGGL(cc_flags_kernel, dim3(cc_blocks(span + 1)), dim3(CC_BS), 0, s, P, items);
    TLC_HIP_CHECK(hipGetLastError());
    int rc = cc_scan(s, P.nscan, P.N + 1, (u64*)(w + L.sums));
    if (rc == TLC_OK) rc = cc_scan(s, P.escan, items + 1, (u64*)(w + L.sums));
    if (rc != TLC_OK) return rc;
    hipLaunchKernelGGL(cc_graph_kernel, dim3(cc_blocks(P.B)), dim3(CC_BS), 0, s, P, items);
    hipLaunchKernelGGL(cc_output_kernel, dim3(cc_blocks(span)), dim3(CC_BS), 0, s, P, items);
    TLC_HIP_CHECK(hipGetLastError());
    return TLC_OK;
}

bool cc_sizes_ok(int64_t B, int64_t N, int64_t M) { return B >= 0 && B < (1ll << 31) && N >= 0 && N < (1ll << 31) && M >= 0 && M < (1ll << 31); }
TlcGraphComponentsScratch cc_layout(int64_t B, int64_t N, int64_t M) {
    return TlcGraphComponentsScratch(B, N, M, CC_WAVE_N, rk_hist_ints(M), RK_TOT_INTS);
}

}  // namespace

extern "C" int tlc_graph_components_work_bytes(int64_t n_graphs, int64_t total_nodes, int64_t total_edges, int64_t* bytes) {
    TLC_REQUIRE(bytes, "null pointer");
    TLC_REQUIRE(cc_sizes_ok(n_graphs, total_nodes, total_edges), "sizes: 0 .. 2^31 - 1");
    *bytes = cc_layout(n_graphs, total_nodes, total_edges).total;
    return TLC_OK;
}

extern "C" int tlc_graph_components(const int64_t* d_node_ptr, const int64_t* d_edge_ptr, const int32_t* d_edges, int64_t n_graphs, int64_t total_nodes,
                                    int64_t total_edges, int64_t max_nodes, int32_t* d_info, int32_t* d_new_id, int32_t* d_out_edges,
                                    uint8_t* d_status, void* d_work, int64_t work_bytes, void* stream) {
    TLC_REQUIRE(cc_sizes_ok(n_graphs, total_nodes, total_edges), "sizes: 0 .. 2^31 - 1");
    if (n_graphs == 0) return TLC_OK;
    TLC_REQUIRE(d_node_ptr && d_edge_ptr && d_info && d_status && d_work && (total_nodes == 0 || d_new_id) &&
                (total_edges == 0 || (d_edges && d_out_edges)), "null pointer");
    const TlcGraphComponentsScratch L = cc_layout(n_graphs, total_nodes, total_edges);
    TLC_REQUIRE(work_bytes >= L.total, "d_work is smaller than tlc_graph_components_work_bytes()");
    TLC_REQUIRE((reinterpret_cast<uintptr_t>(d_work) & 15) == 0, "d_work must be 16-byte aligned");
    int dev = 0, cus = 0;
    TLC_HIP_CHECK(hipGetDevice(&dev));
    TLC_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    if (cus <= 0) cus = 256;
    hipStream_t s = (hipStream_t)stream;
    unsigned char* w = (unsigned char*)d_work;
    CcWide P;
    P.B = n_graphs; P.N = total_nodes; P.M = total_edges;
    P.node_ptr = (const long long*)d_node_ptr; P.edge_ptr = (const long long*)d_edge_ptr; P.edges = d_edges;
    P.head = (int*)(w + L.head);
    P.cls = L.wide ? w + L.cls : nullptr;
    P.best = (u64*)(w + L.best); P.comps = (int*)(w + L.comps); P.first = (int*)(w + L.first);
    P.parent = (u32*)(w + L.parent); P.size = (int*)(w + L.size); P.nscan = (u64*)(w + L.nscan);
    P.klo = (u32*)(w + L.klo_a); P.khi = (u32*)(w + L.khi_a); P.escan = (u64*)(w + L.escan);
    P.info = d_info; P.new_id = d_new_id; P.out_edges = d_out_edges; P.status = d_status;
    int* list = (int*)(w + L.list);
    TLC_HIP_CHECK(hipMemsetAsync(P.head, 0, TlcGraphComponentsScratch::HEAD, s));
    hipLaunchKernelGGL(cc_bin_kernel, dim3(cc_blocks(P.B)), dim3(CC_BS), 0, s, P.B, P.N, P.M, (long long)max_nodes, P.node_ptr, P.edge_ptr, P.head, list,
                       P.cls, P.best, P.comps, d_info, d_status);
    TLC_HIP_CHECK(hipGetLastError());
    const long long g_wave = std::min<long long>((P.B + 3) / 4, 8ll * cus);
    hipLaunchKernelGGL(cc_wave_kernel, dim3((unsigned)g_wave), dim3(CC_BS), 0, s, P.node_ptr, P.edge_ptr, d_edges, d_info, d_new_id, d_out_edges, d_status,
                       P.head, list);
    TLC_HIP_CHECK(hipGetLastError());
    // no graph can be WIDE where the totals or the caller's bound say so: nothing more is launched and nothing is read back
    if (!L.wide || (max_nodes >= 0 && max_nodes <= CC_WAVE_N)) return TLC_OK;
    return cc_wide(s, P, w, L);
}

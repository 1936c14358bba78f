// struct_filt.hip -- tlc_struct_batch: the degree / centrality / clustering filtrations of a packed batch of graphs, the node functions that
// the reference computes with networkx (Knowledge_Distillation/data_utils_LP.py:131-133; data_utils_NC.py:124-135) and this project's host
// route with numpy + scipy (`data_utils_LP.structural_filtration`, whose docstring is the specification):
//   degree      d
//   centrality  d * (1.0 / (n - 1.0))     (n == 1: 1.0)
//   clustering  t / (d * (d - 1)), t = sum over the incident edges (v, w) of |N(v) & N(w)|; 0.0 where t == 0
// each optionally divided by (the graph's max + 1e-10).
//
// Bit-exact by construction: d and t are INTEGERS, counted with integer atomics (LDS or global) or fixed-order sums, so they do not depend on
// the order in which edges arrive; what follows is one int -> fp64 conversion and one or two correctly rounded fp64 operations per value
// (-ffp-contract=off, the Makefile's default: no FMA), the same operations in the same order as the host route.  The maximum is a maximum of
// non-negative doubles -- order-free; in the workgroup tiers an integer atomicMax on their bit patterns.  No floating-point atomics anywhere.
//
// Input check (TLC_ST_BAD_INPUT, nothing of the graph written): offsets while binning; ids outside 0 .. n-1 and self loops before anything is
// indexed by an id; an unordered pair listed twice, in either orientation, by the bit of the adjacency bitmap that is found already set.
// More than n (n - 1) / 2 edges cannot be a simple graph (a pair repeats): refused while binning, which also bounds every tier's edge count.
//
// Tiers by node count, binned ON THE DEVICE from node_ptr; every tier is a persistent loop that draws graphs from its list by a ticket:
//   WAVE    n <= 64    one wavefront per graph, four per workgroup: lane v owns row v of the adjacency matrix as one u64 in LDS (atomicOr),
//                      d = popcount(row), t = sum over the set bits w of popcount(row_v & row_w); the maximum is a wavefront reduction
//   LDS256  n <= 256   one 256-thread workgroup per graph; rows of ceil(n / 64) u64 words in LDS (12 KiB), work per EDGE: AND + popcount
//   LDS1024 n <= 1024  over the two rows, LDS integer atomicAdd into t[a] and t[b] (t <= 1023 * 1022 fits 32 bits); 1 024 threads, 144 KiB
//   CSR     larger     one 1 024-thread workgroup per graph; a CSR of the graph in d_work (count, scan, fill; 64-bit offsets), then one
//                      wavefront per node v: N(v) marked in the wavefront's own LDS bitmap (TLC_STRUCT_BITMAP_BITS bits = 8 KiB; a set bit
//                      found while marking is a repeated edge), |N(v) & N(w)| for the neighbours w > v by testing N(w) against the bitmap,
//                      added to t[v] and t[w] (64-bit integer atomics: 46 341^2 exceeds 2^31).  A graph of more nodes than the bitmap has
//                      bits takes one pass per window of TLC_STRUCT_BITMAP_BITS ids.
// LDS rows have W + 1 words (odd count of u64): a walk down a column of words, one row per lane, touches every bank pair once.
#include "tlc_common.h"

#include <algorithm>

#define ST_WAVE_N TLC_STRUCT_WAVE_NMAX
#define ST_S_N TLC_STRUCT_LDS_SMALL_NMAX
#define ST_L_N TLC_STRUCT_LDS_NMAX
#define ST_BITS TLC_STRUCT_BITMAP_BITS
#define ST_HEAD_BYTES 256           // tier counts [4], tickets [4] (int), then the CSR tier's two allocation cursors (u64: nodes, edges)
#define ST_KINDS (TLC_STRUCT_DEGREE | TLC_STRUCT_CENTRALITY | TLC_STRUCT_CLUSTERING)
#define ST_CSR_NT 1024
#define ST_CSR_WAVES (ST_CSR_NT / 64)
#define ST_LIGHT 64                 // CSR tier: a neighbour of at most this degree is walked by one lane, a heavier one by the wavefront

namespace {

typedef unsigned long long u64;

__device__ __forceinline__ void st_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// the un-normalised value of one node: the host route's operations in its order
__device__ __forceinline__ double st_raw(unsigned bit, long long n, long long d, long long t) {
    if (bit == TLC_STRUCT_DEGREE) return (double)d;
    if (bit == TLC_STRUCT_CENTRALITY) return n > 1 ? (double)d * (1.0 / ((double)n - 1.0)) : 1.0;
    return t > 0 ? (double)t / (double)(d * (d - 1)) : 0.0;
}

// ---- binning: one thread per graph ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void st_bin_kernel(long long B, long long total_nodes, long long total_edges, const long long* __restrict__ node_ptr,
                                                     const long long* __restrict__ edge_ptr, int* __restrict__ head, int* __restrict__ lists,
                                                     unsigned char* __restrict__ status) {
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    int tier = -1;
    if (g < B) {
        const long long n0 = node_ptr[g], n1 = node_ptr[g + 1], e0 = edge_ptr[g], e1 = edge_ptr[g + 1];
        const long long n = n1 - n0, m = e1 - e0;
        if (n0 < 0 || n1 < n0 || n1 > total_nodes || e0 < 0 || e1 < e0 || e1 > total_edges) status[g] = TLC_ST_BAD_INPUT;
        else if (n > 0x7fffffffll || (n == 0 && m > 0) || (n > 0 && m > (n & 1 ? n * ((n - 1) >> 1) : (n >> 1) * (n - 1)))) status[g] = TLC_ST_BAD_INPUT;
        else {
            status[g] = TLC_ST_OK;
            if (n > 0) tier = n <= ST_WAVE_N ? 0 : n <= ST_S_N ? 1 : n <= ST_L_N ? 2 : 3;
        }
    }
    // one atomic per wavefront and tier
    for (int t = 0; t < 4; ++t) {
        const unsigned long long mask = __ballot(tier == t);
        if (!mask) continue;
        int base = 0;
        if (tlc_lane() == __ffsll((long long)mask) - 1) base = atomicAdd(&head[t], __popcll(mask));
        base = __shfl(base, __ffsll((long long)mask) - 1);
        if (tier == t) lists[(long long)t * B + base + __popcll(mask & tlc_lanemask_lt())] = (int)g;
    }
}

// ---- WAVE: n <= 64 ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int st_wave_graph(u64* row, int* flag, int lane, int n, int m, const int* __restrict__ edges, unsigned kinds,
                                             unsigned flags, double* __restrict__ out, long long stride) {
    row[lane] = 0;
    if (lane == 0) flag[0] = 0;
    st_wave_sync();
    for (int e = lane; e < m; e += 64) {
        const int a = edges[2 * e], b = edges[2 * e + 1];
        if ((unsigned)a >= (unsigned)n || (unsigned)b >= (unsigned)n || a == b) flag[0] = 1;
        else {
            const u64 old = atomicOr(&row[a], 1ull << b);
            if ((old >> b) & 1) flag[0] = 1;                  // (a, b) or (b, a) was there already
            atomicOr(&row[b], 1ull << a);
        }
    }
    st_wave_sync();
    if (flag[0]) return TLC_ST_BAD_INPUT;
    const u64 mine = row[lane];
    const int d = __popcll(mine);
    int t = 0;
    for (u64 r = mine; r; r &= r - 1) t += __popcll(mine & row[__ffsll((long long)r) - 1]);
    int k = 0;
    for (unsigned bit = TLC_STRUCT_DEGREE; bit <= TLC_STRUCT_CLUSTERING; bit <<= 1) {
        if (!(kinds & bit)) continue;
        double v = lane < n ? st_raw(bit, n, d, t) : 0.0;
        if (flags & TLC_STRUCT_NORMALISE) v = v / (tlc_wave_max_f64(v) + 1e-10);
        if (lane < n) out[(long long)k * stride + lane] = v;
        ++k;
    }
    return TLC_ST_OK;
}

__global__ __launch_bounds__(256) void st_wave_kernel(long long B, const long long* __restrict__ node_ptr, const long long* __restrict__ edge_ptr,
                                                      const int* __restrict__ edges, unsigned kinds, unsigned flags, double* __restrict__ out,
                                                      long long stride, unsigned char* __restrict__ status, int* __restrict__ head,
                                                      const int* __restrict__ lists) {
    __shared__ u64 rows[4][64];
    __shared__ int flags_s[4][2];
    const int lane = tlc_lane(), wv = (int)(threadIdx.x >> 6);
    const int count = head[0];
    for (;;) {
        int i = lane == 0 ? atomicAdd(&head[4], 1) : 0;
        i = __builtin_amdgcn_readfirstlane(i);
        if (i >= count) break;
        const int g = lists[i];
        const long long n0 = node_ptr[g], e0 = edge_ptr[g];
        const int n = (int)(node_ptr[g + 1] - n0), m = (int)(edge_ptr[g + 1] - e0);
        const int st = st_wave_graph(rows[wv], flags_s[wv], lane, n, m, edges + 2 * e0, kinds, flags, out + n0, stride);
        if (lane == 0 && st != TLC_ST_OK) status[g] = (unsigned char)st;
        st_wave_sync();
    }
}

// ---- LDS256 / LDS1024: adjacency bitmap of the whole graph in LDS --------------------------------------------------------------------
constexpr int st_lds_ld(int nmax) { return nmax / 64 + 1; }
// rows[NMAX][LD] u64 | mx[3] u64, ticket + flag (32 B) | t[NMAX] u32 | deg[NMAX] u32
constexpr size_t st_lds_bytes(int nmax) { return (size_t)nmax * st_lds_ld(nmax) * 8 + 32 + (size_t)nmax * 8; }

// the shared epilogue of the workgroup tiers: raw values, the maximum by integer atomicMax on the bit patterns (non-negative doubles order
// like their bits), the division.  deg_of / t_of: the integer counts of node v.
template <int NT, class DegOf, class TOf>
__device__ __forceinline__ void st_write(u64* mx, int tid, long long n, unsigned kinds, unsigned flags, double* __restrict__ out, long long stride,
                                         DegOf deg_of, TOf t_of) {
    if (tid < 3) mx[tid] = 0;
    __syncthreads();
    if (flags & TLC_STRUCT_NORMALISE) {
        for (long long v = tid; v < n; v += NT) {
            const long long d = deg_of(v), t = (kinds & TLC_STRUCT_CLUSTERING) ? t_of(v) : 0;
            int k = 0;
            for (unsigned bit = TLC_STRUCT_DEGREE; bit <= TLC_STRUCT_CLUSTERING; bit <<= 1, ++k)
                if (kinds & bit) atomicMax(&mx[k], (u64)__double_as_longlong(st_raw(bit, n, d, t)));
        }
        __syncthreads();
    }
    for (long long v = tid; v < n; v += NT) {
        const long long d = deg_of(v), t = (kinds & TLC_STRUCT_CLUSTERING) ? t_of(v) : 0;
        int k = 0, r = 0;
        for (unsigned bit = TLC_STRUCT_DEGREE; bit <= TLC_STRUCT_CLUSTERING; bit <<= 1, ++k) {
            if (!(kinds & bit)) continue;
            const double raw = st_raw(bit, n, d, t);
            out[(long long)r * stride + v] = (flags & TLC_STRUCT_NORMALISE) ? raw / (__longlong_as_double((long long)mx[k]) + 1e-10) : raw;
            ++r;
        }
    }
}

template <int NMAX, int NT>
__device__ __forceinline__ int st_lds_graph(u64* rows, u64* mx, int* flag, unsigned* tcnt, unsigned* deg, int tid, int n, int m,
                                            const int* __restrict__ edges, unsigned kinds, unsigned flags, double* __restrict__ out, long long stride) {
    constexpr int LD = st_lds_ld(NMAX);
    const int W = (n + 63) >> 6;
    for (int i = tid; i < n * LD; i += NT) rows[i] = 0;
    for (int i = tid; i < n; i += NT) tcnt[i] = 0;
    if (tid == 0) flag[0] = 0;
    __syncthreads();
    for (int e = tid; e < m; e += NT) {
        const int a = edges[2 * e], b = edges[2 * e + 1];
        if ((unsigned)a >= (unsigned)n || (unsigned)b >= (unsigned)n || a == b) flag[0] = 1;
        else {
            const u64 bit = 1ull << (b & 63);
            if (atomicOr(&rows[a * LD + (b >> 6)], bit) & bit) flag[0] = 1;      // (a, b) or (b, a) was there already
            atomicOr(&rows[b * LD + (a >> 6)], 1ull << (a & 63));
        }
    }
    __syncthreads();
    if (flag[0]) return TLC_ST_BAD_INPUT;
    if (kinds & TLC_STRUCT_CLUSTERING)
        for (int e = tid; e < m; e += NT) {
            const int a = edges[2 * e], b = edges[2 * e + 1];
            const u64 *ra = rows + a * LD, *rb = rows + b * LD;
            unsigned c = 0;
            for (int j = 0; j < W; ++j) c += (unsigned)__popcll(ra[j] & rb[j]);
            if (c) { atomicAdd(&tcnt[a], c); atomicAdd(&tcnt[b], c); }
        }
    for (int v = tid; v < n; v += NT) {
        unsigned d = 0;
        for (int j = 0; j < W; ++j) d += (unsigned)__popcll(rows[v * LD + j]);
        deg[v] = d;
    }
    __syncthreads();
    st_write<NT>(mx, tid, n, kinds, flags, out, stride, [&](long long v) { return (long long)deg[v]; }, [&](long long v) { return (long long)tcnt[v]; });
    return TLC_ST_OK;
}

template <int NMAX, int NT>
__global__ __launch_bounds__(NT) void st_lds_kernel(int tier, long long B, const long long* __restrict__ node_ptr, const long long* __restrict__ edge_ptr,
                                                    const int* __restrict__ edges, unsigned kinds, unsigned flags, double* __restrict__ out,
                                                    long long stride, unsigned char* __restrict__ status, int* __restrict__ head,
                                                    const int* __restrict__ lists) {
    extern __shared__ __attribute__((aligned(16))) unsigned char st_smem[];
    u64* rows = reinterpret_cast<u64*>(st_smem);
    u64* mx = rows + (size_t)NMAX * st_lds_ld(NMAX);
    int* flag = reinterpret_cast<int*>(mx + 3);
    unsigned* tcnt = reinterpret_cast<unsigned*>(mx + 4);
    unsigned* deg = tcnt + NMAX;
    const int tid = (int)threadIdx.x;
    const int count = head[tier];
    const int* list = lists + (long long)tier * B;
    for (;;) {
        if (tid == 0) flag[1] = atomicAdd(&head[4 + tier], 1);
        __syncthreads();
        const int i = flag[1];
        __syncthreads();
        if (i >= count) break;
        const int g = list[i];
        const long long n0 = node_ptr[g], e0 = edge_ptr[g];
        const int n = (int)(node_ptr[g + 1] - n0), m = (int)(edge_ptr[g + 1] - e0);
        const int st = st_lds_graph<NMAX, NT>(rows, mx, flag, tcnt, deg, tid, n, m, edges + 2 * e0, kinds, flags, out + n0, stride);
        if (tid == 0 && st != TLC_ST_OK) status[g] = (unsigned char)st;
        __syncthreads();
    }
}

// ---- CSR: any size --------------------------------------------------------------------------------------------------------------------
// values other wavefronts changed with atomics (they live in L2): read past this CU's L1
__device__ __forceinline__ long long st_load_l2(const long long* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// LDS: bm[ST_CSR_WAVES][ST_BITS / 32] u32 | sc[ST_CSR_NT] i64 | mx[3] u64, ticket + flag (32 B)
constexpr size_t st_csr_lds_bytes() { return (size_t)ST_CSR_WAVES * (ST_BITS / 8) + (size_t)ST_CSR_NT * 8 + 32; }

// cnt[n]: degree counters, then fill cursors (counted back down to 0), then t;  rp[n + 1];  col[2 m]
__device__ __forceinline__ int st_csr_graph(unsigned* bm_all, long long* sc, u64* mx, int* flag, int tid, long long n, long long m,
                                            const int* __restrict__ edges, long long* cnt, long long* rp, int* col, unsigned kinds, unsigned flags,
                                            double* __restrict__ out, long long stride) {
    constexpr int NT = ST_CSR_NT;
    const int lane = tid & 63, wv = tid >> 6;
    for (long long i = tid; i < n; i += NT) cnt[i] = 0;
    if (tid == 0) flag[0] = 0;
    __threadfence();
    __syncthreads();
    for (long long e = tid; e < m; e += NT) {
        const int a = edges[2 * e], b = edges[2 * e + 1];
        if ((unsigned)a >= (unsigned long long)n || (unsigned)b >= (unsigned long long)n || a == b) flag[0] = 1;
        else { atomicAdd((u64*)&cnt[a], 1ull); atomicAdd((u64*)&cnt[b], 1ull); }
    }
    __threadfence();
    __syncthreads();
    if (flag[0]) return TLC_ST_BAD_INPUT;
    // exclusive scan of the degrees: a contiguous segment per thread, the segment sums by a doubling scan in LDS
    const long long seg = (n + NT - 1) / NT, s0 = std::min<long long>(n, tid * seg), s1 = std::min<long long>(n, s0 + seg);
    long long local = 0;
    for (long long v = s0; v < s1; ++v) local += st_load_l2(&cnt[v]);
    sc[tid] = local;
    __syncthreads();
    for (int off = 1; off < NT; off <<= 1) {
        const long long x = tid >= off ? sc[tid - off] : 0;
        __syncthreads();
        sc[tid] += x;
        __syncthreads();
    }
    long long run = sc[tid] - local;
    for (long long v = s0; v < s1; ++v) { rp[v] = run; run += st_load_l2(&cnt[v]); }
    if (tid == NT - 1) rp[n] = sc[NT - 1];
    __threadfence();
    __syncthreads();
    for (long long e = tid; e < m; e += NT) {
        const int a = edges[2 * e], b = edges[2 * e + 1];
        col[rp[a] + (long long)atomicAdd((u64*)&cnt[a], ~0ull) - 1] = b;
        col[rp[b] + (long long)atomicAdd((u64*)&cnt[b], ~0ull) - 1] = a;
    }
    unsigned* bm = bm_all + (size_t)wv * (ST_BITS / 32);
    for (int i = lane; i < ST_BITS / 32; i += 64) bm[i] = 0;
    __threadfence();
    __syncthreads();                                            // cnt is all zero again: it is t from here on
    // one wavefront per node (no workgroup barrier inside: the wavefronts run their nodes independently)
    for (long long v = wv; v < n; v += ST_CSR_WAVES) {
        const long long r0 = rp[v], dv = rp[v + 1] - r0;
        if (dv == 0) continue;
        long long tv = 0;
        for (long long c0 = 0; c0 < n; c0 += ST_BITS) {
            for (long long j = lane; j < dv; j += 64) {
                const long long x = col[r0 + j] - c0;
                if (x >= 0 && x < ST_BITS) {
                    const unsigned bit = 1u << (x & 31);
                    if (atomicOr(&bm[x >> 5], bit) & bit) flag[0] = 1;           // w twice in N(v): a repeated edge
                }
            }
            st_wave_sync();
            if (kinds & TLC_STRUCT_CLUSTERING)
                for (long long base = 0; base < dv; base += 64) {
                    const long long j = base + lane;
                    const int w = j < dv ? col[r0 + j] : -1;
                    const bool active = w > v;                                   // each edge once, from its lower end
                    const long long w0 = active ? rp[w] : 0, dw = active ? rp[w + 1] - w0 : 0;
                    const bool heavy = dw > ST_LIGHT;
                    long long c = 0;
                    if (!heavy)
                        for (long long k = 0; k < dw; ++k) {
                            const long long x = col[w0 + k] - c0;
                            if (x >= 0 && x < ST_BITS) c += (bm[x >> 5] >> (x & 31)) & 1u;
                        }
                    for (u64 hm = __ballot(heavy); hm; hm &= hm - 1) {
                        const int l = __ffsll((long long)hm) - 1;
                        const long long hw0 = __shfl(w0, l), hdw = __shfl(dw, l);
                        long long cc = 0;
                        for (long long k = lane; k < hdw; k += 64) {
                            const long long x = col[hw0 + k] - c0;
                            if (x >= 0 && x < ST_BITS) cc += (bm[x >> 5] >> (x & 31)) & 1u;
                        }
                        cc = tlc_wave_sum_i64(cc);
                        if (lane == l) c = cc;
                    }
                    if (c) atomicAdd((u64*)&cnt[w], (u64)c);
                    tv += c;
                }
            st_wave_sync();
            for (long long j = lane; j < dv; j += 64) {
                const long long x = col[r0 + j] - c0;
                if (x >= 0 && x < ST_BITS) bm[x >> 5] = 0;
            }
            st_wave_sync();
        }
        tv = tlc_wave_sum_i64(tv);
        if (lane == 0 && tv) atomicAdd((u64*)&cnt[v], (u64)tv);
    }
    __threadfence();
    __syncthreads();
    if (flag[0]) return TLC_ST_BAD_INPUT;
    st_write<NT>(mx, tid, n, kinds, flags, out, stride, [&](long long v) { return rp[v + 1] - rp[v]; }, [&](long long v) { return st_load_l2(&cnt[v]); });
    return TLC_ST_OK;
}

__global__ __launch_bounds__(ST_CSR_NT) void st_csr_kernel(long long B, const long long* __restrict__ node_ptr, const long long* __restrict__ edge_ptr,
                                                           const int* __restrict__ edges, unsigned kinds, unsigned flags, double* __restrict__ out,
                                                           long long stride, unsigned char* __restrict__ status, int* __restrict__ head,
                                                           const int* __restrict__ lists, long long total_nodes, long long total_edges,
                                                           long long* cnt, long long* rp, int* col) {
    extern __shared__ __attribute__((aligned(16))) unsigned char st_smem[];
    unsigned* bm = reinterpret_cast<unsigned*>(st_smem);
    long long* sc = reinterpret_cast<long long*>(st_smem + (size_t)ST_CSR_WAVES * (ST_BITS / 8));
    u64* mx = reinterpret_cast<u64*>(sc + ST_CSR_NT);
    int* flag = reinterpret_cast<int*>(mx + 3);
    const int tid = (int)threadIdx.x;
    const int count = head[3];
    const int* list = lists + 3 * B;
    u64* cursor = reinterpret_cast<u64*>(head + 8);
    for (;;) {
        if (tid == 0) flag[1] = atomicAdd(&head[4 + 3], 1);
        __syncthreads();
        const int i = flag[1];
        __syncthreads();
        if (i >= count) break;
        const int g = list[i];
        const long long n0 = node_ptr[g], e0 = edge_ptr[g];
        const long long n = node_ptr[g + 1] - n0, m = edge_ptr[g + 1] - e0;
        // the graph's slices of the workspace (n + 1 entries of cnt and rp, 2 m of col), handed out by two cursors: the graphs of a batch
        // with offsets in order hold at most total_nodes nodes and total_edges edges together; where slices of out-of-order offsets
        // overlap and the sum goes beyond, the graph is refused instead of written past the workspace
        if (tid == 0) {
            sc[0] = (long long)atomicAdd(&cursor[0], (u64)n + 1);
            sc[1] = (long long)atomicAdd(&cursor[1], (u64)m);
        }
        __syncthreads();
        const long long na = sc[0], ea = sc[1];
        __syncthreads();
        int st = TLC_ST_BAD_INPUT;
        if (na + n + 1 <= total_nodes + B && ea + m <= total_edges)
            st = st_csr_graph(bm, sc, mx, flag, tid, n, m, edges + 2 * e0, cnt + na, rp + na, col + 2 * ea, kinds, flags, out + n0, stride);
        if (tid == 0 && st != TLC_ST_OK) status[g] = (unsigned char)st;
        __syncthreads();
    }
}

struct StLayout {
    int cus;
    bool csr;
    size_t lists_off, cnt_off, rp_off, col_off, bytes;
};

int st_layout(int64_t B, int64_t total_nodes, int64_t total_edges, StLayout* L) {
    int dev = 0, cus = 0;
    TLC_HIP_CHECK(hipGetDevice(&dev));
    TLC_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    if (cus <= 0) cus = 256;
    L->cus = cus;
    L->csr = total_nodes > ST_L_N;                               // a batch of at most ST_L_N nodes has no graph for the CSR tier
    L->lists_off = ST_HEAD_BYTES;
    L->cnt_off = (L->lists_off + (size_t)4 * (size_t)B * sizeof(int) + 255) & ~(size_t)255;
    L->rp_off = L->cnt_off + (L->csr ? ((size_t)total_nodes + (size_t)B) * 8 : 0);
    L->col_off = L->rp_off + (L->csr ? ((size_t)total_nodes + (size_t)B) * 8 : 0);
    L->bytes = L->col_off + (L->csr ? (size_t)total_edges * 8 : 0);
    return TLC_OK;
}

}  // namespace

extern "C" int tlc_struct_batch_work_bytes(int64_t n_graphs, int64_t total_nodes, int64_t total_edges, uint32_t kinds, int64_t* bytes) {
    TLC_REQUIRE(bytes, "null pointer");
    TLC_REQUIRE(n_graphs >= 0 && n_graphs < (1ll << 31) && total_nodes >= 0 && total_edges >= 0, "bad sizes");
    TLC_REQUIRE(kinds != 0 && (kinds & ~ST_KINDS) == 0, "kinds: one or more of TLC_STRUCT_DEGREE / CENTRALITY / CLUSTERING");
    StLayout L;
    const int rc = st_layout(n_graphs, total_nodes, total_edges, &L);
    if (rc != TLC_OK) return rc;
    *bytes = (int64_t)L.bytes;
    return TLC_OK;
}

extern "C" int tlc_struct_batch(const int64_t* d_node_ptr, const int64_t* d_edge_ptr, const int32_t* d_edges, int64_t n_graphs, int64_t total_nodes,
                                int64_t total_edges, uint32_t kinds, uint32_t flags, double* d_out, uint8_t* d_status, void* d_work,
                                int64_t work_bytes, void* stream) {
    TLC_REQUIRE(n_graphs >= 0 && n_graphs < (1ll << 31) && total_nodes >= 0 && total_edges >= 0, "bad sizes");
    TLC_REQUIRE(kinds != 0 && (kinds & ~ST_KINDS) == 0, "kinds: one or more of TLC_STRUCT_DEGREE / CENTRALITY / CLUSTERING");
    TLC_REQUIRE((flags & ~TLC_STRUCT_NORMALISE) == 0, "unknown flag");
    if (n_graphs == 0) return TLC_OK;
    TLC_REQUIRE(d_node_ptr && d_edge_ptr && d_status && d_work && (total_nodes == 0 || d_out) && (total_edges == 0 || d_edges), "null pointer");
    StLayout L;
    const int rc = st_layout(n_graphs, total_nodes, total_edges, &L);
    if (rc != TLC_OK) return rc;
    TLC_REQUIRE(work_bytes >= (int64_t)L.bytes, "d_work is smaller than tlc_struct_batch_work_bytes()");
    TLC_REQUIRE((reinterpret_cast<uintptr_t>(d_work) & 15) == 0, "d_work must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    unsigned char* w = (unsigned char*)d_work;
    int* head = (int*)w;
    int* lists = (int*)(w + L.lists_off);
    const long long B = n_graphs;
    const long long* np = (const long long*)d_node_ptr;
    const long long* ep = (const long long*)d_edge_ptr;
    TLC_HIP_CHECK(hipMemsetAsync(head, 0, ST_HEAD_BYTES, s));
    hipLaunchKernelGGL(st_bin_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, B, (long long)total_nodes, (long long)total_edges, np, ep, head,
                       lists, d_status);
    TLC_HIP_CHECK(hipGetLastError());

    constexpr size_t lds_s = st_lds_bytes(ST_S_N), lds_l = st_lds_bytes(ST_L_N), lds_c = st_csr_lds_bytes();
    static_assert(lds_l <= 160 * 1024 && lds_c <= 160 * 1024, "LDS budget of a gfx950 workgroup");
    TLC_HIP_CHECK(hipFuncSetAttribute((const void*)st_lds_kernel<ST_L_N, 1024>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_l));
    TLC_HIP_CHECK(hipFuncSetAttribute((const void*)st_csr_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_c));
    const long long cus = L.cus, stride = total_nodes;
    // a graph of the later tiers has at least 65 / 257 / 1 025 nodes: no more workgroups than the batch can hold such graphs
    const long long g_wave = std::min<long long>((B + 3) / 4, 8 * cus);
    const long long g_s = std::min<long long>(std::min<long long>(B, total_nodes / (ST_WAVE_N + 1)), 8 * cus);
    const long long g_l = std::min<long long>(std::min<long long>(B, total_nodes / (ST_S_N + 1)), cus);
    const long long g_c = std::min<long long>(std::min<long long>(B, total_nodes / (ST_L_N + 1)), cus);
    hipLaunchKernelGGL(st_wave_kernel, dim3((unsigned)g_wave), dim3(256), 0, s, B, np, ep, d_edges, kinds, flags, d_out, stride, d_status, head, lists);
    TLC_HIP_CHECK(hipGetLastError());
    if (g_s > 0) {
        hipLaunchKernelGGL((st_lds_kernel<ST_S_N, 256>), dim3((unsigned)g_s), dim3(256), lds_s, s, 1, B, np, ep, d_edges, kinds, flags, d_out, stride,
                           d_status, head, lists);
        TLC_HIP_CHECK(hipGetLastError());
    }
    if (g_l > 0) {
        hipLaunchKernelGGL((st_lds_kernel<ST_L_N, 1024>), dim3((unsigned)g_l), dim3(1024), lds_l, s, 2, B, np, ep, d_edges, kinds, flags, d_out, stride,
                           d_status, head, lists);
        TLC_HIP_CHECK(hipGetLastError());
    }
    if (g_c > 0) {
        hipLaunchKernelGGL(st_csr_kernel, dim3((unsigned)g_c), dim3(ST_CSR_NT), lds_c, s, B, np, ep, d_edges, kinds, flags, d_out, stride, d_status, head,
                           lists, (long long)total_nodes, (long long)total_edges, (long long*)(w + L.cnt_off), (long long*)(w + L.rp_off), (int*)(w + L.col_off));
        TLC_HIP_CHECK(hipGetLastError());
    }
    return TLC_OK;
}

// pd_wide.hip -- extended persistence of one big graph on the whole device (tlc_pd_wide): the tier without a node cap behind
// tlc_pd_from_filtration's one-workgroup HUGE tier.  32-bit ids, every array in global memory, grid-stride kernels, and kernel
// boundaries wherever the LDS version (ext1_dc.h) has a barrier.  No grid-wide barrier, no workgroup waits for another one.
//
// Stages of one graph (n nodes, m edges):
//   1. keys      asc = hi + (lo + 1) * 1e-6, desc = lo - (101 - hi) * 1e-6 in fp64 without contraction, as order-preserving u64.
//   2. two sorts the LSD radix sort of radix_passes.h.  Ascending: (asc key, edge id) -> ranks ra.  Descending: (desc key
//                descending, ra descending) -> ranks rd: the contract of fix_desc_ties as a second sort key, for runs of any length.
//                The edges are sorted without the nodes: for -1 <= f <= 101, the domain of the reference's perturbation, every node
//                enters before its edges, so the merged order's edge subsequence is this one; an edge with an end outside that
//                range is TLC_ST_BAD_INPUT.  Everything below is integer ranks.
//   3. forests   one segmented Boruvka primitive (msf_*): a 64-bit atomicMin of (rank << 32 | item) per component, hooking, pointer
//                jumping.  Ranks are unique, so the forest does not depend on the scheduling.  On ra: the ascending pass's spanning
//                forest.  On rd: the Neg / Pos split and the component labels.
//   4. passes    the elder rule over the forest edges only, in sorted order (a non-tree edge merges nothing): one lane per pass, the
//                two passes and the ext0 reduction in three workgroups of one launch, comp[] in LDS up to TLC_PD_WIDE_LDS_NODES nodes
//                and in global memory (L2) above.  This is the serial remainder: n - c steps each.
//   5. swap      sim_dc_ext1.py / ext1_dc.h level by level: P and Q slots, routing by T_mid = MSF(P + Q[l, mid)), contraction of the
//                edges alive throughout a child (one connectivity call in a doubled id space), dense renumbering by a prefix sum.
//                ceil(log2 K) levels; then the end checks of ext1_dc.h: each query owns exactly one removed edge, heavier than itself.
//   6. fallback  if a check fails (or TLC_PD_WIDE_FORCE_FALLBACK), one lane runs the reference's serial swap on fp64 keys.
//   7. points    flags, prefix sum, compaction: the order of the output is the order of the queries; no cursor atomics.
//
// The host loops are bounded by m alone: ceil(log2 m) levels, ceil(log2 V) rounds per forest; a device flag per round and the
// device's level count make the surplus launches return at once, so there is no host synchronisation inside or between graphs.
#include "radix_passes.h"
#include "pd_keys.h"

#include <limits.h>

namespace {

#define PDW_BS TLC_PD_WIDE_BLOCK            // threads per workgroup of every grid-stride kernel
#define PDW_SCAN_IPT 8
#define PDW_SCAN_CHUNK TLC_PD_WIDE_SCAN_CHUNK   // items per workgroup of the prefix sums
#define PDW_MAX_GRID 4096
#define PDW_LDS_NODES TLC_PD_WIDE_LDS_NODES   // most nodes whose comp[] of an elder-rule pass lives in LDS (160 000 B of the 160 KiB)
#define PDW_NOKEY 0xffffffffffffffffull
static_assert(PDW_BS == RK_BS, "the sort and the kernels here share one workgroup width");
static_assert(PDW_SCAN_CHUNK == PDW_BS * PDW_SCAN_IPT, "scan chunk");
static_assert(TLC_PD_WIDE_SORT_TILE == RK_TILE, "sort tile");

// control block (ints, device)
enum {
    C_STATUS = 0, C_N, C_M, C_LEVELS, C_ROUNDS, C_FAIL, C_FELL, C_MINID, C_NPOS, C_K, C_NDY, C_NFIN, C_NUP, C_NDOWN, C_NONE, C_NNEG,
    C_TWOK, C_FLAGS = 32,      // 40 round flags of the running forest call
    C_NS = 72,                 // supernode count of each level (40)
    C_INTS = 112
};

struct Gate {
    const int* ctl;
    int lv;                    // -1: not part of the level loop
};
__device__ __forceinline__ bool closed(const Gate g) { return g.ctl[C_STATUS] != 0 || g.lv >= g.ctl[C_LEVELS]; }

#define PDW_FOR(i, count) for (int i = (int)(blockIdx.x * PDW_BS + threadIdx.x); i < (count); i += (int)(gridDim.x * PDW_BS))

__global__ __launch_bounds__(PDW_BS) void pdw_ctl_kernel(int* __restrict__ ctl, int n, int m) {
    if (threadIdx.x < C_INTS) ctl[threadIdx.x] = threadIdx.x == C_N ? n : threadIdx.x == C_M ? m : threadIdx.x == C_MINID ? INT_MAX : 0;
}

// ---- input check and ascending keys ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(PDW_BS) void pdw_keys_kernel(int* __restrict__ ctl, int n, int m, const int* __restrict__ edges,
                                                          const double* __restrict__ f, unsigned long long* __restrict__ key,
                                                          unsigned* __restrict__ val) {
    PDW_FOR(e, m) {
        const int u = edges[2 * e], v = edges[2 * e + 1];
        unsigned long long k = 0;
        if ((unsigned)u >= (unsigned)n || (unsigned)v >= (unsigned)n || u == v) ctl[C_STATUS] = TLC_ST_BAD_INPUT;
        else {
            // an end outside [-1, 101] (or a NaN): its edge's key may pass the node's own, where the merged order of the reference
            // differs from the edges-only one sorted here -- refused, not answered differently
            const double fu = f[u], fv = f[v];
            if (!(fu >= -1.0 && fu <= 101.0 && fv >= -1.0 && fv <= 101.0)) ctl[C_STATUS] = TLC_ST_BAD_INPUT;
            k = tlc_ord_f64(tlc_key_asc(fu, fv));
        }
        key[e] = k;
        val[e] = (unsigned)e;
    }
}
// ra[e] = r; the descending sort's input in descending ra, so that the stable sort puts the higher ascending rank first
__global__ __launch_bounds__(PDW_BS) void pdw_asc_rank_kernel(const int* __restrict__ ctl, int m, const int* __restrict__ edges,
                                                              const double* __restrict__ f, const unsigned* __restrict__ sorted,
                                                              int* __restrict__ ra, int* __restrict__ aperm,
                                                              unsigned long long* __restrict__ key, unsigned* __restrict__ val) {
    if (ctl[C_STATUS]) return;
    PDW_FOR(r, m) {
        const int e = (int)sorted[r];
        ra[e] = r;
        aperm[r] = e;
        key[m - 1 - r] = ~tlc_ord_f64(tlc_key_desc(f[edges[2 * e]], f[edges[2 * e + 1]]));
        val[m - 1 - r] = (unsigned)e;
    }
}
__global__ __launch_bounds__(PDW_BS) void pdw_desc_rank_kernel(const int* __restrict__ ctl, int m, const unsigned* __restrict__ sorted,
                                                               int* __restrict__ rd, int* __restrict__ dperm) {
    if (ctl[C_STATUS]) return;
    PDW_FOR(t, m) {
        const int e = (int)sorted[t];
        rd[e] = t;
        dperm[t] = e;
    }
}
// the reference's root: first endpoint of its first Neg edge = the edge with the largest desc key, lowest id among equals
__global__ __launch_bounds__(PDW_BS) void pdw_root_kernel(int* __restrict__ ctl, int m, const int* __restrict__ edges,
                                                          const double* __restrict__ f, const int* __restrict__ dperm) {
    if (ctl[C_STATUS]) return;
    const int e0 = dperm[0];
    const unsigned long long k0 = tlc_ord_f64(tlc_key_desc(f[edges[2 * e0]], f[edges[2 * e0 + 1]]));
    PDW_FOR(e, m)
        if (tlc_ord_f64(tlc_key_desc(f[edges[2 * e]], f[edges[2 * e + 1]])) == k0) atomicMin(&ctl[C_MINID], e);
}

// ---- exclusive prefix sum of byte flags -------------------------------------------------------------------------------------
// count = mult * *p_count items in chunks of PDW_SCAN_CHUNK: chunk sums, one workgroup over the sums, then the chunks again.
__global__ __launch_bounds__(PDW_BS) void pdw_scan_sums_kernel(Gate g, const uint8_t* __restrict__ fl, const int* __restrict__ p_count,
                                                               int mult, int* __restrict__ sums) {
    if (closed(g)) return;
    __shared__ BlockScratch<PDW_BS> sh;
    const int count = mult * *p_count, nch = (count + PDW_SCAN_CHUNK - 1) / PDW_SCAN_CHUNK;
    for (int c = blockIdx.x; c < nch; c += gridDim.x) {
        long long v = 0, tot;
        const int i0 = c * PDW_SCAN_CHUNK + threadIdx.x * PDW_SCAN_IPT;
        for (int j = 0; j < PDW_SCAN_IPT; ++j)
            if (i0 + j < count) v += fl[i0 + j];
        block_excl_sum<PDW_BS>(v, sh, &tot);
        if (threadIdx.x == 0) sums[c] = (int)tot;
        __syncthreads();
    }
}
__global__ __launch_bounds__(PDW_BS) void pdw_scan_top_kernel(Gate g, const int* __restrict__ p_count, int mult, int* __restrict__ sums,
                                                              int* __restrict__ total) {
    if (closed(g)) return;
    __shared__ BlockScratch<PDW_BS> sh;
    const int count = mult * *p_count, nch = (count + PDW_SCAN_CHUNK - 1) / PDW_SCAN_CHUNK;
    long long carry = 0;
    for (int c0 = 0; c0 < nch; c0 += PDW_BS) {
        const int c = c0 + threadIdx.x;
        const long long v = c < nch ? sums[c] : 0;
        long long tot;
        const long long ex = block_excl_sum<PDW_BS>(v, sh, &tot);
        if (c < nch) sums[c] = (int)(carry + ex);
        carry += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = (int)carry;
}
__global__ __launch_bounds__(PDW_BS) void pdw_scan_apply_kernel(Gate g, const uint8_t* __restrict__ fl, const int* __restrict__ p_count,
                                                                int mult, const int* __restrict__ sums, int* __restrict__ out) {
    if (closed(g)) return;
    __shared__ BlockScratch<PDW_BS> sh;
    const int count = mult * *p_count, nch = (count + PDW_SCAN_CHUNK - 1) / PDW_SCAN_CHUNK;
    for (int c = blockIdx.x; c < nch; c += gridDim.x) {
        long long v = 0, tot;
        const int i0 = c * PDW_SCAN_CHUNK + threadIdx.x * PDW_SCAN_IPT;
        for (int j = 0; j < PDW_SCAN_IPT; ++j)
            if (i0 + j < count) v += fl[i0 + j];
        int run = sums[c] + (int)block_excl_sum<PDW_BS>(v, sh, &tot);
        for (int j = 0; j < PDW_SCAN_IPT; ++j)
            if (i0 + j < count) {
                out[i0 + j] = run;
                run += fl[i0 + j];
            }
        __syncthreads();
    }
}

// ---- the segmented minimum-spanning-forest primitive ----------------------------------------------------------------------
// Items i < imul * *p_items: (ia[i], ib[i]) in the id space 0 .. nmul * *p_ids - 1, ia[i] < 0: no item; weight iw[i] (NULL: i), unique.
// Out: intree[i]; par[x] = the representative of x's component.  Round r runs only if flag[r] is set (round r-1 hooked something).
struct Msf {
    Gate g;
    const int *ia, *ib;
    const unsigned* iw;
    uint8_t* intree;
    int *par, *hk;
    unsigned long long* best;
    const int *p_items, *p_ids;
    int imul, nmul;
    int* ctl;
};
__global__ __launch_bounds__(PDW_BS) void msf_init_kernel(Msf P) {
    if (closed(P.g)) return;
    const int I = P.imul * *P.p_items, N = P.nmul * *P.p_ids;
    PDW_FOR(x, N) {
        P.par[x] = x;
        P.hk[x] = x;
        P.best[x] = PDW_NOKEY;
    }
    PDW_FOR(i, I) P.intree[i] = 0;
    if (blockIdx.x == 0 && threadIdx.x < 40) P.ctl[C_FLAGS + threadIdx.x] = threadIdx.x == 0;
}
__global__ __launch_bounds__(PDW_BS) void msf_pick_kernel(Msf P, int r) {
    if (closed(P.g) || !P.ctl[C_FLAGS + r]) return;
    const int I = P.imul * *P.p_items;
    PDW_FOR(i, I) {
        const int a = P.ia[i];
        if (a < 0) continue;
        const int ca = P.par[a], cb = P.par[P.ib[i]];
        if (ca == cb) continue;
        const unsigned long long key = ((unsigned long long)(P.iw ? P.iw[i] : (unsigned)i) << 32) | (unsigned)i;
        atomicMin(&P.best[ca], key);
        atomicMin(&P.best[cb], key);
    }
}
__global__ __launch_bounds__(PDW_BS) void msf_hook_kernel(Msf P, int r) {
    if (closed(P.g) || !P.ctl[C_FLAGS + r]) return;
    const int N = P.nmul * *P.p_ids;
    PDW_FOR(x, N) {
        if (P.par[x] != x) continue;
        const unsigned long long b = P.best[x];
        if (b == PDW_NOKEY) continue;
        const int i = (int)(unsigned)b;
        const int ca = P.par[P.ia[i]], cb = P.par[P.ib[i]];
        const int other = ca == x ? cb : ca;
        P.intree[i] = 1;
        if (!(P.best[other] == b && x < other)) P.hk[x] = other;   // of two components that chose the same item, the lower id stays root
        P.ctl[C_FLAGS + r + 1] = 1;
    }
}
// every id to the root of its hook chain.  hk[] is only ever replaced by an ancestor (path halving), so a stale read is still a
// valid step, and the root reached is the same whatever the interleaving.
__global__ __launch_bounds__(PDW_BS) void msf_flat_kernel(Msf P, int r) {
    if (closed(P.g) || !P.ctl[C_FLAGS + r]) return;
    const int N = P.nmul * *P.p_ids;
    if (blockIdx.x == 0 && threadIdx.x == 0) P.ctl[C_ROUNDS] += 1;
    PDW_FOR(x, N) {
        int t = P.par[x];
        for (;;) {
            const int p = __hip_atomic_load(&P.hk[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (p == t) break;
            const int gp = __hip_atomic_load(&P.hk[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (gp == p) { t = p; break; }
            __hip_atomic_store(&P.hk[t], gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            t = gp;
        }
        P.par[x] = t;
        P.best[x] = PDW_NOKEY;
    }
}

// ---- lists ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PDW_BS) void pdw_edge_items_kernel(const int* __restrict__ ctl, int m, const int* __restrict__ edges,
                                                                const uint8_t* __restrict__ keep_a, const uint8_t* __restrict__ keep_b,
                                                                int* __restrict__ ia, int* __restrict__ ib) {
    if (ctl[C_STATUS]) return;
    PDW_FOR(e, m) {
        const bool on = (!keep_a || keep_a[e]) && (!keep_b || keep_b[e]);
        ia[e] = on ? edges[2 * e] : -1;
        ib[e] = edges[2 * e + 1];
    }
}
__global__ __launch_bounds__(PDW_BS) void pdw_copy_kernel(const int* __restrict__ ctl, int n, const int* __restrict__ src, int* __restrict__ dst) {
    if (ctl[C_STATUS]) return;
    PDW_FOR(i, n) dst[i] = src[i];
}
// byte flags in sorted order: Pos (all), queries (Pos edges of the root's component), dying edges of that component; forest edges (asc)
__global__ __launch_bounds__(PDW_BS) void pdw_flags_kernel(const int* __restrict__ ctl, int m, const int* __restrict__ edges,
                                                           const int* __restrict__ aperm, const int* __restrict__ dperm,
                                                           const uint8_t* __restrict__ in_final, const uint8_t* __restrict__ is_neg,
                                                           const int* __restrict__ lab, uint8_t* __restrict__ f_pos, uint8_t* __restrict__ f_q,
                                                           uint8_t* __restrict__ f_dy, uint8_t* __restrict__ f_fin) {
    if (ctl[C_STATUS]) return;
    const int rootc = lab[edges[2 * ctl[C_MINID]]];
    PDW_FOR(t, m) {
        const int e = dperm[t];
        const bool neg = is_neg[e], inroot = lab[edges[2 * e]] == rootc;
        f_pos[t] = !neg;
        f_q[t] = !neg && inroot;
        f_dy[t] = inroot && !in_final[e];
        f_fin[t] = in_final[aperm[t]];
    }
}
__global__ __launch_bounds__(PDW_BS) void pdw_lists_kernel(int* __restrict__ ctl, int m, const int* __restrict__ aperm,
                                                           const int* __restrict__ dperm, const uint8_t* __restrict__ f_pos,
                                                           const uint8_t* __restrict__ f_fin, const int* __restrict__ pos_idx,
                                                           const int* __restrict__ fin_idx, int* __restrict__ t_up, int* __restrict__ t_down) {
    if (ctl[C_STATUS]) return;
    PDW_FOR(t, m) {
        if (f_fin[t]) t_up[fin_idx[t]] = aperm[t];
        if (!f_pos[t]) t_down[t - pos_idx[t]] = dperm[t];
    }
}

// ---- the two elder-rule passes and ext0 -------------------------------------------------------------------------------------
__device__ __forceinline__ int uf_find(int* comp, int p) {
    while (p != comp[p]) {
        comp[p] = comp[comp[p]];
        p = comp[p];
    }
    return p;
}
// one pass: the forest's edges in sorted order, walked by one lane; comp points into LDS or into global memory
__device__ __forceinline__ void elder_pass(int* __restrict__ ctl, int n, int m, const int* __restrict__ edges, const double* __restrict__ f,
                                           int keep0, bool up, const int* __restrict__ list, int* comp, double* __restrict__ out) {
    for (int i = threadIdx.x; i < n; i += PDW_BS) comp[i] = i;
    __syncthreads();
    if (threadIdx.x != 0) return;
    const int nt = up ? ctl[C_NFIN] : m - ctl[C_NPOS];
    int cnt = 0;
    for (int i = 0; i < nt; ++i) {
        const int e = list[i], u = edges[2 * e], v = edges[2 * e + 1];
        const int pu = uf_find(comp, u), pv = uf_find(comp, v);
        if (pu == pv) continue;
        const int small = f[pu] <= f[pv] ? pu : pv, large = pu + pv - small;      // :63-64, :101-102
        if (up) {
            const int max_node = f[u] > f[v] ? u : v;                               // :65
            if (keep0 || f[large] < f[max_node]) { out[2 * cnt] = f[large]; out[2 * cnt + 1] = f[max_node]; ++cnt; }
            comp[large] = small;
        } else {
            const int min_node = f[u] < f[v] ? u : v;                               // :103-104
            if (keep0 || f[small] > f[min_node]) { out[2 * cnt] = f[small]; out[2 * cnt + 1] = f[min_node]; ++cnt; }
            comp[small] = large;
        }
    }
    ctl[up ? C_NUP : C_NDOWN] = cnt;
}
// workgroup 0: ascending pass (:46-68), 1: descending pass (:83-109), 2: ext0.  One lane walks a pass: the forest's edges in sorted order.
__global__ __launch_bounds__(PDW_BS) void pdw_passes_kernel(int* __restrict__ ctl, int n, int m, const int* __restrict__ edges,
                                                            const double* __restrict__ f, int keep0, const int* __restrict__ t_up,
                                                            const int* __restrict__ t_down, int* __restrict__ comp_up,
                                                            int* __restrict__ comp_down, double* __restrict__ pd_up,
                                                            double* __restrict__ pd_down, double* __restrict__ ext0) {
    if (ctl[C_STATUS]) return;
    if (blockIdx.x == 2) {
        __shared__ double smn[PDW_BS / 64], smx[PDW_BS / 64];
        double mn = 99999999, mx = -99999999;                 // :28-38
        for (int i = threadIdx.x; i < n; i += PDW_BS) {
            const double v = f[i];
            if (mn > v) mn = v;
            if (mx < v) mx = v;
        }
        mn = tlc_wave_min_f64(mn);
        mx = tlc_wave_max_f64(mx);
        if ((threadIdx.x & 63) == 0) { smn[threadIdx.x >> 6] = mn; smx[threadIdx.x >> 6] = mx; }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < PDW_BS / 64; ++w) {
                if (mn > smn[w]) mn = smn[w];
                if (mx < smx[w]) mx = smx[w];
            }
            ext0[0] = mn;
            ext0[1] = mx;
        }
        return;
    }
    // comp[] in LDS where the graph fits (one workgroup per pass, so the whole LDS is this pass's), in global memory (L2) otherwise
    __shared__ int lcomp[PDW_LDS_NODES];
    const bool up = blockIdx.x == 0;
    if (n <= PDW_LDS_NODES) elder_pass(ctl, n, m, edges, f, keep0, up, up ? t_up : t_down, lcomp, up ? pd_up : pd_down);
    else elder_pass(ctl, n, m, edges, f, keep0, up, up ? t_up : t_down, up ? comp_up : comp_down, up ? pd_up : pd_down);
}

// ---- the divide and conquer over the insertion order ------------------------------------------------------------------------
struct Dc {
    int *pa, *pb, *pseg, *pe, *qofp;       // P slot d: supernode ends, segment (-1: not spawned), edge, its query (-1: a Neg edge)
    unsigned *pw, *qw;                     // ascending ranks
    int *qa, *qb, *qseg, *qe;              // Q slot k
    uint8_t* qalive;                       // alive at the end of its segment
    int *cnt, *rem, *rem_e;
    uint8_t *tmid, *used;
    int *ren, *par, *ia, *ib;
    unsigned* iw;
    int* ctl;
};
__device__ __forceinline__ int seg_bound(int level, int j, int K) { return (int)(((long long)j * K) >> level); }

__global__ __launch_bounds__(PDW_BS) void dc_init_kernel(Dc D, int n, int m, int force, const int* __restrict__ edges,
                                                         const int* __restrict__ dperm, const int* __restrict__ ra,
                                                         const uint8_t* __restrict__ in_final, const uint8_t* __restrict__ f_pos,
                                                         const uint8_t* __restrict__ f_q, const uint8_t* __restrict__ f_dy,
                                                         const int* __restrict__ q_idx, const int* __restrict__ d_idx) {
    int* ctl = D.ctl;
    if (ctl[C_STATUS]) return;
    const int K = ctl[C_K];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        int levels = 0;
        while (levels < 31 && (1ll << levels) < K) ++levels;
        const bool fail = ctl[C_NDY] != K || force;
        ctl[C_FAIL] = fail;
        ctl[C_LEVELS] = fail ? 0 : levels;
        ctl[C_NS] = n;
        ctl[C_TWOK] = 2 * K;
    }
    PDW_FOR(t, m) {
        const int e = dperm[t], a = D.par[edges[2 * e]], b = D.par[edges[2 * e + 1]];
        const int k = q_idx[t];
        if (f_q[t]) {
            D.qa[k] = a; D.qb[k] = b; D.qalive[k] = in_final[e]; D.qseg[k] = 0; D.qw[k] = (unsigned)ra[e]; D.qe[k] = e;
            D.cnt[k] = 0; D.rem[k] = 0; D.rem_e[k] = -1;
        }
        if (f_dy[t]) {
            const int d = d_idx[t];
            if (d < K) {
                D.pe[d] = e; D.pw[d] = (unsigned)ra[e]; D.qofp[d] = f_q[t] ? k : -1;
                D.pa[d] = a; D.pb[d] = b; D.pseg[d] = f_pos[t] ? -1 : 0;
            }
        }
    }
}
// T_mid's items: the live P slots, and the queries of each segment's left half
__global__ __launch_bounds__(PDW_BS) void dc_items_kernel(Dc D, int lv) {
    const int* ctl = D.ctl;
    if (ctl[C_STATUS] || lv >= ctl[C_LEVELS]) return;
    const int K = ctl[C_K];
    PDW_FOR(i, 2 * K) {
        if (i < K) {
            D.ia[i] = D.pseg[i] >= 0 ? D.pa[i] : -1; D.ib[i] = D.pb[i]; D.iw[i] = D.pw[i];
        } else {
            const int k = i - K, mid = seg_bound(lv + 1, 2 * D.qseg[k] + 1, K);
            D.ia[i] = k < mid ? D.qa[k] : -1; D.ib[i] = D.qb[k]; D.iw[i] = D.qw[k];
        }
    }
}
// the contraction sets in a doubled id space: left child's (P in T_mid) on x, right child's (left-half Q in T_mid, alive at r) on x + ns
__global__ __launch_bounds__(PDW_BS) void dc_contract_kernel(Dc D, int lv) {
    const int* ctl = D.ctl;
    if (ctl[C_STATUS] || lv >= ctl[C_LEVELS]) return;
    const int K = ctl[C_K], ns = ctl[C_NS + lv];
    PDW_FOR(i, 2 * K) {
        if (i < K) {
            D.ia[i] = (D.pseg[i] >= 0 && D.tmid[i]) ? D.pa[i] : -1; D.ib[i] = D.pb[i];
        } else {
            const int k = i - K, mid = seg_bound(lv + 1, 2 * D.qseg[k] + 1, K);
            D.ia[i] = (k < mid && D.tmid[i] && D.qalive[k]) ? D.qa[k] + ns : -1; D.ib[i] = D.qb[k] + ns;
        }
    }
    PDW_FOR(x, 2 * ns) D.used[x] = 0;
}
// P slots: T_mid members live on in the right child, the others die in the left one; a left-half query that is in T_mid and
// dead at r spawns its P slot in the right child.  Reads the Q slots, which dc_route_q_kernel rewrites afterwards.
__global__ __launch_bounds__(PDW_BS) void dc_route_p_kernel(Dc D, int lv) {
    const int* ctl = D.ctl;
    if (ctl[C_STATUS] || lv >= ctl[C_LEVELS]) return;
    const int K = ctl[C_K], ns = ctl[C_NS + lv];
    PDW_FOR(d, K) {
        int a, b;
        if (D.pseg[d] >= 0) {
            const int j = D.pseg[d], sh = D.tmid[d] ? ns : 0;
            D.pseg[d] = 2 * j + (sh ? 1 : 0);
            a = D.par[D.pa[d] + sh]; b = D.par[D.pb[d] + sh];
        } else {
            const int k = D.qofp[d];
            if (k < 0) continue;
            const int j = D.qseg[k], mid = seg_bound(lv + 1, 2 * j + 1, K);
            if (!(k < mid && D.tmid[K + k] && !D.qalive[k])) continue;
            D.pseg[d] = 2 * j + 1;
            a = D.par[D.qa[k] + ns]; b = D.par[D.qb[k] + ns];
        }
        D.pa[d] = a; D.pb[d] = b;
        D.used[a] = 1; D.used[b] = 1;
    }
}
__global__ __launch_bounds__(PDW_BS) void dc_route_q_kernel(Dc D, int lv) {
    const int* ctl = D.ctl;
    if (ctl[C_STATUS] || lv >= ctl[C_LEVELS]) return;
    const int K = ctl[C_K], ns = ctl[C_NS + lv];
    PDW_FOR(k, K) {
        const int j = D.qseg[k], mid = seg_bound(lv + 1, 2 * j + 1, K);
        int sh = ns;
        if (k < mid) {
            D.qalive[k] = D.tmid[K + k];
            sh = 0;
        }
        D.qseg[k] = 2 * j + (sh ? 1 : 0);
        const int a = D.par[D.qa[k] + sh], b = D.par[D.qb[k] + sh];
        D.qa[k] = a; D.qb[k] = b;
        D.used[a] = 1; D.used[b] = 1;
    }
}
__global__ __launch_bounds__(PDW_BS) void dc_renumber_kernel(Dc D, int lv) {
    const int* ctl = D.ctl;
    if (ctl[C_STATUS] || lv >= ctl[C_LEVELS]) return;
    const int K = ctl[C_K];
    PDW_FOR(i, K) {
        if (D.pseg[i] >= 0) { D.pa[i] = D.ren[D.pa[i]]; D.pb[i] = D.ren[D.pb[i]]; }
        D.qa[i] = D.ren[D.qa[i]]; D.qb[i] = D.ren[D.qb[i]];
    }
}
// the end checks of ext1_dc.h: every P slot sits in a one-query segment, every query owns exactly one, heavier than itself
__global__ __launch_bounds__(PDW_BS) void dc_finish_a_kernel(Dc D) {
    int* ctl = D.ctl;
    if (ctl[C_STATUS] || ctl[C_FAIL]) return;
    const int K = ctl[C_K], L = ctl[C_LEVELS];
    PDW_FOR(d, K) {
        const int s = D.pseg[d];
        const int k = s < 0 ? -1 : seg_bound(L, s, K);
        if (s < 0 || k >= K || seg_bound(L, s + 1, K) - k != 1) { ctl[C_FAIL] = 1; continue; }
        atomicAdd(&D.cnt[k], 1);
        D.rem[k] = d;
    }
}
__global__ __launch_bounds__(PDW_BS) void dc_finish_b_kernel(Dc D) {
    int* ctl = D.ctl;
    if (ctl[C_STATUS]) return;
    const int K = ctl[C_K];
    PDW_FOR(k, K) {
        const int d = D.rem[k];
        if (D.cnt[k] != 1 || D.pw[d] <= D.qw[k]) ctl[C_FAIL] = 1;
        else D.rem_e[k] = D.pe[d];
    }
}

// ---- exact fallback: the reference's serial swap (:115-178), one lane, 32-bit ids in global memory -------------------------
__global__ __launch_bounds__(PDW_BS) void pdw_fallback_kernel(int* __restrict__ ctl, int n, int m, const int* __restrict__ edges,
                                                              const double* __restrict__ f, const uint8_t* __restrict__ is_neg,
                                                              const int* __restrict__ qe, int* __restrict__ rem_e,
                                                              int* __restrict__ parent, int* __restrict__ pedge, int* __restrict__ mark,
                                                              int* __restrict__ queue, int* __restrict__ adjptr, int* __restrict__ adjidx) {
    if (ctl[C_STATUS] || !ctl[C_FAIL]) return;
    for (int i = threadIdx.x; i < n; i += PDW_BS) { parent[i] = -1; pedge[i] = -1; mark[i] = -1; adjptr[i] = 0; }
    if (threadIdx.x == 0) { adjptr[n] = 0; adjptr[n + 1] = 0; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    ctl[C_FELL] = 1;
    const int K = ctl[C_K];
    if (K == 0) return;
    for (int e = 0; e < m; ++e)
        if (is_neg[e]) { adjptr[edges[2 * e] + 1]++; adjptr[edges[2 * e + 1] + 1]++; }
    for (int i = 0; i < n; ++i) adjptr[i + 1] += adjptr[i];
    for (int i = 0; i < n; ++i) queue[i] = adjptr[i];
    for (int e = 0; e < m; ++e)
        if (is_neg[e]) { adjidx[queue[edges[2 * e]]++] = e; adjidx[queue[edges[2 * e + 1]]++] = e; }
    const int root = edges[2 * ctl[C_MINID]];
    parent[root] = root;
    int qh = 0, qt = 0;
    queue[qt++] = root;
    while (qh < qt) {
        const int a = queue[qh++];
        for (int j = adjptr[a]; j < adjptr[a + 1]; ++j) {
            const int e = adjidx[j], b = edges[2 * e] == a ? edges[2 * e + 1] : edges[2 * e];
            if (parent[b] < 0) { parent[b] = a; pedge[b] = e; queue[qt++] = b; }
        }
    }
    for (int pi = 0; pi < K; ++pi) {
        const int e = qe[pi], p = edges[2 * e], q = edges[2 * e + 1];
        rem_e[pi] = -1;
        if (parent[p] < 0 || parent[q] < 0) continue;
        for (int a = p; a != root; a = parent[a]) mark[a] = pi;
        int meet = root;
        for (int a = q; a != root; a = parent[a])
            if (mark[a] == pi) { meet = a; break; }
        int best = -1, side = 0;
        double best_val = 0;
        for (int a = p; a != meet; a = parent[a]) {
            const int t = pedge[a];
            const double val = tlc_key_asc(f[edges[2 * t]], f[edges[2 * t + 1]]);
            if (best < 0 || val > best_val) { best = a; best_val = val; side = 0; }
        }
        for (int a = q; a != meet; a = parent[a]) {
            const int t = pedge[a];
            const double val = tlc_key_asc(f[edges[2 * t]], f[edges[2 * t + 1]]);
            if (best < 0 || val > best_val) { best = a; best_val = val; side = 1; }
        }
        if (best < 0) continue;
        rem_e[pi] = pedge[best];
        int node = side == 0 ? p : q, nodec = side == 0 ? q : p, e_in = e;
        while (nodec != best) {
            const int tp = parent[node], te = pedge[node];
            parent[node] = nodec; pedge[node] = e_in;
            nodec = node; node = tp; e_in = te;
        }
    }
}

// ---- Ext1 points and the graph's row ------------------------------------------------------------------------------------------
__device__ __forceinline__ void ext1_point(const int* edges, const double* f, int e, int le, double* lo, double* hi) {
    const double fa = f[edges[2 * le]], fb = f[edges[2 * le + 1]], fp = f[edges[2 * e]], fq = f[edges[2 * e + 1]];
    *hi = fa > fb ? fa : fb;                                                      // :160
    *lo = fp < fq ? fp : fq;                                                      // :162
}
__global__ __launch_bounds__(PDW_BS) void pdw_point_flags_kernel(const int* __restrict__ ctl, const int* __restrict__ edges,
                                                                 const double* __restrict__ f, int keep0, const int* __restrict__ qe,
                                                                 const int* __restrict__ rem_e, uint8_t* __restrict__ fl) {
    if (ctl[C_STATUS]) return;
    PDW_FOR(k, ctl[C_K]) {
        double lo, hi;
        const int le = rem_e[k];
        if (le < 0) { fl[k] = 0; continue; }
        ext1_point(edges, f, qe[k], le, &lo, &hi);
        fl[k] = keep0 || hi > lo;                                                 // :164
    }
}
__global__ __launch_bounds__(PDW_BS) void pdw_point_write_kernel(const int* __restrict__ ctl, const int* __restrict__ edges,
                                                                 const double* __restrict__ f, const int* __restrict__ qe,
                                                                 const int* __restrict__ rem_e, const uint8_t* __restrict__ fl,
                                                                 const int* __restrict__ idx, double* __restrict__ pd_one) {
    if (ctl[C_STATUS]) return;
    PDW_FOR(k, ctl[C_K]) {
        if (!fl[k]) continue;
        double lo, hi;
        ext1_point(edges, f, qe[k], rem_e[k], &lo, &hi);
        pd_one[2 * idx[k]] = lo;
        pd_one[2 * idx[k] + 1] = hi;
    }
}
__global__ __launch_bounds__(PDW_BS) void pdw_row_kernel(const int* __restrict__ ctl, int n, int m, int ext1, const int* __restrict__ dperm,
                                                         const uint8_t* __restrict__ f_pos, const int* __restrict__ pos_idx,
                                                         int* __restrict__ counts, int* __restrict__ edge_rank) {
    if (ctl[C_STATUS]) {
        if (blockIdx.x == 0 && threadIdx.x < 4) counts[threadIdx.x] = TLC_PD_WIDE_BAD_INPUT_ROW;
        return;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        counts[0] = ctl[C_NUP];
        counts[1] = ctl[C_NDOWN];
        counts[2] = ext1 ? ctl[C_NONE] : 0;
        counts[3] = n - (m - ctl[C_NPOS]);
    }
    if (edge_rank)
        PDW_FOR(t, m) edge_rank[dperm[t]] = f_pos[t] ? pos_idx[t] : -(t - pos_idx[t]) - 1;
}
__global__ void pdw_bad_row_kernel(int* __restrict__ counts) {
    if (threadIdx.x < 4) counts[threadIdx.x] = TLC_PD_WIDE_BAD_INPUT_ROW;
}

// ---- workspace ----------------------------------------------------------------------------------------------------------------
struct Lay {
    size_t ctl, key_a, key_b, val_a, val_b, hist, tot, ra, rd, aperm, dperm, in_final, is_neg, tmid, tree2, f_pos, f_q, f_dy, f_fin, f_pt,
        pos_idx, q_idx, d_idx, fin_idx, pt_idx, used, ren, sums, t_up, t_down, comp_up, comp_down, lab, par, hk, best, ia, ib, iw, pa, pb,
        pseg, pe, qofp, pw, qw, qa, qb, qseg, qe, qalive, cnt, rem, rem_e, fb, bytes;
    long long idcap;
};
Lay layout(long long n, long long m) {
    Lay L;
    TlcCarver W;
    const long long idcap = n > 4 * m + 4 ? n : 4 * m + 4, n2 = 2 * idcap;
    L.idcap = idcap;
    L.ctl = W.take(C_INTS, 4);
    L.key_a = W.take(m, 8); L.key_b = W.take(m, 8); L.val_a = W.take(m, 4); L.val_b = W.take(m, 4);
    L.hist = W.take(rk_hist_ints(m), 4); L.tot = W.take(RK_TOT_INTS, 4);
    L.ra = W.take(m, 4); L.rd = W.take(m, 4); L.aperm = W.take(m, 4); L.dperm = W.take(m, 4);
    L.in_final = W.take(m, 1); L.is_neg = W.take(m, 1); L.tmid = W.take(2 * m, 1); L.tree2 = W.take(2 * m, 1);
    L.f_pos = W.take(m, 1); L.f_q = W.take(m, 1); L.f_dy = W.take(m, 1); L.f_fin = W.take(m, 1); L.f_pt = W.take(m, 1);
    L.pos_idx = W.take(m, 4); L.q_idx = W.take(m, 4); L.d_idx = W.take(m, 4); L.fin_idx = W.take(m, 4); L.pt_idx = W.take(m, 4);
    L.used = W.take(n2, 1); L.ren = W.take(n2, 4);
    L.sums = W.take((n2 > m ? n2 : m) / PDW_SCAN_CHUNK + 2, 4);
    L.t_up = W.take(n, 4); L.t_down = W.take(n, 4); L.comp_up = W.take(n, 4); L.comp_down = W.take(n, 4); L.lab = W.take(n, 4);
    L.par = W.take(n2, 4); L.hk = W.take(n2, 4); L.best = W.take(n2, 8);
    L.ia = W.take(2 * m, 4); L.ib = W.take(2 * m, 4); L.iw = W.take(2 * m, 4);
    L.pa = W.take(m, 4); L.pb = W.take(m, 4); L.pseg = W.take(m, 4); L.pe = W.take(m, 4); L.qofp = W.take(m, 4);
    L.pw = W.take(m, 4); L.qw = W.take(m, 4);
    L.qa = W.take(m, 4); L.qb = W.take(m, 4); L.qseg = W.take(m, 4); L.qe = W.take(m, 4); L.qalive = W.take(m, 1);
    L.cnt = W.take(m, 4); L.rem = W.take(m, 4); L.rem_e = W.take(m, 4);
    L.fb = W.take(7 * n + 8, 4);
    L.bytes = W.bytes();
    return L;
}

int ceil_log2(long long v) {
    int l = 0;
    while ((1ll << l) < v) ++l;
    return l;
}
unsigned pdw_grid(long long count) { return tlc_grid_for(count, PDW_BS, PDW_MAX_GRID); }

struct Run {
    hipStream_t s;
    long long launches;
};
#define PDW_LAUNCH(R, kernel, grid, ...)                                                       \
    do {                                                                                       \
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(PDW_BS), 0, (R).s, __VA_ARGS__);           \
        (R).launches += 1;                                                                     \
    } while (0)

void scan_flags(Run& R, Gate g, const uint8_t* fl, const int* p_count, int mult, long long bound, int* sums, int* out, int* total) {
    const unsigned grid = pdw_grid((bound + PDW_SCAN_IPT - 1) / PDW_SCAN_IPT);
    PDW_LAUNCH(R, pdw_scan_sums_kernel, grid, g, fl, p_count, mult, sums);
    PDW_LAUNCH(R, pdw_scan_top_kernel, 1, g, p_count, mult, sums, total);
    PDW_LAUNCH(R, pdw_scan_apply_kernel, grid, g, fl, p_count, mult, sums, out);
}
// id_bound / item_bound: what the host knows of the sizes; the device's own counts decide what runs
void msf(Run& R, const Msf& P, long long id_bound, long long item_bound) {
    const long long v = id_bound < 2 * item_bound ? id_bound : 2 * item_bound;   // components that have an item
    const int rounds = v < 2 ? 1 : ceil_log2(v) > 32 ? 32 : ceil_log2(v);
    const unsigned gi = pdw_grid(item_bound), gn = pdw_grid(id_bound);
    PDW_LAUNCH(R, msf_init_kernel, gn > gi ? gn : gi, P);
    for (int r = 0; r < rounds; ++r) {
        PDW_LAUNCH(R, msf_pick_kernel, gi, P, r);
        PDW_LAUNCH(R, msf_hook_kernel, gn, P, r);
        PDW_LAUNCH(R, msf_flat_kernel, gn, P, r);
    }
}

int run_graph(Run& R, char* w, const Lay& L, int n, int m, const int* edges, const double* f, uint32_t flags, double* pd_up,
              double* pd_down, double* pd_one, double* ext0, int* counts, int* edge_rank, int* h_levels_bound) {
    int* ctl = (int*)(w + L.ctl);
    unsigned long long *key_a = (unsigned long long*)(w + L.key_a), *key_b = (unsigned long long*)(w + L.key_b);
    unsigned *val_a = (unsigned*)(w + L.val_a), *val_b = (unsigned*)(w + L.val_b);
    int *hist = (int*)(w + L.hist), *tot = (int*)(w + L.tot), *ra = (int*)(w + L.ra), *rd = (int*)(w + L.rd);
    int *aperm = (int*)(w + L.aperm), *dperm = (int*)(w + L.dperm);
    uint8_t *in_final = (uint8_t*)(w + L.in_final), *is_neg = (uint8_t*)(w + L.is_neg), *tmid = (uint8_t*)(w + L.tmid);
    uint8_t *tree2 = (uint8_t*)(w + L.tree2), *f_pos = (uint8_t*)(w + L.f_pos), *f_q = (uint8_t*)(w + L.f_q);
    uint8_t *f_dy = (uint8_t*)(w + L.f_dy), *f_fin = (uint8_t*)(w + L.f_fin), *f_pt = (uint8_t*)(w + L.f_pt);
    int *pos_idx = (int*)(w + L.pos_idx), *q_idx = (int*)(w + L.q_idx), *d_idx = (int*)(w + L.d_idx), *fin_idx = (int*)(w + L.fin_idx);
    int *pt_idx = (int*)(w + L.pt_idx), *sums = (int*)(w + L.sums), *t_up = (int*)(w + L.t_up), *t_down = (int*)(w + L.t_down);
    int *comp_up = (int*)(w + L.comp_up), *comp_down = (int*)(w + L.comp_down), *lab = (int*)(w + L.lab);
    int *par = (int*)(w + L.par), *hk = (int*)(w + L.hk), *ia = (int*)(w + L.ia), *ib = (int*)(w + L.ib), *fb = (int*)(w + L.fb);
    unsigned long long* best = (unsigned long long*)(w + L.best);
    const Gate open{ctl, -1};
    const int keep0 = (flags & TLC_KEEP_ZERO_PERS) != 0, ext1 = !(flags & TLC_NO_EXT1);
    const unsigned gm = pdw_grid(m), gn = pdw_grid(n);

    PDW_LAUNCH(R, pdw_ctl_kernel, 1, ctl, n, m);
    *h_levels_bound = 0;

    if (m > 0) {
        PDW_LAUNCH(R, pdw_keys_kernel, gm, ctl, n, m, edges, f, key_a, val_a);
        R.launches += rk_sort<64>(R.s, m, key_a, key_b, val_a, val_b, hist, tot);
        PDW_LAUNCH(R, pdw_asc_rank_kernel, gm, ctl, m, edges, f, val_a, ra, aperm, key_b, val_b);
        R.launches += rk_sort<64>(R.s, m, key_b, key_a, val_b, val_a, hist, tot);
        PDW_LAUNCH(R, pdw_desc_rank_kernel, gm, ctl, m, val_b, rd, dperm);
        PDW_LAUNCH(R, pdw_root_kernel, gm, ctl, m, edges, f, dperm);
        // the two forests of the whole graph
        PDW_LAUNCH(R, pdw_edge_items_kernel, gm, ctl, m, edges, (const uint8_t*)nullptr, (const uint8_t*)nullptr, ia, ib);
        Msf P{open, ia, ib, (const unsigned*)ra, in_final, par, hk, best, ctl + C_M, ctl + C_N, 1, 1, ctl};
        msf(R, P, n, m);
        P.iw = (const unsigned*)rd; P.intree = is_neg;
        msf(R, P, n, m);
        PDW_LAUNCH(R, pdw_copy_kernel, gn, ctl, n, par, lab);
        PDW_LAUNCH(R, pdw_flags_kernel, gm, ctl, m, edges, aperm, dperm, in_final, is_neg, lab, f_pos, f_q, f_dy, f_fin);
        scan_flags(R, open, f_pos, ctl + C_M, 1, m, sums, pos_idx, ctl + C_NPOS);
        scan_flags(R, open, f_fin, ctl + C_M, 1, m, sums, fin_idx, ctl + C_NFIN);
        PDW_LAUNCH(R, pdw_lists_kernel, gm, ctl, m, aperm, dperm, f_pos, f_fin, pos_idx, fin_idx, t_up, t_down);
    }
    PDW_LAUNCH(R, pdw_passes_kernel, 3, ctl, n, m, edges, f, keep0, t_up, t_down, comp_up, comp_down, pd_up, pd_down, ext0);

    if (ext1 && m > 0) {
        scan_flags(R, open, f_q, ctl + C_M, 1, m, sums, q_idx, ctl + C_K);
        scan_flags(R, open, f_dy, ctl + C_M, 1, m, sums, d_idx, ctl + C_NDY);
        // the root segment's supernodes: components of the Neg edges that are never removed
        PDW_LAUNCH(R, pdw_edge_items_kernel, gm, ctl, m, edges, in_final, is_neg, ia, ib);
        Msf P{open, ia, ib, nullptr, tree2, par, hk, best, ctl + C_M, ctl + C_N, 1, 1, ctl};
        msf(R, P, n, m);
        Dc D;
        D.pa = (int*)(w + L.pa); D.pb = (int*)(w + L.pb); D.pseg = (int*)(w + L.pseg); D.pe = (int*)(w + L.pe); D.qofp = (int*)(w + L.qofp);
        D.pw = (unsigned*)(w + L.pw); D.qw = (unsigned*)(w + L.qw);
        D.qa = (int*)(w + L.qa); D.qb = (int*)(w + L.qb); D.qseg = (int*)(w + L.qseg); D.qe = (int*)(w + L.qe);
        D.qalive = (uint8_t*)(w + L.qalive);
        D.cnt = (int*)(w + L.cnt); D.rem = (int*)(w + L.rem); D.rem_e = (int*)(w + L.rem_e);
        D.tmid = tmid; D.used = (uint8_t*)(w + L.used); D.ren = (int*)(w + L.ren); D.par = par; D.ia = ia; D.ib = ib;
        D.iw = (unsigned*)(w + L.iw); D.ctl = ctl;
        PDW_LAUNCH(R, dc_init_kernel, gm, D, n, m, (int)((flags & TLC_PD_WIDE_FORCE_FALLBACK) != 0), edges, dperm, ra, in_final, f_pos, f_q,
                   f_dy, q_idx, d_idx);
        const int levels = (flags & TLC_PD_WIDE_FORCE_FALLBACK) ? 0 : ceil_log2(m);      // K <= m
        *h_levels_bound = levels;
        const unsigned gk = pdw_grid(2ll * m);
        for (int lv = 0; lv < levels; ++lv) {
            const Gate g{ctl, lv};
            const long long ids = lv == 0 ? n : (4ll * m + 4 < L.idcap ? 4ll * m + 4 : L.idcap);
            PDW_LAUNCH(R, dc_items_kernel, gk, D, lv);
            Msf T{g, ia, ib, D.iw, tmid, par, hk, best, ctl + C_TWOK, ctl + C_NS + lv, 1, 1, ctl};
            msf(R, T, ids, 2ll * m);
            PDW_LAUNCH(R, dc_contract_kernel, pdw_grid(2 * ids > 2ll * m ? 2 * ids : 2ll * m), D, lv);
            Msf C{g, ia, ib, nullptr, tree2, par, hk, best, ctl + C_TWOK, ctl + C_NS + lv, 1, 2, ctl};
            msf(R, C, 2 * ids, 2ll * m);
            PDW_LAUNCH(R, dc_route_p_kernel, gm, D, lv);
            PDW_LAUNCH(R, dc_route_q_kernel, gm, D, lv);
            scan_flags(R, g, D.used, ctl + C_NS + lv, 2, 2 * ids, sums, D.ren, ctl + C_NS + lv + 1);
            PDW_LAUNCH(R, dc_renumber_kernel, gm, D, lv);
        }
        PDW_LAUNCH(R, dc_finish_a_kernel, gm, D);
        PDW_LAUNCH(R, dc_finish_b_kernel, gm, D);
        PDW_LAUNCH(R, pdw_fallback_kernel, 1, ctl, n, m, edges, f, is_neg, D.qe, D.rem_e, fb, fb + n, fb + 2 * (size_t)n, fb + 3 * (size_t)n,
                   fb + 4 * (size_t)n, fb + 5 * (size_t)n + 2);
        PDW_LAUNCH(R, pdw_point_flags_kernel, gm, ctl, edges, f, keep0, D.qe, D.rem_e, f_pt);
        scan_flags(R, open, f_pt, ctl + C_K, 1, m, sums, pt_idx, ctl + C_NONE);
        PDW_LAUNCH(R, pdw_point_write_kernel, gm, ctl, edges, f, D.qe, D.rem_e, f_pt, pt_idx, pd_one);
    }
    PDW_LAUNCH(R, pdw_row_kernel, edge_rank ? gm : 1u, ctl, n, m, ext1, dperm, f_pos, pos_idx, counts, edge_rank);
    TLC_HIP_CHECK(hipGetLastError());
    return TLC_OK;
}

}  // namespace

extern "C" int tlc_pd_wide_work_bytes(const int64_t* h_sel_nodes, const int64_t* h_sel_edges, int64_t n_sel, int64_t* bytes) {
    TLC_REQUIRE(bytes, "null pointer");
    TLC_REQUIRE(n_sel >= 0 && n_sel < (1ll << 31), "bad sizes");
    TLC_REQUIRE(n_sel == 0 || (h_sel_nodes && h_sel_edges), "null pointer");
    int64_t mx = 0;
    for (int64_t i = 0; i < n_sel; ++i) {
        TLC_REQUIRE(h_sel_nodes[i] >= 0 && h_sel_edges[i] >= 0, "negative size");
        if (h_sel_nodes[i] > TLC_PD_WIDE_MAX_ITEMS || h_sel_edges[i] > TLC_PD_WIDE_MAX_ITEMS ||
            h_sel_nodes[i] + h_sel_edges[i] > TLC_PD_WIDE_MAX_ITEMS) {
            tlc_set_error("%s: a graph of %lld nodes and %lld edges: n + m is above TLC_PD_WIDE_MAX_ITEMS", __func__,
                          (long long)h_sel_nodes[i], (long long)h_sel_edges[i]);
            return TLC_ERR_UNSUPPORTED;
        }
        const int64_t b = (int64_t)layout(h_sel_nodes[i], h_sel_edges[i]).bytes;
        mx = b > mx ? b : mx;
    }
    *bytes = mx;
    return TLC_OK;
}

extern "C" int tlc_pd_wide(int64_t n_graphs, const int64_t* d_node_offs, const int64_t* d_edge_offs, const int32_t* d_edges, const double* d_f,
                           uint32_t flags, const int64_t* h_sel, int64_t n_sel, double* d_pd_up, double* d_pd_down, double* d_pd_one,
                           double* d_ext0, int32_t* d_counts, int32_t* d_edge_rank, void* d_work, int64_t work_bytes, int64_t* h_stats,
                           void* stream) {
    TLC_REQUIRE(n_graphs >= 0 && n_graphs < (1ll << 31), "bad sizes");
    TLC_REQUIRE(n_sel >= 0 && n_sel < (1ll << 31) && work_bytes >= 0, "bad sizes");
    TLC_REQUIRE((flags & ~(TLC_KEEP_ZERO_PERS | TLC_NO_EXT1 | TLC_PD_WIDE_FORCE_FALLBACK)) == 0, "unknown flag");
    TLC_REQUIRE(n_sel == 0 || h_sel, "null pointer");
    for (int64_t i = 0; i < n_sel; ++i) TLC_REQUIRE(h_sel[i] >= 0 && h_sel[i] < n_graphs, "h_sel outside 0 .. n_graphs-1");
    if (h_stats) memset(h_stats, 0, TLC_PD_WIDE_N_STATS * sizeof(int64_t));
    if (n_sel == 0) return TLC_OK;
    TLC_REQUIRE(d_node_offs && d_edge_offs && d_f && d_pd_up && d_pd_down && d_pd_one && d_ext0 && d_counts && d_work, "null pointer");
    const int64_t least = (int64_t)layout(1, 0).bytes;
    if (work_bytes < least) {
        tlc_set_error("%s: d_work holds %lld bytes; the smallest graph needs %lld (tlc_pd_wide_work_bytes)", __func__, (long long)work_bytes,
                      (long long)least);
        return TLC_ERR_INVALID_ARG;
    }
    Run R{(hipStream_t)stream, 0};
    // sizes of the selected graphs: the call's one read-back before the work starts
    int64_t* offs = (int64_t*)malloc((size_t)n_sel * 4 * sizeof(int64_t));
    if (!offs) return TLC_ERR_OUT_OF_MEMORY;
    int rc = TLC_OK;
    for (int64_t i = 0; i < n_sel && rc == TLC_OK; ++i) {
        if (hipMemcpyAsync(offs + 4 * i, d_node_offs + h_sel[i], 2 * sizeof(int64_t), hipMemcpyDeviceToHost, R.s) != hipSuccess ||
            hipMemcpyAsync(offs + 4 * i + 2, d_edge_offs + h_sel[i], 2 * sizeof(int64_t), hipMemcpyDeviceToHost, R.s) != hipSuccess)
            rc = TLC_ERR_HIP;
    }
    if (rc == TLC_OK && hipStreamSynchronize(R.s) != hipSuccess) rc = TLC_ERR_HIP;
    if (rc != TLC_OK) {
        tlc_set_error("%s: reading the offsets failed", __func__);
        free(offs);
        return rc;
    }
    for (int64_t i = 0; i < n_sel; ++i) {
        const int64_t n = offs[4 * i + 1] - offs[4 * i], m = offs[4 * i + 3] - offs[4 * i + 2];
        if (offs[4 * i] < 0 || offs[4 * i + 2] < 0 || n < 0 || m < 0) continue;      // TLC_ST_BAD_INPUT below
        if (n > TLC_PD_WIDE_MAX_ITEMS || m > TLC_PD_WIDE_MAX_ITEMS || n + m > TLC_PD_WIDE_MAX_ITEMS) {
            tlc_set_error("%s: graph %lld has %lld nodes and %lld edges: n + m is above TLC_PD_WIDE_MAX_ITEMS", __func__, (long long)h_sel[i],
                          (long long)n, (long long)m);
            free(offs);
            return TLC_ERR_UNSUPPORTED;
        }
        const int64_t need = (int64_t)layout(n, m).bytes;
        if (work_bytes < need) {
            tlc_set_error("%s: d_work holds %lld bytes; graph %lld (%lld nodes, %lld edges) needs %lld", __func__, (long long)work_bytes,
                          (long long)h_sel[i], (long long)n, (long long)m, (long long)need);
            free(offs);
            return TLC_ERR_INVALID_ARG;
        }
    }
    char* w = tlc_align256(d_work);
    for (int64_t i = 0; i < n_sel && rc == TLC_OK; ++i) {
        const int64_t g = h_sel[i], no = offs[4 * i], eo = offs[4 * i + 2];
        const int64_t n = offs[4 * i + 1] - no, m = offs[4 * i + 3] - eo;
        const bool last = i + 1 == n_sel;
        const long long before = R.launches;
        int levels_bound = 0;
        if (no < 0 || eo < 0 || n < 0 || m < 0 || (m > 0 && !d_edges)) {
            hipLaunchKernelGGL(pdw_bad_row_kernel, dim3(1), dim3(64), 0, R.s, d_counts + 4 * g);
            R.launches += 1;
            if (last && h_stats) { h_stats[3] = 0; h_stats[4] = TLC_ST_BAD_INPUT; h_stats[2] = 1; }
            continue;
        }
        const Lay L = layout(n, m);
        rc = run_graph(R, w, L, (int)n, (int)m, d_edges + 2 * eo, d_f + no, flags, d_pd_up + 2 * no, d_pd_down + 2 * no, d_pd_one + 2 * eo,
                       d_ext0 + 2 * g, d_counts + 4 * g, d_edge_rank ? d_edge_rank + eo : nullptr, &levels_bound);
        if (rc == TLC_OK && last && h_stats) {
            int ctl[C_INTS];
            if (hipMemcpyAsync(ctl, w + L.ctl, sizeof(ctl), hipMemcpyDeviceToHost, R.s) != hipSuccess || hipStreamSynchronize(R.s) != hipSuccess) {
                tlc_set_error("%s: reading the statistics failed", __func__);
                rc = TLC_ERR_HIP;
                break;
            }
            h_stats[0] = ctl[C_LEVELS];
            h_stats[1] = ctl[C_ROUNDS];
            h_stats[2] = R.launches - before;
            h_stats[3] = ctl[C_FELL];
            h_stats[4] = ctl[C_STATUS];
        }
    }
    free(offs);
    return rc;
}

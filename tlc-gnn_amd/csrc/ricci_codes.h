// ricci_codes.h -- what the two Ollivier-Ricci transport methods share (ricci.hip: Sinkhorn, ricci_otd.hip: exact): the group
// barrier and the 2-bit hop codes of one edge's cost matrix, staged by the whole group.
#ifndef TLC_RICCI_CODES_H
#define TLC_RICCI_CODES_H
#include "tlc_common.h"

// (an anonymous namespace: every includer is one translation unit of its own, ricci.hip and ricci_otd.hip)
namespace {

template <int W>
__device__ __forceinline__ void group_sync() {
    if (W == 64) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    } else {
        __syncthreads();
    }
}

// hop codes are packed sixteen to a 32-bit word (a 437 x 404 hub-hub edge: 44 KB instead of 176 KB -- LDS instead of HBM)
__device__ __forceinline__ int code_at(const unsigned int* codes, int q) { return (int)((codes[q >> 4] >> ((q & 15) * 2)) & 3u); }

// Hop codes of edge (s, t): codes[(i * nb + j) / 16] holds d(a_i, b_j) in {0, 1, 2, 3}, a_i = the neighbours of s (ascending) then
// s itself, b_j likewise for t; na = deg(s) + 1, nb = deg(t) + 1.  codes: (na * nb + 15) / 16 words (LDS, or an HBM slot); idx:
// na + nb + 1 ints of LDS, left holding the ids of t's neighbours (idx[0 .. nb - 1)) and the prefix of deg(a_i) behind them.  The
// last pass (distance 0) is not followed by a barrier: the caller syncs before it reads the codes.
template <int W>
__device__ __forceinline__ void ricci_stage_codes(const int* rowptr, const int* col, int s, int t, unsigned int* codes,
                                                  int* idx, int tid) {
    const int sl = rowptr[s], tl = rowptr[t];
    const int ds = rowptr[s + 1] - sl, dt = rowptr[t + 1] - tl;
    const int na = ds + 1, nb = dt + 1;
    // support a_i: the neighbours of s, then s itself (mass alpha); the target support likewise (its ids are staged in LDS below)
    auto sup_a = [&](int i) { return i < ds ? col[sl + i] : s; };
    // Hop codes.  One entry at a time (two dependent binary searches over global rows per entry) took 4.7 ms on a 172 x 172 hub
    // edge; instead the rows around the source support are streamed once: the target support's ids sit in LDS (sorted), every
    // entry starts at 3, and for every (a_i, y in row(a_i)) unit -- dealt to the threads through a prefix over deg(a_i) -- the
    // row of y marks distance 2, y itself distance 1, a_i itself distance 0 (later passes overwrite earlier ones).
    int* const bid = idx;                    // [nb - 1] neighbours of t, ascending
    int* const off = idx + nb;               // [na + 1] prefix of deg(a_i)
    for (int j = tid; j < dt; j += W) bid[j] = col[tl + j];
    for (int i = tid; i < na; i += W) { const int a = sup_a(i); off[i + 1] = rowptr[a + 1] - rowptr[a]; }
    for (int q = tid; q < (na * nb + 15) / 16; q += W) codes[q] = 0xffffffffu;         // every entry 3
    group_sync<W>();
    if (tid == 0) {
        int run = 0;
        off[0] = 0;
        for (int i = 0; i < na; ++i) { run += off[i + 1]; off[i + 1] = run; }
    }
    group_sync<W>();
    const int units = off[na];
    auto pos_b = [&](int z) -> int {         // index of z in the target support, or -1
        if (z == t) return dt;
        int lo = 0, hi = dt;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            const int c = bid[mid];
            if (c == z) return mid;
            if (c < z) lo = mid + 1; else hi = mid;
        }
        return -1;
    };
    auto unit_row = [&](int k) -> int {      // the i whose row holds unit k: last i with off[i] <= k
        int lo = 0, hi = na;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (off[mid] <= k) lo = mid; else hi = mid;
        }
        return lo;
    };
    for (int k = tid; k < units; k += W) {
        const int i = unit_row(k);
        const int a = sup_a(i);
        const int y = col[rowptr[a] + (k - off[i])];
        const int yl = rowptr[y], yh = rowptr[y + 1];
        for (int q = yl; q < yh; ++q) {
            const int j = pos_b(col[q]);
            if (j >= 0) { const int q2 = i * nb + j; atomicAnd(&codes[q2 >> 4], ~(1u << ((q2 & 15) * 2))); }        // 3 -> 2
        }
    }
    group_sync<W>();
    for (int k = tid; k < units; k += W) {
        const int i = unit_row(k);
        const int j = pos_b(col[rowptr[sup_a(i)] + (k - off[i])]);
        if (j >= 0) {                                                                           // -> 1
            const int q1 = i * nb + j;
            atomicAnd(&codes[q1 >> 4], ~(3u << ((q1 & 15) * 2)));
            atomicOr(&codes[q1 >> 4], 1u << ((q1 & 15) * 2));
        }
    }
    group_sync<W>();
    for (int i = tid; i < na; i += W) {
        const int j = pos_b(sup_a(i));
        if (j >= 0) { const int q0 = i * nb + j; atomicAnd(&codes[q0 >> 4], ~(3u << ((q0 & 15) * 2))); }            // -> 0
    }
}

}  // namespace
#endif

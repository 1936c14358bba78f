// lp_metrics.hip -- binary ranking metrics of link-prediction scores on the device: ROC-AUC and average precision with
// sklearn's binary semantics (pos_label 1), the numbers pipelines.test scores the val and test splits with (pipelines.py:20-40).
//
//   tlc_binary_rank_metrics   per segment of (score, label): scores in descending order, equal scores one threshold
//                             (sklearn's _binary_clf_curve), -0.0 == +0.0.  AUC = the Mann-Whitney count
//                             U2 = sum_g p_g (2 N_below,g + n_g) in int64 over the tie groups g, divided by 2 P N with one
//                             rounding; AP = sum_g (p_g / P) tp_g / (tp_g + fp_g) in f64.
//
// Two tiers.  LDS: one 1024-thread workgroup per segment of at most TLC_RANK_LDS_CAP scores sorts it in LDS (bitonic, keys
// u64 + labels u8 = 9 B per score: 16 384 x 9 B = 144 KiB of the 160 KiB a gfx950 workgroup can declare; 20 480 u64 = 163 840 B
// compiles, one more u64 does not) and reduces it; up to 64 segments per launch.  Radix: a longer segment is sorted by an LSD
// radix sort over 8-bit digits (4 passes of u32 keys for f32 scores, 8 of u64 keys for f64; each pass = histogram, per-digit
// scan, stable scatter), then reduced in 4 096-score tiles (tile summary, one-workgroup tile scan, tile reduction, finalise).
//
// Sorted order is ascending in the key ~ord(score): descending scores.  The reduction needs, at each group end i, tp = positives
// through i and the positives before the group's first index s; it carries the latest group start as (s << 32) | cp_excl(s),
// whose max is the latest start (a max-scan).  U2 = 2 N P - W with W = sum_g p_g (2 fp_g - n_g), so tiles need no totals.
//
// Determinism: no floating-point atomics; the only atomics are LDS integer histogram counts.  The AP sum is a double-double
// (TwoSum) reduction in an order fixed by the segment's length alone, so a segment gives the same bits alone or in a batch.
#include "tlc_common.h"
#include "radix_passes.h"   // RK_BS / RK_IPT / RK_TILE, block_excl_sum, rk_tiles, rk_sort

namespace {

#define RK_CAP TLC_RANK_LDS_CAP        // scores per LDS-tier segment
#define RK_LDS_BS 1024                 // LDS tier: threads per workgroup, RK_CAP / RK_LDS_BS = 16 scores per thread
#define RK_MAX_SMALL 64                // LDS-tier segments per launch (kernel argument: 1 KiB)

struct SmallSegs {
    long long beg[RK_MAX_SMALL];
    int n[RK_MAX_SMALL];
    int seg[RK_MAX_SMALL];
};

// ---- keys and labels ------------------------------------------------------------------------------------------------------
// ascending key order == descending score order; -0.0 canonicalised to +0.0 first.  f32 keys are 32-bit (4 radix passes).
__device__ __forceinline__ uint32_t key_f32(float x, bool& nonfinite) {
    uint32_t u = __float_as_uint(x);
    nonfinite |= (u & 0x7f800000u) == 0x7f800000u;
    if (u == 0x80000000u) u = 0u;
    const uint32_t asc = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ~asc;
}
__device__ __forceinline__ uint64_t key_f64(double x, bool& nonfinite) {
    nonfinite |= ((uint64_t)__double_as_longlong(x) & 0x7ff0000000000000ull) == 0x7ff0000000000000ull;
    return ~tlc_ord_f64(x);
}
template <typename K>
__device__ __forceinline__ K load_key(const void* scores, int sdt, long long i, bool& nonfinite) {
    if (sdt == TLC_SCORE_F32) return (K)key_f32(((const float*)scores)[i], nonfinite);
    return (K)key_f64(((const double*)scores)[i], nonfinite);
}
// 1 for a positive, 0 for a negative; anything but 0 / 1 sets `bad` (stored as a negative)
__device__ __forceinline__ uint8_t load_label(const void* labels, int ldt, long long i, bool& bad) {
    if (ldt == TLC_LABEL_U8) {
        const uint8_t v = ((const uint8_t*)labels)[i];
        bad |= v > 1;
        return v == 1;
    }
    if (ldt == TLC_LABEL_I64) {
        const long long v = ((const long long*)labels)[i];
        bad |= (unsigned long long)v > 1ull;
        return v == 1;
    }
    const float v = ((const float*)labels)[i];
    bad |= !(v == 0.0f || v == 1.0f);
    return v == 1.0f;
}

// ---- double-double (TwoSum) accumulation --------------------------------------------------------------------------------
struct DD {
    double hi, lo;
};
__device__ __forceinline__ DD dd_add(DD a, double b) {
    const double s = a.hi + b, bp = s - a.hi;
    const double e = (a.hi - (s - bp)) + (b - bp);
    return DD{s, a.lo + e};
}
__device__ __forceinline__ DD dd_add(DD a, DD b) {
    DD s = dd_add(a, b.hi);
    const double lo = s.lo + b.lo;
    const double t = s.hi + lo;
    return DD{t, lo - (t - s.hi)};
}

// ---- block-level scans and reductions in a fixed order ------------------------------------------------------------------
// exclusive max-scan (identity -1) over the block; *total = the block's max
template <int BS>
__device__ long long block_excl_max(long long v, BlockScratch<BS>& sh, long long* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long o = __shfl_up(inc, d);
        if (lane >= d && o > inc) inc = o;
    }
    long long excl = __shfl_up(inc, 1);
    if (lane == 0) excl = -1;
    __syncthreads();
    if (lane == 63) sh.w[wave] = inc;
    __syncthreads();
    long long before = -1, tot = -1;
    for (int w = 0; w < BS / 64; ++w) {
        if (w < wave && sh.w[w] > before) before = sh.w[w];
        if (sh.w[w] > tot) tot = sh.w[w];
    }
    *total = tot;
    return before > excl ? before : excl;
}

// the block's double-double sum, in a butterfly order fixed by the thread index; valid in thread 0
template <int BS>
__device__ DD block_dd_sum(DD v, BlockScratch<BS>& sh) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        DD o{__shfl_xor(v.hi, d), __shfl_xor(v.lo, d)};
        v = dd_add(v, o);
    }
    __syncthreads();
    if (lane == 0) {
        sh.h[wave] = v.hi;
        sh.l[wave] = v.lo;
    }
    __syncthreads();
    DD r{0.0, 0.0};
    if (threadIdx.x == 0)
        for (int w = 0; w < BS / 64; ++w) r = dd_add(r, DD{sh.h[w], sh.l[w]});
    return r;
}

// ---- the pass over a sorted run ------------------------------------------------------------------------------------------
// Thread t takes scores [t0 + t*IPT, t0 + (t+1)*IPT) of the sorted segment (keys `key`, labels `lab`, length n).  carry_cp: the
// positives before t0; carry_start: the latest group start before t0 as (s << 32) | cp_excl(s), or -1.
// *tile_pos (if not NULL): the run's positives.  FINAL false: *tile_start = the run's latest group start (cp relative to the run).
// FINAL true: *W = the run's sum of p_g (2 fp_g - n_g) over the groups that END in it, *ap = sum p_g tp_g / (tp_g + fp_g).
template <int BS, bool FINAL, typename K>
__device__ void sorted_pass(const K* key, const uint8_t* lab, long long t0, long long n, long long carry_cp, long long carry_start,
                            BlockScratch<BS>& sh, long long* tile_pos, long long* tile_start, long long* W, DD* ap) {
    const long long i0 = t0 + (long long)threadIdx.x * RK_IPT;
    uint32_t pos = 0, start = 0, end = 0;          // bit j: score i0 + j is a positive / starts a group / ends a group
    int c = 0;
    if (i0 < n) {
        // a window (prev, cur, next) slides over the thread's scores: no per-score key array in registers
        K cur = key[i0];
        K prev = i0 > 0 ? key[i0 - 1] : ~cur;
#pragma unroll
        for (int j = 0; j < RK_IPT; ++j) {
            const long long i = i0 + j;
            if (i < n) {
                const K next = i + 1 < n ? key[i + 1] : ~cur;
                if (lab[i]) { pos |= 1u << j; ++c; }
                if (prev != cur) start |= 1u << j;
                if (next != cur) end |= 1u << j;
                prev = cur;
                cur = next;
            }
        }
    }
    long long tot;
    const long long cp0 = carry_cp + block_excl_sum<BS>(c, sh, &tot);
    long long st = -1, cp = cp0;
#pragma unroll
    for (int j = 0; j < RK_IPT; ++j) {
        if (start >> j & 1) st = ((i0 + j) << 32) | cp;
        cp += pos >> j & 1;
    }
    long long stmax;
    long long stx = block_excl_max<BS>(st, sh, &stmax);
    if (tile_pos) *tile_pos = tot;
    if (!FINAL) {
        *tile_start = stmax;
        return;
    }
    if (carry_start > stx) stx = carry_start;
    long long w = 0;
    DD a{0.0, 0.0};
    cp = cp0;
#pragma unroll 1
    for (int j = 0; j < RK_IPT; ++j) {
        const long long i = i0 + j;
        if (start >> j & 1) stx = (i << 32) | cp;
        cp += pos >> j & 1;
        if (end >> j & 1) {
            const long long s = stx >> 32, cps = stx & 0xffffffffll;
            const long long tp = cp, fp = i + 1 - cp;
            const long long p = tp - cps, ng = fp - (s - cps);
            w += p * (2 * fp - ng);
            if (p) a = dd_add(a, (double)(p * tp) / (double)(i + 1));
        }
    }
    long long wt;
    (void)block_excl_sum<BS>(w, sh, &wt);
    *W = wt;
    *ap = block_dd_sum<BS>(a, sh);
}

// a / b correctly rounded, 0 <= a <= b < 2^63, b > 0: 64 quotient bits by long division, the remainder as a sticky bit
__device__ double exact_ratio(unsigned long long a, unsigned long long b) {
    if (a == 0) return 0.0;
    if (a == b) return 1.0;
    unsigned long long r = a, q = 0;
    int bits = 0, e = 0;
    while (bits < 64) {
        r <<= 1;
        ++e;
        const unsigned long long bit = r >= b;
        if (bit) r -= b;
        if (q || bit) {
            q = (q << 1) | bit;
            ++bits;
        }
    }
    if (r) q |= 1;
    return ldexp((double)q, -e);
}

__device__ void write_result(int s, long long n, long long P, long long W, DD ap, int status, double* auc, double* apo,
                             long long* n_pos, long long* n_neg, int* st) {
    const long long N = n - P;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    if (n == 0) status |= TLC_RANK_EMPTY;
    n_pos[s] = P;
    n_neg[s] = N;
    st[s] = status;
    auc[s] = (P == 0 || N == 0) ? nan : exact_ratio((unsigned long long)(2 * N * P - W), (unsigned long long)(2 * N * P));
    apo[s] = n == 0 ? nan : P == 0 ? 0.0 : (ap.hi + ap.lo) / (double)P;
}

// ---- LDS tier: one workgroup per segment ----------------------------------------------------------------------------------
__global__ __launch_bounds__(RK_LDS_BS) void rank_lds_kernel(const void* __restrict__ scores, int sdt, const void* __restrict__ labels,
                                                             int ldt, SmallSegs segs, double* auc, double* ap, long long* n_pos,
                                                             long long* n_neg, int* status) {
    __shared__ uint64_t sk[RK_CAP];
    __shared__ uint8_t sl[RK_CAP];
    __shared__ BlockScratch<RK_LDS_BS> sh;
    const int tid = threadIdx.x;
    const long long beg = segs.beg[blockIdx.x];
    const int n = segs.n[blockIdx.x], s = segs.seg[blockIdx.x];
    int np = 2;
    while (np < n) np <<= 1;
    bool nf = false, bad = false;
    for (int i = tid; i < np; i += RK_LDS_BS) {
        if (i < n) {
            sk[i] = load_key<uint64_t>(scores, sdt, beg + i, nf);
            sl[i] = load_label(labels, ldt, beg + i, bad);
        } else {
            sk[i] = ~0ull;                   // padding sorts last; the reduction reads the first n only
            sl[i] = 0;
        }
    }
    const int flags = (__syncthreads_or(nf) ? TLC_RANK_NONFINITE : 0) | (__syncthreads_or(bad) ? TLC_RANK_BAD_LABEL : 0);
    // bitonic sort, ascending
    for (int k = 2; k <= np; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (np >> 1); t += RK_LDS_BS) {
                const int i = 2 * j * (t / j) + (t % j), l = i + j;
                const uint64_t a = sk[i], b = sk[l];
                if (((i & k) == 0) == (a > b)) {
                    sk[i] = b;
                    sk[l] = a;
                    const uint8_t x = sl[i];
                    sl[i] = sl[l];
                    sl[l] = x;
                }
            }
            __syncthreads();
        }
    }
    long long P, W;
    DD a;
    sorted_pass<RK_LDS_BS, true>(sk, sl, 0, n, 0, -1, sh, &P, nullptr, &W, &a);
    if (tid == 0) write_result(s, n, P, W, a, flags, auc, ap, n_pos, n_neg, status);
}

// ---- radix tier -----------------------------------------------------------------------------------------------------------
template <typename K>
__global__ __launch_bounds__(RK_BS) void rk_keys_kernel(const void* __restrict__ scores, int sdt, const void* __restrict__ labels,
                                                        int ldt, long long beg, long long n, K* __restrict__ keys,
                                                        uint8_t* __restrict__ labs, int* __restrict__ blk_flags) {
    bool nf = false, bad = false;
    const long long t0 = (long long)blockIdx.x * RK_TILE;
    for (int j = threadIdx.x; j < RK_TILE; j += RK_BS) {
        const long long i = t0 + j;
        if (i < n) {
            keys[i] = load_key<K>(scores, sdt, beg + i, nf);
            labs[i] = load_label(labels, ldt, beg + i, bad);
        }
    }
    const int f = (__syncthreads_or(nf) ? TLC_RANK_NONFINITE : 0) | (__syncthreads_or(bad) ? TLC_RANK_BAD_LABEL : 0);
    if (threadIdx.x == 0) blk_flags[blockIdx.x] = f;
}

template <typename K>
__global__ __launch_bounds__(RK_BS) void rk_tile_summary_kernel(const K* __restrict__ keys, const uint8_t* __restrict__ labs, long long n,
                                                                long long* __restrict__ tpos, long long* __restrict__ tstart) {
    __shared__ BlockScratch<RK_BS> sh;
    long long p, st;
    sorted_pass<RK_BS, false>(keys, labs, (long long)blockIdx.x * RK_TILE, n, 0, -1, sh, &p, &st, nullptr, nullptr);
    if (threadIdx.x == 0) {
        tpos[blockIdx.x] = p;
        tstart[blockIdx.x] = st;
    }
}

// one workgroup: per tile the positives before it and the latest group start before it; info[0] = P, info[1] = flags
#define RK_SCAN_BS 1024
__global__ __launch_bounds__(RK_SCAN_BS) void rk_tile_scan_kernel(int nb, const long long* __restrict__ tpos, const long long* __restrict__ tstart,
                                                                  const int* __restrict__ blk_flags, long long* __restrict__ ccp,
                                                                  long long* __restrict__ cst, long long* __restrict__ info) {
    __shared__ BlockScratch<RK_SCAN_BS> sh;
    const int per = (nb + RK_SCAN_BS - 1) / RK_SCAN_BS;
    const int b0 = threadIdx.x * per, b1 = min(nb, b0 + per);
    long long sum = 0;
    int f = 0;
    for (int b = b0; b < b1; ++b) {
        sum += tpos[b];
        f |= blk_flags[b];
    }
    long long P;
    long long cp = block_excl_sum<RK_SCAN_BS>(sum, sh, &P);
    long long mx = -1, cp2 = cp;
    for (int b = b0; b < b1; ++b) {
        if (tstart[b] >= 0) mx = tstart[b] + cp2;           // the run-relative cp of the start, made global
        cp2 += tpos[b];
    }
    long long dummy;
    long long st = block_excl_max<RK_SCAN_BS>(mx, sh, &dummy);
    for (int b = b0; b < b1; ++b) {
        ccp[b] = cp;
        cst[b] = st;
        if (tstart[b] >= 0) st = tstart[b] + cp;
        cp += tpos[b];
    }
    f = (__syncthreads_or(f & TLC_RANK_NONFINITE) ? TLC_RANK_NONFINITE : 0) | (__syncthreads_or(f & TLC_RANK_BAD_LABEL) ? TLC_RANK_BAD_LABEL : 0);
    if (threadIdx.x == 0) {
        info[0] = P;
        info[1] = f;
    }
}

template <typename K>
__global__ __launch_bounds__(RK_BS) void rk_tile_reduce_kernel(const K* __restrict__ keys, const uint8_t* __restrict__ labs, long long n,
                                                               const long long* __restrict__ ccp, const long long* __restrict__ cst,
                                                               long long* __restrict__ tw, double* __restrict__ tap) {
    __shared__ BlockScratch<RK_BS> sh;
    long long w;
    DD a;
    sorted_pass<RK_BS, true>(keys, labs, (long long)blockIdx.x * RK_TILE, n, ccp[blockIdx.x], cst[blockIdx.x], sh, nullptr, nullptr, &w, &a);
    if (threadIdx.x == 0) {
        tw[blockIdx.x] = w;
        tap[2 * blockIdx.x] = a.hi;
        tap[2 * blockIdx.x + 1] = a.lo;
    }
}

// one workgroup: the tiles' W and AP partials in a fixed order (thread t: its run of tiles in order, then the block tree)
__global__ __launch_bounds__(RK_SCAN_BS) void rk_finalize_kernel(int nb, long long n, const long long* __restrict__ tw,
                                                                 const double* __restrict__ tap, const long long* __restrict__ info, int s,
                                                                 double* auc, double* ap, long long* n_pos, long long* n_neg, int* status) {
    __shared__ BlockScratch<RK_SCAN_BS> sh;
    const int per = (nb + RK_SCAN_BS - 1) / RK_SCAN_BS;
    const int b0 = threadIdx.x * per, b1 = min(nb, b0 + per);
    long long w = 0;
    DD a{0.0, 0.0};
    for (int b = b0; b < b1; ++b) {
        w += tw[b];
        a = dd_add(a, DD{tap[2 * b], tap[2 * b + 1]});
    }
    long long W;
    (void)block_excl_sum<RK_SCAN_BS>(w, sh, &W);
    a = block_dd_sum<RK_SCAN_BS>(a, sh);
    if (threadIdx.x == 0) write_result(s, n, info[0], W, a, (int)info[1], auc, ap, n_pos, n_neg, status);
}

// ---- host side ------------------------------------------------------------------------------------------------------------
inline long long rk_align(long long x) { return (x + 255) & ~255ll; }

struct RadixLayout {
    long long keys_a, keys_b, labs_a, labs_b, hist, tot, flags, tpos, tstart, ccp, cst, tw, tap, info, bytes;
};
RadixLayout radix_layout(long long n, int key_bytes) {
    const long long nb = rk_tiles(n);
    RadixLayout L;
    long long o = 0;
    L.keys_a = o; o += rk_align(n * key_bytes);
    L.keys_b = o; o += rk_align(n * key_bytes);
    L.labs_a = o; o += rk_align(n);
    L.labs_b = o; o += rk_align(n);
    L.hist = o; o += rk_align(rk_hist_ints(n) * 4);
    L.tot = o; o += rk_align(RK_TOT_INTS * 4);
    L.flags = o; o += rk_align(nb * 4);
    L.tpos = o; o += rk_align(nb * 8);
    L.tstart = o; o += rk_align(nb * 8);
    L.ccp = o; o += rk_align(nb * 8);
    L.cst = o; o += rk_align(nb * 8);
    L.tw = o; o += rk_align(nb * 8);
    L.tap = o; o += rk_align(nb * 16);
    L.info = o; o += rk_align(2 * 8);
    L.bytes = o;
    return L;
}

bool is_small(long long len, uint32_t flags) { return len == 0 || (len <= RK_CAP && !(flags & TLC_RANK_FORCE_RADIX)); }

// -1: malformed seg_ptr / flags; -2: a segment of 2^31 scores or more
long long rank_work_bytes(const int64_t* seg_ptr, int32_t n_segs, int score_dtype, uint32_t flags) {
    if (!seg_ptr || n_segs < 1 || (flags & ~TLC_RANK_FORCE_RADIX) || seg_ptr[0] < 0) return -1;
    long long mx = 0;
    for (int s = 0; s < n_segs; ++s) {
        const long long len = seg_ptr[s + 1] - seg_ptr[s];
        if (len < 0) return -1;
        if (len >= (1ll << 31)) return -2;
        if (!is_small(len, flags)) {
            const long long b = radix_layout(len, score_dtype == TLC_SCORE_F32 ? 4 : 8).bytes;
            if (b > mx) mx = b;
        }
    }
    return mx;
}

template <typename K>
int radix_segment(const void* scores, int sdt, const void* labels, int ldt, long long beg, long long n, int s, char* work, double* auc,
                  double* ap, long long* n_pos, long long* n_neg, int* status, hipStream_t st) {
    const RadixLayout L = radix_layout(n, sizeof(K));
    const int nb = (int)rk_tiles(n);
    K* ka = (K*)(work + L.keys_a);
    K* kb = (K*)(work + L.keys_b);
    uint8_t* la = (uint8_t*)(work + L.labs_a);
    uint8_t* lb = (uint8_t*)(work + L.labs_b);
    int* hist = (int*)(work + L.hist);
    int* tot = (int*)(work + L.tot);
    int* fl = (int*)(work + L.flags);
    long long *tpos = (long long*)(work + L.tpos), *tstart = (long long*)(work + L.tstart), *ccp = (long long*)(work + L.ccp),
              *cst = (long long*)(work + L.cst), *tw = (long long*)(work + L.tw), *info = (long long*)(work + L.info);
    double* tap = (double*)(work + L.tap);
    hipLaunchKernelGGL(rk_keys_kernel<K>, dim3(nb), dim3(RK_BS), 0, st, scores, sdt, labels, ldt, beg, n, ka, la, fl);
    rk_sort<8 * sizeof(K)>(st, n, ka, kb, la, lb, hist, tot);      // (a forced segment of one score: nothing to sort)
    hipLaunchKernelGGL(rk_tile_summary_kernel<K>, dim3(nb), dim3(RK_BS), 0, st, ka, la, n, tpos, tstart);
    hipLaunchKernelGGL(rk_tile_scan_kernel, dim3(1), dim3(RK_SCAN_BS), 0, st, nb, tpos, tstart, fl, ccp, cst, info);
    hipLaunchKernelGGL(rk_tile_reduce_kernel<K>, dim3(nb), dim3(RK_BS), 0, st, ka, la, n, ccp, cst, tw, tap);
    hipLaunchKernelGGL(rk_finalize_kernel, dim3(1), dim3(RK_SCAN_BS), 0, st, nb, n, tw, tap, info, s, auc, ap, n_pos, n_neg, status);
    TLC_HIP_CHECK(hipGetLastError());
    return TLC_OK;
}

}  // namespace

extern "C" int64_t tlc_binary_rank_metrics_work_bytes(const int64_t* h_seg_ptr, int32_t n_segs, int score_dtype, uint32_t flags) {
    if (score_dtype != TLC_SCORE_F32 && score_dtype != TLC_SCORE_F64) return -1;
    const long long b = rank_work_bytes(h_seg_ptr, n_segs, score_dtype, flags);
    return b < 0 ? -1 : b;
}

extern "C" int tlc_binary_rank_metrics(const void* d_scores, int score_dtype, const void* d_labels, int label_dtype, const int64_t* h_seg_ptr,
                                       int32_t n_segs, uint32_t flags, double* d_auc, double* d_ap, int64_t* d_n_pos, int64_t* d_n_neg,
                                       int32_t* d_status, void* d_work, int64_t work_bytes, void* stream) {
    if (score_dtype != TLC_SCORE_F32 && score_dtype != TLC_SCORE_F64) {
        tlc_set_error("tlc_binary_rank_metrics: score_dtype %d is not TLC_SCORE_F32 / TLC_SCORE_F64", score_dtype);
        return TLC_ERR_UNSUPPORTED;
    }
    if (label_dtype != TLC_LABEL_U8 && label_dtype != TLC_LABEL_I64 && label_dtype != TLC_LABEL_F32) {
        tlc_set_error("tlc_binary_rank_metrics: label_dtype %d is not TLC_LABEL_U8 / I64 / F32", label_dtype);
        return TLC_ERR_UNSUPPORTED;
    }
    TLC_REQUIRE(d_auc && d_ap && d_n_pos && d_n_neg && d_status, "output pointers must not be NULL");
    const long long need = rank_work_bytes(h_seg_ptr, n_segs, score_dtype, flags);
    if (need == -2) {
        tlc_set_error("tlc_binary_rank_metrics: a segment holds 2^31 scores or more");
        return TLC_ERR_UNSUPPORTED;
    }
    TLC_REQUIRE(need >= 0, "seg_ptr must be non-NULL, start at >= 0 and be non-decreasing; n_segs >= 1; flags: TLC_RANK_FORCE_RADIX only");
    TLC_REQUIRE(h_seg_ptr[n_segs] == h_seg_ptr[0] || (d_scores && d_labels), "scores / labels must not be NULL");
    TLC_REQUIRE(need == 0 || (d_work && work_bytes >= need && ((uintptr_t)d_work & 15) == 0),
                "d_work must be 16-byte aligned and hold tlc_binary_rank_metrics_work_bytes() bytes");
    hipStream_t st = (hipStream_t)stream;
    SmallSegs small;
    int ns = 0;
    for (int s = 0; s <= n_segs; ++s) {
        if (ns == RK_MAX_SMALL || (s == n_segs && ns > 0)) {
            hipLaunchKernelGGL(rank_lds_kernel, dim3(ns), dim3(RK_LDS_BS), 0, st, d_scores, score_dtype, d_labels, label_dtype, small,
                               d_auc, d_ap, (long long*)d_n_pos, (long long*)d_n_neg, (int*)d_status);
            TLC_HIP_CHECK(hipGetLastError());
            ns = 0;
        }
        if (s == n_segs) break;
        const long long len = h_seg_ptr[s + 1] - h_seg_ptr[s];
        if (is_small(len, flags)) {
            small.beg[ns] = h_seg_ptr[s];
            small.n[ns] = (int)len;
            small.seg[ns] = s;
            ++ns;
        }
    }
    for (int s = 0; s < n_segs; ++s) {
        const long long len = h_seg_ptr[s + 1] - h_seg_ptr[s];
        if (is_small(len, flags)) continue;
        const int rc = score_dtype == TLC_SCORE_F32
                           ? radix_segment<uint32_t>(d_scores, score_dtype, d_labels, label_dtype, h_seg_ptr[s], len, s, (char*)d_work,
                                                     d_auc, d_ap, (long long*)d_n_pos, (long long*)d_n_neg, (int*)d_status, st)
                           : radix_segment<uint64_t>(d_scores, score_dtype, d_labels, label_dtype, h_seg_ptr[s], len, s, (char*)d_work,
                                                     d_auc, d_ap, (long long*)d_n_pos, (long long*)d_n_neg, (int*)d_status, st);
        if (rc != TLC_OK) return rc;
    }
    return TLC_OK;
}

// landscape.hip -- persistence landscapes of packed diagrams and their gradient (tlc_landscape, tlc_landscape_vjp).
//
// out[b, k, j] = the k-th largest tent value  v_i(t_j) = min(t_j - birth_i, death_i - t_j) > 0  among the points of diagram b, ties
// to the lower index; include/tlcgnn.h defines it operation by operation.  The design rests on one fact: a lane owns a sample and the
// points stream past it.  The lane keeps its K best (value, index) pairs as a sorted list in registers (LsTop<KT>: KT = 1, 2, 4, 8, 16
// is a template parameter, a requested K runs in the next one up; the insertion is fully unrolled, every index a compile-time constant,
// so nothing goes to scratch).  Inserting on strict > while the points arrive in ascending index gives the tie rule for free, and
// absent cells (no value above the list's initial +0.0) keep (+0.0, -1).  Three implementations, cut on the device by n (every kernel
// skips the diagrams of the other classes):
//
//   n <= TLC_LS_WAVE_NMAX   one wavefront per diagram, LS_WAVES per workgroup, grid-stride over the batch.  Lane i loads point i once;
//                           the scan broadcasts point i with a wave-uniform readlane; lanes take the samples lane, lane + 64, ...
//   n <= TLC_LS_LDS_NMAX    one workgroup per (diagram, block of LS_BS samples).  The points are staged once in LDS (16 B each, as much
//                           as the call's largest diagram of this class needs: 64 KB at the cap, two workgroups per CU) and every
//                           thread scans them with broadcast reads -- the same address across a wavefront, no bank conflict.
//   above                   the whole device, one diagram after the other.  Work items are (slice of TLC_LS_LDS_NMAX points, sample
//                           block): each writes its slice's K-list per sample (value, index in the diagram) to d_work, and a merge
//                           kernel offers a cell's lists to one LsTop, the slices ascending.  The order (value descending, index
//                           ascending) is strict and total, so the K best of a union are the K best of the parts' K best, in the
//                           same order whatever the parts: a smaller workspace (fewer slices in flight, the running list in slot 0
//                           carried from group to group) gives the same bits.
//
// The VJP is a +-1 selection.  One owner sums a point: thread i scans the diagram's K * T winners in ascending (k, j) and adds the
// cells that name it, so there is no floating-point atomic and the order is the header's.  n <= 64: lanes own points; 64 cells at a
// time (winner, upstream, sample) are loaded coalesced and pass by as wave-uniform readlanes.  Above: a workgroup owns LS_BS points and
// stages the cells through LDS in chunks of LS_CHUNK, four winners per broadcast read; a hit -- at most one lane per cell -- reads the
// (upstream, sample) pair.  The cost is n * K * T / 64 wavefront steps per diagram; a sort of the cells by winner (radix_passes.h) would be
// O(K * T log) and is not built: the entry takes no workspace (DESIGN.md 6.16 has what the scan costs).
#include "tlc_common.h"

#include <stdlib.h>

#include <cmath>

#include "scratch_layouts.h"

namespace {

#define LS_BS 256
#define LS_WAVES (LS_BS / 64)
#define LS_MAX_GRID 2048                     // workgroups of a grid-stride launch: 8 per CU
#define LS_WAVE_N TLC_LS_WAVE_NMAX
#define LS_LDS_N TLC_LS_LDS_NMAX
#define LS_CHUNK 1024                        // cells of the VJP's LDS stage
#define LS_MAX_POINTS (1ll << 27)
static_assert(LS_WAVE_N == 64, "one lane per point");
static_assert(LS_LDS_N == TlcLandscapeScratch::SLICE, "a slice of the whole-device class is one LDS stage");
static_assert(LS_LDS_N * 16 <= 64 * 1024, "the staged points fit the default dynamic LDS");
static_assert(TLC_LS_KMAX == 16, "the instantiations below");

__device__ __forceinline__ bool ls_finite(double x) {
    return ((unsigned long long)__double_as_longlong(x) & 0x7FF0000000000000ull) != 0x7FF0000000000000ull;
}
__device__ __forceinline__ double ls_nan() { return __longlong_as_double(0x7FF8000000000000ll); }
__device__ __forceinline__ double ls_readlane_f64(double v, int l) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, l);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), l);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
__device__ __forceinline__ double ls_tent(double t, double b, double d) {
    const double up = t - b, down = d - t;
    return up < down ? up : down;
}

// The K best (value, index) of the values offered so far, value descending; a value enters above the entries it is strictly greater
// than, so among equal values the one offered first stays first.
template <int KT>
struct LsTop {
    double v[KT];
    int id[KT];
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int k = 0; k < KT; ++k) { v[k] = 0.0; id[k] = -1; }
    }
    __device__ __forceinline__ void offer(double x, int i) {
        if (x > v[KT - 1]) {
#pragma unroll
            for (int k = KT - 1; k >= 0; --k) {
                if (x > v[k]) {
                    if (k + 1 < KT) { v[k + 1] = v[k]; id[k + 1] = id[k]; }
                    v[k] = x; id[k] = i;
                }
            }
        }
    }
};

struct LsArgs {
    int n_dgms;
    const long long* offs;
    const double* pts;       // [sum n, 2]
    int T;
    const double* ts;
    int K;
    double* out;             // [B, K, T]
    int* winner;             // [B, K, T] or null
    unsigned char* status;
};

// the K rows of sample j of one diagram (bad: a NaN / Inf coordinate)
template <int KT>
__device__ __forceinline__ void ls_store(const LsArgs& A, long long p, int j, const LsTop<KT>& L, bool bad) {
    const long long base = p * A.K * (long long)A.T + j;
#pragma unroll
    for (int k = 0; k < KT; ++k) {
        if (k < A.K) {
            A.out[base + (long long)k * A.T] = bad ? ls_nan() : L.v[k];
            if (A.winner) A.winner[base + (long long)k * A.T] = bad ? -1 : L.id[k];
        }
    }
}

// ---- n <= 64: one wavefront per diagram ---------------------------------------------------------------------------------------
template <int KT>
__global__ __launch_bounds__(LS_BS) void ls_wave_kernel(LsArgs A) {
    const int lane = (int)(threadIdx.x & 63);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long w0 = (long long)blockIdx.x * LS_WAVES + wave, stride = (long long)gridDim.x * LS_WAVES;
    for (long long p = w0; p < A.n_dgms; p += stride) {
        const long long o0 = A.offs[p], nn = A.offs[p + 1] - o0;
        if (nn > LS_WAVE_N) continue;
        const int n = (int)nn;
        double pb = 0.0, pd = 0.0;
        if (lane < n) { pb = A.pts[2 * (o0 + lane)]; pd = A.pts[2 * (o0 + lane) + 1]; }
        const bool bad = __ballot(!(ls_finite(pb) && ls_finite(pd))) != 0ull;
        if (lane == 0) A.status[p] = bad ? 3 : 0;
        for (int j0 = 0; j0 < A.T; j0 += 64) {
            const int j = j0 + lane;
            const double t = j < A.T ? A.ts[j] : 0.0;
            LsTop<KT> L;
            L.init();
            if (!bad)
                for (int i = 0; i < n; ++i) L.offer(ls_tent(t, ls_readlane_f64(pb, i), ls_readlane_f64(pd, i)), i);
            if (j < A.T) ls_store<KT>(A, p, j, L, bad);
        }
    }
}

// ---- the scan of the staged points: sm[i] = (birth, death) of point i0 + i ------------------------------------------------------
template <int KT>
__device__ __forceinline__ void ls_scan(const double2* sm, int cnt, int i0, double t, LsTop<KT>& L) {
    for (int i = 0; i < cnt; ++i) {
        const double2 q = sm[i];
        L.offer(ls_tent(t, q.x, q.y), i0 + i);
    }
}
// stage cnt points from row `first`; true on this thread when one of its points has a NaN / Inf coordinate
__device__ __forceinline__ bool ls_stage(double2* sm, const double* pts, long long first, int cnt) {
    bool bad = false;
    for (int i = (int)threadIdx.x; i < cnt; i += LS_BS) {
        double2 q;
        q.x = pts[2 * (first + i)];
        q.y = pts[2 * (first + i) + 1];
        sm[i] = q;
        bad |= !(ls_finite(q.x) && ls_finite(q.y));
    }
    return bad;
}

// ---- 64 < n <= LS_LDS_N: one workgroup per (diagram, sample block) --------------------------------------------------------------
template <int KT>
__global__ __launch_bounds__(LS_BS) void ls_lds_kernel(LsArgs A, int nsb) {
    extern __shared__ double2 ls_sm[];
    const long long items = (long long)A.n_dgms * nsb;
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const long long p = it / nsb;
        const int sb = (int)(it - p * nsb);
        const long long o0 = A.offs[p], nn = A.offs[p + 1] - o0;
        if (nn <= LS_WAVE_N || nn > LS_LDS_N) continue;          // (the same for the whole workgroup)
        const int n = (int)nn;
        __syncthreads();                                         // the item before is read
        const bool bad = __syncthreads_or(ls_stage(ls_sm, A.pts, o0, n)) != 0;
        const int j = sb * LS_BS + (int)threadIdx.x;
        const double t = j < A.T ? A.ts[j] : 0.0;
        LsTop<KT> L;
        L.init();
        if (!bad) ls_scan<KT>(ls_sm, n, 0, t, L);
        if (sb == 0 && threadIdx.x == 0) A.status[p] = bad ? 3 : 0;
        if (j < A.T) ls_store<KT>(A, p, j, L, bad);
    }
}

// ---- above: slices of one diagram, then the merge ---------------------------------------------------------------------------------
struct LsWide {
    long long o0, n;         // the diagram's first row and its points
    int s0, G;               // the group's first slice and its slices
    char* slots;             // slot 0: the running list; slot 1 + g: slice s0 + g
    long long slot_bytes, val, idx;
    int* ctl;                // != 0: a NaN / Inf coordinate
    __device__ __forceinline__ double* sv(int slot) const { return (double*)(slots + slot * slot_bytes + val); }
    __device__ __forceinline__ int* si(int slot) const { return (int*)(slots + slot * slot_bytes + idx); }
};

template <int KT>
__global__ __launch_bounds__(LS_BS) void ls_slice_kernel(LsArgs A, LsWide W, int nsb) {
    extern __shared__ double2 ls_sm[];
    const int items = W.G * nsb;
    for (int it = (int)blockIdx.x; it < items; it += (int)gridDim.x) {
        const int g = it / nsb, sb = it - g * nsb;
        const long long i0 = (long long)(W.s0 + g) * LS_LDS_N;
        const int cnt = (int)(W.n - i0 < LS_LDS_N ? W.n - i0 : LS_LDS_N);
        __syncthreads();
        if (__syncthreads_or(ls_stage(ls_sm, A.pts, W.o0 + i0, cnt)) && threadIdx.x == 0) atomicOr(W.ctl, 1);
        const int j = sb * LS_BS + (int)threadIdx.x;
        const double t = j < A.T ? A.ts[j] : 0.0;
        LsTop<KT> L;
        L.init();
        ls_scan<KT>(ls_sm, cnt, (int)i0, t, L);
        if (j < A.T) {
            double* sv = W.sv(1 + g);
            int* si = W.si(1 + g);
#pragma unroll
            for (int k = 0; k < KT; ++k)
                if (k < A.K) { sv[(long long)k * A.T + j] = L.v[k]; si[(long long)k * A.T + j] = L.id[k]; }
        }
    }
}

// a thread per sample: the running list (unless this is the first group), then the group's slices ascending; the running list again,
// or after the last group the diagram's rows and status
template <int KT>
__global__ __launch_bounds__(LS_BS) void ls_merge_kernel(LsArgs A, LsWide W, long long p, int first, int last) {
    const bool bad = *W.ctl != 0;
    for (int j = (int)(blockIdx.x * LS_BS + threadIdx.x); j < A.T; j += (int)(gridDim.x * LS_BS)) {
        LsTop<KT> L;
        L.init();
        for (int slot = first ? 1 : 0; slot <= W.G; ++slot) {
            const double* sv = W.sv(slot);
            const int* si = W.si(slot);
#pragma unroll
            for (int k = 0; k < KT; ++k)
                if (k < A.K) L.offer(sv[(long long)k * A.T + j], si[(long long)k * A.T + j]);
        }
        if (last) {
            ls_store<KT>(A, p, j, L, bad);
        } else {
            double* sv = W.sv(0);
            int* si = W.si(0);
#pragma unroll
            for (int k = 0; k < KT; ++k)
                if (k < A.K) { sv[(long long)k * A.T + j] = L.v[k]; si[(long long)k * A.T + j] = L.id[k]; }
        }
    }
    if (last && blockIdx.x == 0 && threadIdx.x == 0) A.status[p] = bad ? 3 : 0;
}

// ---- the VJP ------------------------------------------------------------------------------------------------------------------------
struct LsVjpArgs {
    int n_dgms;
    const long long* offs;
    const double* pts;
    int T;
    const double* ts;
    int K;
    const int* winner;       // [B, K, T]
    const double* gout;      // [B, K, T]
    double* gpts;            // [sum n, 2]
};
// cell (winner i, upstream g, sample t) of the point (b, d): the birth side wins the tie at the peak
__device__ __forceinline__ void ls_vjp_add(double& gb, double& gd, double b, double d, double g, double t) {
    if (t - b <= d - t) gb += -g;
    else gd += g;
}

__global__ __launch_bounds__(LS_BS) void ls_vjp_wave_kernel(LsVjpArgs A) {
    const int lane = (int)(threadIdx.x & 63);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long w0 = (long long)blockIdx.x * LS_WAVES + wave, stride = (long long)gridDim.x * LS_WAVES;
    const int cells = A.K * A.T;
    for (long long p = w0; p < A.n_dgms; p += stride) {
        const long long o0 = A.offs[p], nn = A.offs[p + 1] - o0;
        if (nn > LS_WAVE_N) continue;
        const int n = (int)nn;
        double b = 0.0, d = 0.0, gb = 0.0, gd = 0.0;
        if (lane < n) { b = A.pts[2 * (o0 + lane)]; d = A.pts[2 * (o0 + lane) + 1]; }
        const int* win = A.winner + p * cells;
        const double* go = A.gout + p * cells;
        // 64 cells at a time: lane l loads cell c0 + l (coalesced), then the cells pass by in order, each a wave-uniform readlane
        for (int c0 = 0; c0 < cells; c0 += 64) {
            const int c = c0 + lane;
            int wv = -1;
            double gv = 0.0, tv = 0.0;
            if (c < cells) { wv = win[c]; gv = go[c]; tv = A.ts[c % A.T]; }
            const int cc = cells - c0 < 64 ? cells - c0 : 64;
            for (int i = 0; i < cc; ++i) {
                const int w = __builtin_amdgcn_readlane(wv, i);
                if (w < 0) continue;
                const double g = ls_readlane_f64(gv, i), t = ls_readlane_f64(tv, i);
                if (w == lane) ls_vjp_add(gb, gd, b, d, g, t);
            }
        }
        if (lane < n) { A.gpts[2 * (o0 + lane)] = gb; A.gpts[2 * (o0 + lane) + 1] = gd; }
    }
}

// a workgroup per (diagram, block of LS_BS points); only: >= 0 the one diagram of the whole-device class (its blocks are the grid's
// items), < 0 every diagram of the workgroup class (items (diagram, block) with LS_LDS_N / LS_BS blocks each)
__global__ __launch_bounds__(LS_BS) void ls_vjp_block_kernel(LsVjpArgs A, long long only) {
    __shared__ int4 s_w4[LS_CHUNK / 4];
    __shared__ double2 s_gt[LS_CHUNK];
    int* s_w = (int*)s_w4;
    constexpr int PB = LS_LDS_N / LS_BS;
    const int cells = A.K * A.T;
    const long long n_only = only >= 0 ? A.offs[only + 1] - A.offs[only] : 0;
    const long long items = only >= 0 ? (n_only + LS_BS - 1) / LS_BS : (long long)A.n_dgms * PB;
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const long long p = only >= 0 ? only : it / PB, pb = only >= 0 ? it : it - p * PB;
        const long long o0 = A.offs[p], n = A.offs[p + 1] - o0;
        if (only < 0 && (n <= LS_WAVE_N || n > LS_LDS_N || pb * LS_BS >= n)) continue;
        const long long i = pb * LS_BS + threadIdx.x;
        const int me = i < n ? (int)i : -2;                      // (no winner is -2)
        double b = 0.0, d = 0.0, gb = 0.0, gd = 0.0;
        if (i < n) { b = A.pts[2 * (o0 + i)]; d = A.pts[2 * (o0 + i) + 1]; }
        const int* win = A.winner + p * cells;
        const double* go = A.gout + p * cells;
        for (int c0 = 0; c0 < cells; c0 += LS_CHUNK) {
            const int cc = cells - c0 < LS_CHUNK ? cells - c0 : LS_CHUNK;
            __syncthreads();
            for (int c = (int)threadIdx.x; c < LS_CHUNK; c += LS_BS) {
                s_w[c] = c < cc ? win[c0 + c] : -1;
                if (c < cc) {
                    double2 gt;
                    gt.x = go[c0 + c];
                    gt.y = A.ts[(c0 + c) % A.T];
                    s_gt[c] = gt;
                }
            }
            __syncthreads();
            for (int q = 0; 4 * q < cc; ++q) {                   // four winners per broadcast read, the cells still ascending
                const int4 w = s_w4[q];
                if (w.x == me) { const double2 gt = s_gt[4 * q]; ls_vjp_add(gb, gd, b, d, gt.x, gt.y); }
                if (w.y == me) { const double2 gt = s_gt[4 * q + 1]; ls_vjp_add(gb, gd, b, d, gt.x, gt.y); }
                if (w.z == me) { const double2 gt = s_gt[4 * q + 2]; ls_vjp_add(gb, gd, b, d, gt.x, gt.y); }
                if (w.w == me) { const double2 gt = s_gt[4 * q + 3]; ls_vjp_add(gb, gd, b, d, gt.x, gt.y); }
            }
        }
        if (i < n) { A.gpts[2 * (o0 + i)] = gb; A.gpts[2 * (o0 + i) + 1] = gd; }
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------
unsigned ls_grid(long long items) { return (unsigned)(items < 1 ? 1 : items > LS_MAX_GRID ? LS_MAX_GRID : items); }

template <int KT>
int ls_launch(const LsArgs& A, const int64_t* offs, long long n_wave, long long n_lds, long long n_wide, long long max_lds, char* w,
              int64_t work_bytes, const TlcLandscapeScratch& S, hipStream_t st) {
    const int nsb = (A.T + LS_BS - 1) / LS_BS;
    if (n_wave) hipLaunchKernelGGL(ls_wave_kernel<KT>, dim3(ls_grid(((long long)A.n_dgms + LS_WAVES - 1) / LS_WAVES)), dim3(LS_BS), 0, st, A);
    if (n_lds)
        hipLaunchKernelGGL(ls_lds_kernel<KT>, dim3(ls_grid((long long)A.n_dgms * nsb)), dim3(LS_BS), (size_t)max_lds * 16, st, A, nsb);
    if (!n_wide) return TLC_OK;
    const int G = (int)S.groups_in(work_bytes);                  // (the entry checked that one slice fits)
    LsWide W{0, 0, 0, 0, w + S.slots, S.slot_bytes, S.val, S.idx, (int*)(w + S.ctl)};
    for (long long p = 0; p < A.n_dgms; ++p) {
        W.o0 = offs[p];
        W.n = offs[p + 1] - offs[p];
        if (W.n <= LS_LDS_N) continue;
        if (hipMemsetAsync(W.ctl, 0, sizeof(int), st) != hipSuccess) return TLC_ERR_HIP;
        const int slices = (int)TlcLandscapeScratch::slices_of(W.n);
        for (int s0 = 0; s0 < slices; s0 += G) {
            W.s0 = s0;
            W.G = slices - s0 < G ? slices - s0 : G;
            hipLaunchKernelGGL(ls_slice_kernel<KT>, dim3(ls_grid((long long)W.G * nsb)), dim3(LS_BS), (size_t)LS_LDS_N * 16, st, A, W, nsb);
            hipLaunchKernelGGL(ls_merge_kernel<KT>, dim3((unsigned)nsb), dim3(LS_BS), 0, st, A, W, p, (int)(s0 == 0), (int)(s0 + W.G >= slices));
        }
    }
    return TLC_OK;
}

// what both entries check before a pointer is read; 0 or the code to return
int ls_check_sizes(const char* fn, int32_t n_dgms, int32_t T, int32_t K, int64_t max_points) {
    if (n_dgms < 0 || max_points < 0) { tlc_set_error("%s: negative size", fn); return TLC_ERR_INVALID_ARG; }
    if (T < 1 || T > TLC_LS_TMAX) { tlc_set_error("%s: T outside 1 .. TLC_LS_TMAX", fn); return TLC_ERR_INVALID_ARG; }
    if (K < 1 || K > TLC_LS_KMAX) { tlc_set_error("%s: K outside 1 .. TLC_LS_KMAX", fn); return TLC_ERR_INVALID_ARG; }
    return TLC_OK;
}

// The offsets and the samples, read back once; the classes counted.  Returns TLC_OK or the refusal.
struct LsHost {
    int64_t* offs = nullptr;
    long long n_wave = 0, n_lds = 0, n_wide = 0, max_lds = 0;
    ~LsHost() { free(offs); }
};
int ls_read_back(const char* fn, LsHost& H, int32_t n_dgms, const int64_t* d_offs, int32_t T, const double* d_ts, int64_t max_points,
                 hipStream_t st) {
    const size_t B = (size_t)n_dgms;
    H.offs = (int64_t*)malloc((B + 1) * sizeof(int64_t) + (size_t)T * sizeof(double));
    if (!H.offs) { tlc_set_error("%s: out of host memory", fn); return TLC_ERR_OUT_OF_MEMORY; }
    double* ts = (double*)(H.offs + B + 1);
    if (hipMemcpyAsync(H.offs, d_offs, (B + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(ts, d_ts, (size_t)T * sizeof(double), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
        tlc_set_error("%s: reading the offsets and the samples failed: %s", fn, hipGetErrorString(hipGetLastError()));
        return TLC_ERR_HIP;
    }
    for (int j = 0; j < T; ++j)
        if (!std::isfinite(ts[j])) { tlc_set_error("%s: sample %d is NaN or Inf", fn, j); return TLC_ERR_INVALID_ARG; }
    if (H.offs[0] < 0) { tlc_set_error("%s: negative offset", fn); return TLC_ERR_INVALID_ARG; }
    for (size_t p = 0; p < B; ++p) {
        const long long n = H.offs[p + 1] - H.offs[p];
        if (n < 0) { tlc_set_error("%s: the offsets of diagram %lld decrease", fn, (long long)p); return TLC_ERR_INVALID_ARG; }
        if (n > max_points) {
            tlc_set_error("%s: diagram %lld has %lld points, max_points is %lld", fn, (long long)p, n, (long long)max_points);
            return TLC_ERR_INVALID_ARG;
        }
        if (n > LS_MAX_POINTS) { tlc_set_error("%s: diagram %lld has more than 2^27 points", fn, (long long)p); return TLC_ERR_UNSUPPORTED; }
        if (n <= LS_WAVE_N) ++H.n_wave;
        else if (n <= LS_LDS_N) { ++H.n_lds; H.max_lds = n > H.max_lds ? n : H.max_lds; }
        else ++H.n_wide;
    }
    return TLC_OK;
}

}  // namespace

extern "C" int64_t tlc_landscape_work_bytes(int32_t n_dgms, int64_t max_points, int32_t K, int32_t T, int64_t* least) {
    if (least) *least = 0;
    if (ls_check_sizes(__func__, n_dgms, T, K, max_points) != TLC_OK) return -1;
    const TlcLandscapeScratch S(max_points < LS_MAX_POINTS ? max_points : LS_MAX_POINTS, K, T, TlcCarver());
    if (least) *least = S.least;
    return S.total;
}

extern "C" int tlc_landscape(int32_t n_dgms, const int64_t* d_offs, const double* d_pts, int32_t T, const double* d_ts, int32_t K,
                             int64_t max_points, double* d_out, int32_t* d_winner, uint8_t* d_status, void* d_work, int64_t work_bytes,
                             void* stream) {
    const int rc = ls_check_sizes(__func__, n_dgms, T, K, max_points);
    if (rc != TLC_OK) return rc;
    TLC_REQUIRE(work_bytes >= 0, "negative size");
    if (n_dgms == 0) return TLC_OK;
    TLC_REQUIRE(d_offs && d_ts && d_out && d_status, "null pointer");
    TLC_REQUIRE(max_points == 0 || d_pts, "null pointer");
    const TlcLandscapeScratch S(max_points < LS_MAX_POINTS ? max_points : LS_MAX_POINTS, K, T, TlcCarver());
    if (work_bytes < S.least || (S.least > 0 && !d_work)) {
        if (!d_work && work_bytes >= S.least) tlc_set_error("%s: null pointer", __func__);
        else tlc_set_error("%s: d_work holds %lld bytes; a diagram of %lld points needs %lld (tlc_landscape_work_bytes)", __func__,
                           (long long)work_bytes, (long long)max_points, (long long)S.least);
        return TLC_ERR_INVALID_ARG;
    }
    hipStream_t st = (hipStream_t)stream;
    LsHost H;
    const int rb = ls_read_back(__func__, H, n_dgms, d_offs, T, d_ts, max_points, st);
    if (rb != TLC_OK) return rb;
    const LsArgs A{n_dgms, (const long long*)d_offs, d_pts, T, d_ts, K, d_out, d_winner, d_status};
    char* w = d_work ? tlc_align256(d_work) : nullptr;
    int lr;
    if (K <= 1) lr = ls_launch<1>(A, H.offs, H.n_wave, H.n_lds, H.n_wide, H.max_lds, w, work_bytes, S, st);
    else if (K <= 2) lr = ls_launch<2>(A, H.offs, H.n_wave, H.n_lds, H.n_wide, H.max_lds, w, work_bytes, S, st);
    else if (K <= 4) lr = ls_launch<4>(A, H.offs, H.n_wave, H.n_lds, H.n_wide, H.max_lds, w, work_bytes, S, st);
    else if (K <= 8) lr = ls_launch<8>(A, H.offs, H.n_wave, H.n_lds, H.n_wide, H.max_lds, w, work_bytes, S, st);
    else lr = ls_launch<16>(A, H.offs, H.n_wave, H.n_lds, H.n_wide, H.max_lds, w, work_bytes, S, st);
    if (lr != TLC_OK) {
        tlc_set_error("%s: clearing the control word failed: %s", __func__, hipGetErrorString(hipGetLastError()));
        return lr;
    }
    TLC_HIP_CHECK(hipGetLastError());
    return TLC_OK;
}

extern "C" int tlc_landscape_vjp(int32_t n_dgms, const int64_t* d_offs, const double* d_pts, int32_t T, const double* d_ts, int32_t K,
                                 int64_t max_points, const int32_t* d_winner, const double* d_grad_out, double* d_grad_pts, void* stream) {
    const int rc = ls_check_sizes(__func__, n_dgms, T, K, max_points);
    if (rc != TLC_OK) return rc;
    if (n_dgms == 0) return TLC_OK;
    TLC_REQUIRE(d_offs && d_ts && d_winner && d_grad_out, "null pointer");
    TLC_REQUIRE(max_points == 0 || (d_pts && d_grad_pts), "null pointer");
    hipStream_t st = (hipStream_t)stream;
    LsHost H;
    const int rb = ls_read_back(__func__, H, n_dgms, d_offs, T, d_ts, max_points, st);
    if (rb != TLC_OK) return rb;
    const LsVjpArgs A{n_dgms, (const long long*)d_offs, d_pts, T, d_ts, K, d_winner, d_grad_out, d_grad_pts};
    if (H.n_wave) hipLaunchKernelGGL(ls_vjp_wave_kernel, dim3(ls_grid(((long long)n_dgms + LS_WAVES - 1) / LS_WAVES)), dim3(LS_BS), 0, st, A);
    if (H.n_lds) hipLaunchKernelGGL(ls_vjp_block_kernel, dim3(ls_grid((long long)n_dgms * (LS_LDS_N / LS_BS))), dim3(LS_BS), 0, st, A, -1ll);
    if (H.n_wide)
        for (long long p = 0; p < n_dgms; ++p) {
            const long long n = H.offs[p + 1] - H.offs[p];
            if (n > LS_LDS_N) hipLaunchKernelGGL(ls_vjp_block_kernel, dim3(ls_grid((n + LS_BS - 1) / LS_BS)), dim3(LS_BS), 0, st, A, p);
        }
    TLC_HIP_CHECK(hipGetLastError());
    return TLC_OK;
}

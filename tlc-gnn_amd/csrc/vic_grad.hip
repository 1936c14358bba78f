// vic_grad.hip -- what the vicinity images need to be differentiable in the GRAPH's edge weights (include/tlcgnn.h).
//
//   tlc_packed_edge_lookup     packed vicinity edge -> its edge of the graph (binary search in the sorted edge list), pair endpoints ->
//                              their local ids; a wavefront per vicinity
//   tlc_segment_index          item keys -> the items of every key, ascending by position (a stable radix sort through radix_passes.h)
//   tlc_segment_sum_f64        out[k] = the sum of val over key k's items: the adjoint of the gather w[eid], a CSR row sum whose rows
//                              run from empty to tens of thousands of entries.  Three classes by the row's length, cut on the device.
//   tlc_lp_decode_bwd_pi_f32   d loss / d PI of the link-prediction decoder
//
// fp64 sums, no fused multiply-add (-ffp-contract=off), no floating-point atomics: the order of every sum is fixed by the segment's
// length alone.  The only atomics are integer counts (LDS digits in the radix sort, the two list lengths of the segment sum).
#include "radix_passes.h"
#include "scratch_layouts.h"
#include "tlc_common.h"

namespace {

// ---- lookup -------------------------------------------------------------------------------------------------------------------------
// index of (lo, hi) in the list sorted ascending by (lo, hi), -1 if absent
__device__ __forceinline__ int vg_find_edge(const int2* __restrict__ ge, long long M, long long lo, long long hi) {
    long long a = 0, b = M;
    while (a < b) {
        const long long mid = (a + b) >> 1;
        const int2 e = ge[mid];
        if (e.x < lo || (e.x == lo && e.y < hi)) a = mid + 1;
        else b = mid;
    }
    if (a < M) {
        const int2 e = ge[a];
        if (e.x == lo && e.y == hi) return (int)a;
    }
    return -1;
}

// local id of the global id `want` in the ascending slice ids[0 .. n), -1 if absent
template <typename ID>
__device__ __forceinline__ int vg_find_id(const ID* __restrict__ ids, long long n, long long want) {
    long long a = 0, b = n;
    while (a < b) {
        const long long mid = (a + b) >> 1;
        if ((long long)ids[mid] < want) a = mid + 1;
        else b = mid;
    }
    return (a < n && (long long)ids[a] == want) ? (int)a : -1;
}

// A wavefront per vicinity (grid-stride).  Lanes take the vicinity's edges 64 at a time; lane 0 finds the roots; one ballot decides
// whether the vicinity is refused, and then the same lanes overwrite what they wrote.
template <typename ID>
__global__ __launch_bounds__(256) void vg_lookup_kernel(long long M, const int2* __restrict__ ge, long long B, const long long* __restrict__ node_ptr,
                                                        const long long* __restrict__ edge_ptr, const ID* __restrict__ ids,
                                                        const int2* __restrict__ edges, long long tot_n, long long tot_m,
                                                        const int2* __restrict__ pairs, int one_root, int* __restrict__ eid,
                                                        int2* __restrict__ roots, unsigned char* __restrict__ status) {
    const int lane = threadIdx.x & 63;
    const long long stride = (long long)gridDim.x * (blockDim.x >> 6);
    for (long long g = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); g < B; g += stride) {
        const long long a = node_ptr[g], b = node_ptr[g + 1], ea = edge_ptr[g], eb = edge_ptr[g + 1];
        const bool offs_ok = a >= 0 && b >= a && b <= tot_n && ea >= 0 && eb >= ea && eb <= tot_m && b - a < (1ll << 31);
        if (!offs_ok) {                                   // (no slice to speak of: nothing of eid is written)
            if (lane == 0) {
                status[g] = TLC_ST_BAD_INPUT;
                if (roots) roots[g] = make_int2(-1, -1);
            }
            continue;
        }
        const long long n = b - a;
        bool bad = false;
        for (long long e = ea + lane; e < eb; e += 64) {
            const int2 le = edges[e];
            int id = -1;
            if (le.x >= 0 && le.x < n && le.y >= 0 && le.y < n) {
                const long long ga = (long long)ids[a + le.x], gb = (long long)ids[a + le.y];
                id = vg_find_edge(ge, M, ga < gb ? ga : gb, ga < gb ? gb : ga);
            }
            eid[e] = id;
            bad |= id < 0;
        }
        int r0 = -1, r1 = -1;
        if (pairs && lane == 0) {
            const int2 p = pairs[g];
            r0 = vg_find_id(ids + a, n, p.x);
            r1 = one_root ? -1 : vg_find_id(ids + a, n, p.y);
            bad |= r0 < 0 || (!one_root && r1 < 0);
        }
        bad = __ballot(bad) != 0ull;
        if (bad)
            for (long long e = ea + lane; e < eb; e += 64) eid[e] = -1;
        if (lane == 0) {
            status[g] = bad ? TLC_ST_BAD_INPUT : TLC_ST_OK;
            if (roots) roots[g] = bad ? make_int2(-1, -1) : make_int2(r0, r1);
        }
    }
}

// ---- segment index ------------------------------------------------------------------------------------------------------------------
// sort key of item i: its key, or n_keys for an item that is skipped (a negative key, or one past the last); payload: i
__global__ __launch_bounds__(256) void vg_seg_keys_kernel(long long n, const int* __restrict__ key, long long n_keys, unsigned* __restrict__ k,
                                                          unsigned* __restrict__ pos) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int v = key[i];
        k[i] = (v < 0 || v >= n_keys) ? (unsigned)n_keys : (unsigned)v;
        pos[i] = (unsigned)i;
    }
}

// seg_ptr[q] = the first sorted position whose key is >= q, for q = 0 .. n_keys
__global__ __launch_bounds__(256) void vg_seg_ptr_kernel(long long n, const unsigned* __restrict__ sorted, long long n_keys,
                                                         long long* __restrict__ seg_ptr) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q <= n_keys; q += stride) {
        long long a = 0, b = n;
        while (a < b) {
            const long long mid = (a + b) >> 1;
            if ((long long)sorted[mid] < q) a = mid + 1;
            else b = mid;
        }
        seg_ptr[q] = a;
    }
}

// ---- segment sum --------------------------------------------------------------------------------------------------------------------
constexpr int SS_LANE_MAX = TLC_SEG_LANE_MAX, SS_WAVE_MAX = TLC_SEG_WAVE_MAX;
constexpr int SS_BS = 256;                            // threads of every kernel below; the workgroup class's stride

// item j of the segment that starts at `a`: val[seg_pos[a + j]]; a position outside 0 .. n_items-1 counts as +0.0
__device__ __forceinline__ double ss_item(const int* __restrict__ seg_pos, const double* __restrict__ val, long long n_items, long long at) {
    const int p = seg_pos[at];
    return (p >= 0 && p < n_items) ? val[p] : 0.0;
}

// the length of segment k; offsets out of order or outside 0 .. n_items make it empty
__device__ __forceinline__ long long ss_len(const long long* __restrict__ seg_ptr, long long n_items, long long k, long long* a) {
    const long long s = seg_ptr[k], e = seg_ptr[k + 1];
    *a = s;
    return (s >= 0 && e >= s && e <= n_items) ? e - s : 0;
}

// p = p + item, for the items at, at + step, ... below end, in that order; four loads in flight per trip
__device__ __forceinline__ double ss_strided(const int* __restrict__ seg_pos, const double* __restrict__ val, long long n_items, long long at,
                                             long long end, long long step) {
    double p = 0.0;
    for (; at + 3 * step < end; at += 4 * step) {
        const double v0 = ss_item(seg_pos, val, n_items, at), v1 = ss_item(seg_pos, val, n_items, at + step);
        const double v2 = ss_item(seg_pos, val, n_items, at + 2 * step), v3 = ss_item(seg_pos, val, n_items, at + 3 * step);
        p = p + v0;
        p = p + v1;
        p = p + v2;
        p = p + v3;
    }
    for (; at < end; at += step) p = p + ss_item(seg_pos, val, n_items, at);
    return p;
}

// the fold of a wavefront's 64 partials: for d = 32, 16, 8, 4, 2, 1: p[l] = p[l] + p[l + d] for l < d.  As a butterfly every lane below
// d holds that value after step d (a + b == b + a bit for bit), and lane 0 holds the result.
__device__ __forceinline__ double ss_wave_fold(double p) {
    p = p + tlc_lane_xor_f64<32>(p);
    p = p + tlc_lane_xor_f64<16>(p);
    p = p + tlc_lane_xor_f64<8>(p);
    p = p + tlc_lane_xor_f64<4>(p);
    p = p + tlc_lane_xor_f64<2>(p);
    p = p + tlc_lane_xor_f64<1>(p);
    return p;
}

// A thread per segment: the lane class is summed here; the others are appended to their class's list (one integer atomic per
// wavefront and class; the lists' order does not reach any sum).
__global__ __launch_bounds__(SS_BS) void ss_lane_kernel(long long n_keys, const long long* __restrict__ seg_ptr, const int* __restrict__ seg_pos,
                                                        long long n_items, const double* __restrict__ val, double* __restrict__ out,
                                                        int* __restrict__ counts, int* __restrict__ wave_list, int* __restrict__ wg_list) {
    const int lane = threadIdx.x & 63;
    const unsigned long long lt = (1ull << lane) - 1ull;
    const long long stride = (long long)gridDim.x * SS_BS;
    // (whole wavefronts stay in the loop together: k0 is the wavefront's first segment)
    for (long long k0 = (long long)blockIdx.x * SS_BS + (threadIdx.x & ~63); k0 < n_keys; k0 += stride) {
        const long long k = k0 + lane;
        long long a = 0, L = -1;
        if (k < n_keys) L = ss_len(seg_ptr, n_items, k, &a);
        if (L >= 0 && L <= SS_LANE_MAX) {
            double s = 0.0;
            for (long long j = 0; j < L; ++j) s = s + ss_item(seg_pos, val, n_items, a + j);
            out[k] = s;
        }
        const bool is_wave = L > SS_LANE_MAX && L <= SS_WAVE_MAX, is_wg = L > SS_WAVE_MAX;
        const unsigned long long mw = __ballot(is_wave), mg = __ballot(is_wg);
        if (mw) {
            int base = 0;
            if (lane == 0) base = atomicAdd(&counts[0], __popcll(mw));
            base = __builtin_amdgcn_readfirstlane(base);
            if (is_wave) wave_list[base + __popcll(mw & lt)] = (int)k;
        }
        if (mg) {
            int base = 0;
            if (lane == 0) base = atomicAdd(&counts[1], __popcll(mg));
            base = __builtin_amdgcn_readfirstlane(base);
            if (is_wg) wg_list[base + __popcll(mg & lt)] = (int)k;
        }
    }
}

// A wavefront per listed segment (grid-stride over the list): lane l adds the items l, l + 64, ... from +0.0, then the fold.
__global__ __launch_bounds__(SS_BS) void ss_wave_kernel(const int* __restrict__ counts, const int* __restrict__ list, const long long* __restrict__ seg_ptr,
                                                        const int* __restrict__ seg_pos, long long n_items, const double* __restrict__ val,
                                                        double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int n_list = counts[0];
    const int stride = (int)gridDim.x * (SS_BS / 64);
    for (int q = (int)blockIdx.x * (SS_BS / 64) + (threadIdx.x >> 6); q < n_list; q += stride) {
        const long long k = list[q];
        long long a;
        const long long L = ss_len(seg_ptr, n_items, k, &a);
        const double p = ss_wave_fold(ss_strided(seg_pos, val, n_items, a + lane, a + L, 64));
        if (lane == 0) out[k] = p;
    }
}

// A workgroup per listed segment: thread t adds the items t, t + 256, ... from +0.0; every wavefront folds its 64 partials; the four
// wavefront totals are added in wavefront order.
__global__ __launch_bounds__(SS_BS) void ss_wg_kernel(const int* __restrict__ counts, const int* __restrict__ list, const long long* __restrict__ seg_ptr,
                                                      const int* __restrict__ seg_pos, long long n_items, const double* __restrict__ val,
                                                      double* __restrict__ out) {
    __shared__ double q_w[SS_BS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n_list = counts[1];
    for (int q = blockIdx.x; q < n_list; q += gridDim.x) {
        const long long k = list[q];
        long long a;
        const long long L = ss_len(seg_ptr, n_items, k, &a);
        const double p = ss_wave_fold(ss_strided(seg_pos, val, n_items, a + threadIdx.x, a + L, SS_BS));
        if (lane == 0) q_w[wave] = p;
        __syncthreads();
        if (threadIdx.x == 0) {
            double s = q_w[0] + q_w[1];
            s = s + q_w[2];
            s = s + q_w[3];
            out[k] = s;
        }
        __syncthreads();
    }
}

// ---- d loss / d PI of the decoder ---------------------------------------------------------------------------------------------------
// A thread per pair: the forward of the fused decode recomputed as lp_decode_bwd_kernel (lp_backward.hip) does, its pre-activation
// gradient gz[k] (parked in LDS, column = thread), then d_gpi[i][j] = sum over k ascending of W1[k][16 + j] * gz[k], from +0.0.
constexpr int DP_ED = 16, DP_PD = 25, DP_IN = DP_ED + DP_PD, DP_T = 128, DP_S = DP_T + 1;

__global__ __launch_bounds__(DP_T) void lp_decode_bwd_pi_kernel(long long n_pairs, const int* __restrict__ pairs, const float* __restrict__ emb,
                                                                const float* __restrict__ pi, const float* __restrict__ W1,
                                                                const float* __restrict__ b1, const float* __restrict__ W2,
                                                                const float* __restrict__ b2, const float* __restrict__ gprob,
                                                                int n_nodes, float* __restrict__ gpi) {
    __shared__ float s_h[DP_PD][DP_S];
    const int t = threadIdx.x;
    const long long i = (long long)blockIdx.x * DP_T + t;
    if (i >= n_pairs) return;                             // (no barrier below: every thread works on its own LDS column)
    float in[DP_IN];
    {
        const int u = pairs[2 * i], v = pairs[2 * i + 1];
        if (u < 0 || u >= n_nodes || v < 0 || v >= n_nodes) {            // (no row to read: the pair's gradient is zeros)
            for (int j = 0; j < DP_PD; ++j) gpi[(size_t)i * DP_PD + j] = 0.0f;
            return;
        }
        const float* eu = emb + (size_t)u * DP_ED;
        const float* ev = emb + (size_t)v * DP_ED;
#pragma unroll
        for (int c = 0; c < DP_ED; ++c) {
            const float d = eu[c] - ev[c];
            in[c] = d * d;
        }
#pragma unroll
        for (int c = 0; c < DP_PD; ++c) in[DP_ED + c] = pi[(size_t)i * DP_PD + c];
    }
    float d = b2[0];
#pragma unroll 1
    for (int o = 0; o < DP_PD; ++o) {
        float acc = b1[o];
#pragma unroll
        for (int k = 0; k < DP_IN; ++k) acc += W1[o * DP_IN + k] * in[k];
        s_h[o][t] = acc;
        d += W2[o] * (acc > 0.0f ? acc : 0.2f * acc);
    }
    const float ad = fabsf(d);
    const float c = ad > 40.0f ? 40.0f : ad;
    const float ez = expf((c - 2.0f) / 1.0f);
    const float p = 1.0f / (ez + 1.0f);
    const float gz = -gprob[i] * (p * p) * ez;           // d/dz of 1 / (exp(z) + 1)
    const float sg = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
    const float dd = (ad >= 0.0f && ad <= 40.0f) ? gz * sg : 0.0f;
#pragma unroll 1
    for (int o = 0; o < DP_PD; ++o) {
        const float h = s_h[o][t];
        s_h[o][t] = (dd * W2[o]) * (h > 0.0f ? 1.0f : 0.2f);
    }
#pragma unroll 1
    for (int j = 0; j < DP_PD; ++j) {
        float acc = 0.0f;
#pragma unroll
        for (int k = 0; k < DP_PD; ++k) acc += W1[k * DP_IN + DP_ED + j] * s_h[k][t];
        gpi[(size_t)i * DP_PD + j] = acc;
    }
}

}  // namespace

// ======================================================================================================================
// C ABI
// ======================================================================================================================
extern "C" int tlc_packed_edge_lookup(int64_t n_graph_edges, const int32_t* d_graph_edges, int64_t n_vicinities, const int64_t* d_node_ptr,
                                      const int64_t* d_edge_ptr, const void* d_ids, int32_t ids_int64, const int32_t* d_edges,
                                      int64_t total_nodes, int64_t total_edges, const int32_t* d_pairs, int32_t one_root, int32_t* d_eid,
                                      int32_t* d_roots, uint8_t* d_status, void* stream) {
    TLC_REQUIRE(n_graph_edges >= 0 && n_vicinities >= 0 && total_nodes >= 0 && total_edges >= 0, "negative size");
    TLC_REQUIRE(n_graph_edges < (1ll << 31) && total_edges < (1ll << 31), "2^31 edges or more");
    TLC_REQUIRE((ids_int64 == 0 || ids_int64 == 1) && (one_root == 0 || one_root == 1), "ids_int64 / one_root is 0 or 1");
    if (n_vicinities == 0) return TLC_OK;
    TLC_REQUIRE(d_node_ptr && d_edge_ptr && d_status, "null pointer");
    TLC_REQUIRE(n_graph_edges == 0 || d_graph_edges, "null edge list");
    TLC_REQUIRE(total_nodes == 0 || d_ids, "null ids");
    TLC_REQUIRE(total_edges == 0 || (d_edges && d_eid), "null packed edges / eid");
    TLC_REQUIRE((d_pairs == nullptr) == (d_roots == nullptr), "d_pairs and d_roots go together");
    hipStream_t s = (hipStream_t)stream;
    const unsigned grid = tlc_grid_for(n_vicinities, 4, 8192);
    if (ids_int64)
        hipLaunchKernelGGL(vg_lookup_kernel<long long>, dim3(grid), dim3(256), 0, s, (long long)n_graph_edges, (const int2*)d_graph_edges,
                           (long long)n_vicinities, (const long long*)d_node_ptr, (const long long*)d_edge_ptr, (const long long*)d_ids,
                           (const int2*)d_edges, (long long)total_nodes, (long long)total_edges, (const int2*)d_pairs, (int)one_root, d_eid,
                           (int2*)d_roots, d_status);
    else
        hipLaunchKernelGGL(vg_lookup_kernel<int>, dim3(grid), dim3(256), 0, s, (long long)n_graph_edges, (const int2*)d_graph_edges,
                           (long long)n_vicinities, (const long long*)d_node_ptr, (const long long*)d_edge_ptr, (const int*)d_ids,
                           (const int2*)d_edges, (long long)total_nodes, (long long)total_edges, (const int2*)d_pairs, (int)one_root, d_eid,
                           (int2*)d_roots, d_status);
    TLC_HIP_CHECK(hipGetLastError());
    return TLC_OK;
}

extern "C" int tlc_segment_index_work_bytes(int64_t n_items, int64_t n_keys, int64_t* bytes) {
    TLC_REQUIRE(bytes, "null pointer");
    TLC_REQUIRE(n_items >= 0 && n_keys >= 0 && n_items < (1ll << 31) && n_keys < (1ll << 31), "sizes outside 0 .. 2^31 - 1");
    *bytes = TlcSegmentIndexScratch(n_items, rk_hist_ints(n_items), RK_TOT_INTS).total;
    return TLC_OK;
}

extern "C" int tlc_segment_index(int64_t n_items, const int32_t* d_key, int64_t n_keys, int64_t* d_seg_ptr, int32_t* d_seg_pos, void* d_work,
                                 int64_t work_bytes, void* stream) {
    TLC_REQUIRE(n_items >= 0 && n_keys >= 0 && n_items < (1ll << 31) && n_keys < (1ll << 31), "sizes outside 0 .. 2^31 - 1");
    TLC_REQUIRE(d_seg_ptr && (n_items == 0 || (d_key && d_seg_pos)), "null pointer");
    const TlcSegmentIndexScratch L(n_items, rk_hist_ints(n_items), RK_TOT_INTS);
    TLC_REQUIRE(n_items == 0 || (d_work && work_bytes >= L.total), "d_work below tlc_segment_index_work_bytes");
    TLC_REQUIRE((reinterpret_cast<uintptr_t>(d_work) & 255) == 0, "d_work not 256-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    char* w = (char*)d_work;
    unsigned *ka = nullptr, *pa = (unsigned*)d_seg_pos;
    if (n_items > 0) {
        ka = (unsigned*)(w + L.key_a);
        unsigned *kb = (unsigned*)(w + L.key_b), *pb = (unsigned*)(w + L.pos_b);
        int *hist = (int*)(w + L.hist), *tot = (int*)(w + L.tot);
        hipLaunchKernelGGL(vg_seg_keys_kernel, dim3(tlc_grid_for(n_items, 256, 4096)), dim3(256), 0, s, (long long)n_items, d_key,
                           (long long)n_keys, ka, pa);
        // the keys are 0 .. n_keys: two digits where they fit, else four; stable, so a key's items stay in ascending position
        if (n_keys <= 0xFFFF) rk_sort<16>(s, (long long)n_items, ka, kb, pa, pb, hist, tot);
        else rk_sort<32>(s, (long long)n_items, ka, kb, pa, pb, hist, tot);
    }
    hipLaunchKernelGGL(vg_seg_ptr_kernel, dim3(tlc_grid_for(n_keys + 1, 256, 4096)), dim3(256), 0, s, (long long)n_items, (const unsigned*)ka,
                       (long long)n_keys, (long long*)d_seg_ptr);
    TLC_HIP_CHECK(hipGetLastError());
    return TLC_OK;
}

extern "C" int tlc_segment_sum_work_bytes(int64_t n_keys, int64_t* bytes) {
    TLC_REQUIRE(bytes, "null pointer");
    TLC_REQUIRE(n_keys >= 0 && n_keys < (1ll << 31), "n_keys outside 0 .. 2^31 - 1");
    *bytes = TlcSegmentSumScratch(n_keys).total;
    return TLC_OK;
}

extern "C" int tlc_segment_sum_f64(int64_t n_keys, const int64_t* d_seg_ptr, const int32_t* d_seg_pos, int64_t n_items, const double* d_val,
                                   double* d_out, void* d_work, int64_t work_bytes, void* stream) {
    TLC_REQUIRE(n_keys >= 0 && n_keys < (1ll << 31) && n_items >= 0 && n_items < (1ll << 31), "sizes outside 0 .. 2^31 - 1");
    if (n_keys == 0) return TLC_OK;
    TLC_REQUIRE(d_seg_ptr && d_out && (n_items == 0 || (d_seg_pos && d_val)), "null pointer");
    const TlcSegmentSumScratch L(n_keys);
    TLC_REQUIRE(d_work && work_bytes >= L.total, "d_work below tlc_segment_sum_work_bytes");
    TLC_REQUIRE((reinterpret_cast<uintptr_t>(d_work) & 255) == 0, "d_work not 256-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    char* w = (char*)d_work;
    int *counts = (int*)(w + L.head), *wave_list = (int*)(w + L.wave_list), *wg_list = (int*)(w + L.wg_list);
    TLC_HIP_CHECK(hipMemsetAsync(counts, 0, 2 * sizeof(int), s));
    hipLaunchKernelGGL(ss_lane_kernel, dim3(tlc_grid_for(n_keys, SS_BS, 4096)), dim3(SS_BS), 0, s, (long long)n_keys, (const long long*)d_seg_ptr,
                       d_seg_pos, (long long)n_items, d_val, d_out, counts, wave_list, wg_list);
    // the lists' lengths stay on the device: both grids are sized by n_keys and stride over what the lists hold
    hipLaunchKernelGGL(ss_wave_kernel, dim3(tlc_grid_for(n_keys, SS_BS / 64, 8192)), dim3(SS_BS), 0, s, (const int*)counts, (const int*)wave_list,
                       (const long long*)d_seg_ptr, d_seg_pos, (long long)n_items, d_val, d_out);
    hipLaunchKernelGGL(ss_wg_kernel, dim3(tlc_grid_for(n_keys, 1, 2048)), dim3(SS_BS), 0, s, (const int*)counts, (const int*)wg_list,
                       (const long long*)d_seg_ptr, d_seg_pos, (long long)n_items, d_val, d_out);
    TLC_HIP_CHECK(hipGetLastError());
    return TLC_OK;
}

extern "C" int tlc_lp_decode_bwd_pi_f32(int64_t n_pairs, const int32_t* d_pairs, const float* d_emb_pre, const float* d_emb, int32_t n_nodes,
                                        int32_t emb_dim, const float* d_pi, int32_t pi_dim, const float* d_W1, const float* d_b1,
                                        const float* d_W2, const float* d_b2, const float* d_gprob, float* d_gpi, void* stream) {
    (void)d_emb_pre;                                      // (the renorm lies in front of the embedding, not of the images)
    TLC_REQUIRE(n_pairs >= 0 && n_nodes >= 1, "bad sizes");
    if (emb_dim != DP_ED || pi_dim != DP_PD) {
        tlc_set_error("tlc_lp_decode_bwd_pi_f32: emb_dim %d / pi_dim %d: only 16 / 25 (TLCGNN's conv2 width, dimension 5) is built", emb_dim, pi_dim);
        return TLC_ERR_UNSUPPORTED;
    }
    TLC_REQUIRE(n_pairs <= (1ll << 30), "more than 2^30 pairs");
    if (n_pairs == 0) return TLC_OK;
    TLC_REQUIRE(d_pairs && d_emb && d_pi && d_W1 && d_b1 && d_W2 && d_b2 && d_gprob && d_gpi, "null pointer");
    hipLaunchKernelGGL(lp_decode_bwd_pi_kernel, dim3((unsigned)((n_pairs + DP_T - 1) / DP_T)), dim3(DP_T), 0, (hipStream_t)stream,
                       (long long)n_pairs, d_pairs, d_emb, d_pi, d_W1, d_b1, d_W2, d_b2, d_gprob, (int)n_nodes, d_gpi);
    TLC_HIP_CHECK(hipGetLastError());
    return TLC_OK;
}

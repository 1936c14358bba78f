// lp_backward.hip -- the backward half of the TLCGNN link-prediction step (pipelines.py:10-18: loss.backward()).
//
//   tlc_gemm_tn_f32       C = A^T B for a long K on the f32 MFMA (v_mfma_f32_16x16x4_f32), split-K with a fixed-order
//                         reduction: dW = X^T d(XW) of GCNConv; with d_A NULL the column sums 1^T B (the bias gradients)
//   tlc_lp_decode_bwd_f32 the backward of tlc_lp_decode_fused_f32 and of the emb.renorm_(2, 0, 1) in front of it
//                         (TLCGNN.py:48-61): per-pair endpoint gradients, the two Linear layers' gradients, d emb
//
// Like the forward (lp_forward.hip): no atomics.  Every sum runs in an order fixed by the shapes alone, so the same inputs give
// bit-identical gradients on every call.  (A^T G of the GCN layer is tlc_spmm_csr_f32 over the transposed operator,
// tlc_gcn_norm_csr_t, which lives next to the forward operator's build in lp_forward.hip.)
#include "tlc_common.h"
#include "scratch_layouts.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// compensated (Kahan) addition: s + c carries the sum; the weight gradients add hundreds of O(1) terms per output whose total
// may be small, and a plain fp32 running sum loses ~n eps |term| there.  (No reassociation: -fno-fast-math.)
__device__ __forceinline__ void kahan_add(float& s, float& c, float v) {
    const float y = v - c;
    const float t = s + y;
    c = (t - s) - y;
    s = t;
}

// ---- fixed-order sum of partials ---------------------------------------------------------------------------------------------
// out[o] = sum_p part[p][o]: workgroup (64, SP_R) -- 64 outputs, SP_R strided runs over the partials (run r takes p = r, r + SP_R,
// ... in ascending order), the SP_R run totals then added in run order through LDS.  The order depends on n_part alone.
#define SP_R 16
__global__ __launch_bounds__(64 * SP_R) void sum_partials_kernel(long long n_out, int n_part, const float* __restrict__ part,
                                                                 float* __restrict__ out) {
    __shared__ float s[SP_R][64];
    const int tx = threadIdx.x & 63, r = threadIdx.x >> 6;
    const long long o = (long long)blockIdx.x * 64 + tx;
    float acc = 0.0f, cmp = 0.0f;
    if (o < n_out)
        for (int p = r; p < n_part; p += SP_R) kahan_add(acc, cmp, part[(size_t)p * n_out + o]);
    s[r][tx] = acc - cmp;
    __syncthreads();
    if (r == 0 && o < n_out) {
        float t = s[0][tx], tc = 0.0f;
#pragma unroll
        for (int q = 1; q < SP_R; ++q) kahan_add(t, tc, s[q][tx]);
        out[o] = t - tc;
    }
}

// ---- C[M,N] = A[K,M]^T B[K,N] -------------------------------------------------------------------------------------------------
// Workgroup = 4 wavefronts on one 32 x 64 tile of C and one K range (blockIdx.z of gridDim.z splits).  The MFMA operands come
// straight from global memory, no LDS: lane (l16, g) of a 16x16x4 step at k0 holds A^T[m][k0 + g] = A[k0 + g][m] (m = l16 of the
// row tile) and B[k0 + g][n] (n = l16 of the column tile) -- 16 consecutive floats of one row per lane group, and each operand
// feeds two (A) or four (B) MFMAs.  Wavefront w takes the 4-row steps w, w + 4, w + 8, ... of the range; the four wavefront tiles
// are added in wavefront order through LDS.  Rows past K, columns past M / N read as zeros (ONES: A is a column of ones, M = 1).
// One split: the tile goes to C; more: to part[split] for sum_partials_kernel.
#define TN_BM 32
#define TN_BN 64
template <bool ONES>
__global__ __launch_bounds__(256) void gemm_tn_kernel(int M, int N, long long K, long long k_per_split, const float* __restrict__ A,
                                                      const float* __restrict__ B, float* __restrict__ out) {
    __shared__ float red[3][TN_BM][TN_BN + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l16 = lane & 15, g = lane >> 4;
    const int m0 = blockIdx.x * TN_BM, n0 = blockIdx.y * TN_BN;
    const long long kb = (long long)blockIdx.z * k_per_split;
    const long long ke = kb + k_per_split < K ? kb + k_per_split : K;
    const int ma[2] = {m0 + l16, m0 + 16 + l16};
    const bool va[2] = {ma[0] < M, ma[1] < M};
    int nb[4];
    bool vb[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        nb[j] = n0 + 16 * j + l16;
        vb[j] = nb[j] < N;
    }
    f32x4 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    // four steps per trip, every load of the four requested before the first MFMA (one step per trip waits a full memory
    // round trip per step)
    for (long long k0 = kb + 4 * wave; k0 < ke; k0 += 64) {
        float a[4][2], b[4][4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long long k = k0 + 16 * u + g;
            const bool vk = k < ke;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                if (ONES) a[u][i] = (vk && va[i]) ? 1.0f : 0.0f;
                else a[u][i] = (vk && va[i]) ? A[(size_t)k * M + ma[i]] : 0.0f;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) b[u][j] = (vk && vb[j]) ? B[(size_t)k * N + nb[j]] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][i], b[u][j], acc[i][j], 0, 0, 0);
    }
    // C/D layout: column l16, row 4 g + reg.  Wavefronts 1..3 park their tiles, wavefront 0 adds them in order and stores.
    if (wave > 0) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) red[wave - 1][16 * i + 4 * g + r][16 * j + l16] = acc[i][j][r];
    }
    __syncthreads();
    if (wave == 0) {
        float* dst = out + (size_t)blockIdx.z * M * N;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int rr = 16 * i + 4 * g + r, cc = 16 * j + l16;
                    float v = acc[i][j][r];
                    v += red[0][rr][cc];
                    v += red[1][rr][cc];
                    v += red[2][rr][cc];
                    const int m = m0 + rr, n = n0 + cc;
                    if (m < M && n < N) dst[(size_t)m * N + n] = v;
                }
    }
}

// splits of tlc_gemm_tn_f32: enough workgroups to cover the CUs twice over (512), at least 256 rows of K per split, at most
// TN_MAX_SPLITS (the scratch the caller provides)
constexpr int TN_MAX_SPLITS = TlcGemmTnScratch::MAX_SPLITS;
int gemm_tn_splits(int M, int N, long long K) {
    const long long tiles = (long long)((M + TN_BM - 1) / TN_BM) * ((N + TN_BN - 1) / TN_BN);
    long long s = (512 + tiles - 1) / tiles;
    const long long by_k = (K + 255) / 256;
    if (by_k < s) s = by_k;
    if (s > TN_MAX_SPLITS) s = TN_MAX_SPLITS;
    return s < 1 ? 1 : (int)s;
}

// ---- decoder backward ------------------------------------------------------------------------------------------------------------
// One thread per pair (DB_T pairs per tile, one tile at a time per workgroup, grid-stride over the tiles): the forward of
// lp_decode_mfma_kernel recomputed from the renormalised rows (in = (e_u - e_v)^2 || PI, h = W1 in + b1, LeakyReLU(0.2),
// d = W2 . lh + b2, |.|, clamp to [0, 40], Fermi-Dirac), then torch's backward of each of those ops:
//   p = 1 / (exp(z) + 1), z = (c - 2) / 1     dz = -gp p^2 exp(z)     (reciprocal, exp)
//   c = clamp(|d|, 0, 40)                     passes where 0 <= |d| <= 40
//   |d|                                       times sign(d), 0 at 0
//   lh = LeakyReLU(h)                         dh = dlh (h > 0 ? 1 : 0.2)
//   in_c = (e_u - e_v)_c^2                    d e_u = d in_c 2 (e_u - e_v)_c = -d e_v
// The pair's d e_u (16 floats; d e_v is its negation) goes to gpair[i].  The weight gradients of the tile meet in LDS (column t =
// the tile's pair t: in, dh, lh, dd) and every thread adds up its outputs over the tile's pairs in order t = 0, 1, ... (compensated
// sums); the workgroup's sums over its tiles (ascending) are its partial, part[wg][DB_NW], summed by sum_partials_kernel.
// Output q of the DB_NW: [0, PD*IN) dW1 row-major | [.., + PD) db1 | [.., + PD) dW2 | db2.
constexpr int DB_ED = 16, DB_PD = 25, DB_IN = DB_ED + DB_PD;
constexpr int DB_NW = DB_PD * DB_IN + 2 * DB_PD + 1;             // 1076
constexpr int DB_T = 128, DB_S = DB_T + 1;                        // pairs per tile; LDS row stride (rows on distinct banks)
constexpr int DB_Q = (DB_NW + DB_T - 1) / DB_T;                   // outputs per thread
constexpr int DB_MAX_WG = TlcLpDecodeBwdScratch::MAX_WG;
static_assert(DB_ED == TlcLpDecodeBwdScratch::ED && DB_NW == TlcLpDecodeBwdScratch::NW, "the row widths of scratch_layouts.h");

__global__ __launch_bounds__(DB_T) void lp_decode_bwd_kernel(long long n_pairs, const int* __restrict__ pairs, const float* __restrict__ emb,
                                                             const float* __restrict__ pi, const float* __restrict__ W1,
                                                             const float* __restrict__ b1, const float* __restrict__ W2,
                                                             const float* __restrict__ b2, const float* __restrict__ gprob,
                                                             float* __restrict__ gpair, float* __restrict__ part) {
    __shared__ float s_in[DB_IN][DB_S];
    __shared__ float s_dh[DB_PD][DB_S];
    __shared__ float s_lh[DB_PD][DB_S];
    __shared__ float s_dd[DB_S];
    const int t = threadIdx.x;
    float wacc[DB_Q], wcmp[DB_Q];
#pragma unroll
    for (int s = 0; s < DB_Q; ++s) wacc[s] = wcmp[s] = 0.0f;
    const long long n_tiles = (n_pairs + DB_T - 1) / DB_T;
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long long i = tile * DB_T + t;
        const bool live = i < n_pairs;
        float in[DB_IN], diff[DB_ED];
        float dd = 0.0f;
        if (live) {
            const int u = pairs[2 * i], v = pairs[2 * i + 1];
            const float4* eu = reinterpret_cast<const float4*>(emb + (size_t)u * DB_ED);
            const float4* ev = reinterpret_cast<const float4*>(emb + (size_t)v * DB_ED);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 a = eu[q], b = ev[q];
                diff[4 * q] = a.x - b.x; diff[4 * q + 1] = a.y - b.y; diff[4 * q + 2] = a.z - b.z; diff[4 * q + 3] = a.w - b.w;
            }
#pragma unroll
            for (int c = 0; c < DB_ED; ++c) in[c] = diff[c] * diff[c];
#pragma unroll
            for (int c = 0; c < DB_PD; ++c) in[DB_ED + c] = pi[(size_t)i * DB_PD + c];
        } else {
#pragma unroll
            for (int c = 0; c < DB_ED; ++c) diff[c] = 0.0f;
#pragma unroll
            for (int k = 0; k < DB_IN; ++k) in[k] = 0.0f;
        }
        // hidden layer, one unit at a time (the weights are the same for every lane: scalar loads); h parks in s_lh
        float d = b2[0];
#pragma unroll 1
        for (int o = 0; o < DB_PD; ++o) {
            float acc = b1[o];
#pragma unroll
            for (int k = 0; k < DB_IN; ++k) acc += W1[o * DB_IN + k] * in[k];
            s_lh[o][t] = acc;
            d += W2[o] * (acc > 0.0f ? acc : 0.2f * acc);
        }
        if (live) {
            const float ad = fabsf(d);
            const float c = ad < 0.0f ? 0.0f : (ad > 40.0f ? 40.0f : ad);
            const float ez = expf((c - 2.0f) / 1.0f);
            const float p = 1.0f / (ez + 1.0f);
            const float gz = -gprob[i] * (p * p) * ez;                 // d/dz of 1 / (exp(z) + 1)
            const float gc = gz / 1.0f;
            const float sg = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
            dd = (ad >= 0.0f && ad <= 40.0f) ? gc * sg : 0.0f;
        }
        float gin[DB_ED];
#pragma unroll
        for (int c = 0; c < DB_ED; ++c) gin[c] = 0.0f;
#pragma unroll 1
        for (int o = 0; o < DB_PD; ++o) {
            const float h = s_lh[o][t];
            const float dh = (dd * W2[o]) * (h > 0.0f ? 1.0f : 0.2f);
            s_dh[o][t] = dh;
            s_lh[o][t] = h > 0.0f ? h : 0.2f * h;
#pragma unroll
            for (int c = 0; c < DB_ED; ++c) gin[c] += dh * W1[o * DB_IN + c];
        }
#pragma unroll
        for (int k = 0; k < DB_IN; ++k) s_in[k][t] = in[k];
        s_dd[t] = dd;
        if (live) {
            float4* gp = reinterpret_cast<float4*>(gpair + (size_t)i * DB_ED);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float4 w;
                w.x = gin[4 * q] * (2.0f * diff[4 * q]);
                w.y = gin[4 * q + 1] * (2.0f * diff[4 * q + 1]);
                w.z = gin[4 * q + 2] * (2.0f * diff[4 * q + 2]);
                w.w = gin[4 * q + 3] * (2.0f * diff[4 * q + 3]);
                gp[q] = w;
            }
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < DB_Q; ++s) {
            const int q = t + DB_T * s;
            if (q < DB_PD * DB_IN) {
                const int o = q / DB_IN, k = q - o * DB_IN;
                float a = 0.0f, ac = 0.0f;
#pragma unroll 8
                for (int j = 0; j < DB_T; ++j) kahan_add(a, ac, s_dh[o][j] * s_in[k][j]);
                kahan_add(wacc[s], wcmp[s], a - ac);
            } else if (q < DB_PD * DB_IN + DB_PD) {
                const int o = q - DB_PD * DB_IN;
                float a = 0.0f, ac = 0.0f;
#pragma unroll 8
                for (int j = 0; j < DB_T; ++j) kahan_add(a, ac, s_dh[o][j]);
                kahan_add(wacc[s], wcmp[s], a - ac);
            } else if (q < DB_PD * DB_IN + 2 * DB_PD) {
                const int o = q - DB_PD * DB_IN - DB_PD;
                float a = 0.0f, ac = 0.0f;
#pragma unroll 8
                for (int j = 0; j < DB_T; ++j) kahan_add(a, ac, s_dd[j] * s_lh[o][j]);
                kahan_add(wacc[s], wcmp[s], a - ac);
            } else if (q < DB_NW) {
                float a = 0.0f, ac = 0.0f;
#pragma unroll 8
                for (int j = 0; j < DB_T; ++j) kahan_add(a, ac, s_dd[j]);
                kahan_add(wacc[s], wcmp[s], a - ac);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int s = 0; s < DB_Q; ++s) {
        const int q = t + DB_T * s;
        if (q < DB_NW) part[(size_t)blockIdx.x * DB_NW + q] = wacc[s] - wcmp[s];
    }
}

// d emb of node r = renorm backward of the sum of its endpoint gradients, gathered in the order the caller's grouping lists them
// (slot 2 i: pair i's first endpoint, +gpair[i]; slot 2 i + 1: its second, -gpair[i]).  16 lanes per node, lane = column.
// torch's renorm_backward (maxnorm 1): rows with ||x|| > 1 get g / (n + 1e-7) - (x . g) x / (n (n + 1e-7)^2), the others g.
__global__ __launch_bounds__(256) void lp_node_grad_kernel(int n_nodes, const int* __restrict__ node_ptr, const int* __restrict__ slots,
                                                           const float* __restrict__ gpair, const float* __restrict__ x,
                                                           float* __restrict__ gx) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int r = (int)(gid >> 4), c = (int)(gid & 15);
    const bool live = r < n_nodes;
    float g = 0.0f, xc = 0.0f, s2 = 0.0f;
    if (live) {
        const int b = node_ptr[r], e = node_ptr[r + 1];
        int j = b;
        // (a hub node has thousands of endpoints: sixteen gathers in flight per trip, added in list order)
        for (; j + 16 <= e; j += 16) {
            int sl[16];
            float v[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) sl[q] = slots[j + q];
#pragma unroll
            for (int q = 0; q < 16; ++q) v[q] = gpair[(size_t)(sl[q] >> 1) * DB_ED + c];
#pragma unroll
            for (int q = 0; q < 16; ++q) g += (sl[q] & 1) ? -v[q] : v[q];
        }
        for (; j < e; ++j) {
            const int sl = slots[j];
            const float v = gpair[(size_t)(sl >> 1) * DB_ED + c];
            g += (sl & 1) ? -v : v;
        }
        const float* row = x + (size_t)r * DB_ED;
        xc = row[c];
        for (int k = 0; k < DB_ED; ++k) s2 += row[k] * row[k];
    }
    // x . g over the node's 16 lanes: butterfly (every lane ends with the same sum: a + b == b + a)
    float dot = xc * g;
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) dot += __shfl_xor(dot, m, 16);
    if (!live) return;
    const float n = sqrtf(s2);
    float out = g;
    if (n > 1.0f) {
        const float inv = 1.0f / (n + 1e-7f);
        out = inv * g - (inv * inv) * (xc * (dot / n));
    }
    gx[(size_t)r * DB_ED + c] = out;
}

}  // namespace

// ======================================================================================================================
// C ABI
// ======================================================================================================================
extern "C" int64_t tlc_gemm_tn_work_floats(int32_t M, int32_t N) {
    if (M < 0 || N < 0) return -1;
    return TlcGemmTnScratch(M, N).total;
}

extern "C" int tlc_gemm_tn_f32(int32_t M, int32_t N, int64_t K, const float* d_A, const float* d_B, float* d_C, float* d_work,
                               void* stream) {
    TLC_REQUIRE(M >= 1 && N >= 1 && K >= 0, "bad sizes");
    TLC_REQUIRE(d_A || M == 1 || K == 0, "d_A NULL (column sums) needs M = 1");
    TLC_REQUIRE(d_C && (K == 0 || d_B), "null pointer");
    TLC_REQUIRE((long long)M * N <= (1ll << 31) / TN_MAX_SPLITS, "M * N too large");
    hipStream_t s = (hipStream_t)stream;
    const int S = gemm_tn_splits(M, N, K);
    TLC_REQUIRE(S == 1 || d_work, "null scratch");
    const long long kps = S == 1 ? (K > 0 ? K : 1) : (K + S - 1) / S;
    const dim3 grid((M + TN_BM - 1) / TN_BM, (N + TN_BN - 1) / TN_BN, S);
    float* part = S == 1 ? nullptr : d_work + TlcGemmTnScratch(M, N).part;
    float* dst = S == 1 ? d_C : part;
    if (d_A) hipLaunchKernelGGL(gemm_tn_kernel<false>, grid, dim3(256), 0, s, M, N, (long long)K, kps, d_A, d_B, dst);
    else hipLaunchKernelGGL(gemm_tn_kernel<true>, grid, dim3(256), 0, s, M, N, (long long)K, kps, d_A, d_B, dst);
    if (S > 1) {
        const long long n_out = (long long)M * N;
        hipLaunchKernelGGL(sum_partials_kernel, dim3((unsigned)((n_out + 63) / 64)), dim3(64 * SP_R), 0, s, n_out, S,
                           (const float*)part, d_C);
    }
    TLC_HIP_CHECK(hipGetLastError());
    return TLC_OK;
}

extern "C" int64_t tlc_lp_decode_bwd_work_floats(int64_t n_pairs) {
    if (n_pairs < 0) return -1;
    return TlcLpDecodeBwdScratch(n_pairs).total;
}

extern "C" int tlc_lp_decode_bwd_f32(int64_t n_pairs, const int32_t* d_pairs, const float* d_emb_pre, const float* d_emb, int32_t n_nodes,
                                     int32_t emb_dim, const float* d_pi, int32_t pi_dim, const float* d_W1, const float* d_b1,
                                     const float* d_W2, const float* d_b2, const float* d_gprob, const int32_t* d_node_ptr,
                                     const int32_t* d_node_slots, float* d_gemb, float* d_gw, float* d_work, void* stream) {
    TLC_REQUIRE(n_pairs >= 0 && n_nodes >= 1, "bad sizes");
    if (emb_dim != DB_ED || pi_dim != DB_PD) {
        tlc_set_error("tlc_lp_decode_bwd_f32: emb_dim %d / pi_dim %d: only 16 / 25 (TLCGNN's conv2 width, dimension 5) is built", emb_dim, pi_dim);
        return TLC_ERR_UNSUPPORTED;
    }
    TLC_REQUIRE(n_pairs <= (1ll << 30), "more than 2^30 pairs (slots are int32)");
    TLC_REQUIRE(d_emb_pre && d_node_ptr && d_gemb && d_gw && d_work, "null pointer");
    TLC_REQUIRE(n_pairs == 0 || (d_pairs && d_emb && d_pi && d_W1 && d_b1 && d_W2 && d_b2 && d_gprob && d_node_slots), "null pointer");
    TLC_REQUIRE((reinterpret_cast<uintptr_t>(d_emb) & 15) == 0 && (reinterpret_cast<uintptr_t>(d_work) & 15) == 0, "emb / work not 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const TlcLpDecodeBwdScratch L(n_pairs);
    float *gpair = d_work + L.gpair, *part = d_work + L.part;
    if (n_pairs == 0) {
        TLC_HIP_CHECK(hipMemsetAsync(d_gw, 0, DB_NW * sizeof(float), s));
    } else {
        const long long tiles = (n_pairs + DB_T - 1) / DB_T;
        const int wg = (int)(tiles < DB_MAX_WG ? tiles : DB_MAX_WG);
        hipLaunchKernelGGL(lp_decode_bwd_kernel, dim3(wg), dim3(DB_T), 0, s, (long long)n_pairs, d_pairs, d_emb, d_pi, d_W1, d_b1, d_W2,
                           d_b2, d_gprob, gpair, part);
        hipLaunchKernelGGL(sum_partials_kernel, dim3((DB_NW + 63) / 64), dim3(64 * SP_R), 0, s, (long long)DB_NW, wg, (const float*)part, d_gw);
    }
    const long long th = (long long)n_nodes * DB_ED;
    hipLaunchKernelGGL(lp_node_grad_kernel, dim3((unsigned)((th + 255) / 256)), dim3(256), 0, s, n_nodes, d_node_ptr, d_node_slots,
                       (const float*)gpair, d_emb_pre, d_gemb);
    TLC_HIP_CHECK(hipGetLastError());
    return TLC_OK;
}

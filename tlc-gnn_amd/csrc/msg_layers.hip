// msg_layers.hip -- the PDGNN layer family: Knowledge_Distillation/gat_conv.py:113-216 with its ablation switches (new_node_feat :78-79,
// :193-195; use_edge_attn :197-200) and PD_conv.py's PDConv (:179-219), forward and backward, on a CSR by target with self loops added.
// include/tlcgnn.h states the contract; DESIGN.md 6.15 the reasons.
//
//   x_l = X Wl^T      alpha = x_l . att      P = x_l Wij[:, :C]^T      Q = x_l Wij[:, C:]^T   (without NODE_FEAT: Q = x_l)
//   per entry e = (j -> i):  h_e = leaky_relu(P_i + Q_j, 0.2) or Q_j;  a_e = softmax_i(leaky_relu(alpha_j + alpha_i, 0.2)) or 1;  m_e = a_e h_e
//   out_i = [ sum_e m_e || min_e m_e (+ max_e m_e) ] + bias, then the fused PReLU
//
// The node rows are f32 MFMA products (mfma_rows.h, the row-group code of gnn_layers.hip).  The aggregation and both backward passes give
// a target (or source) row to a group of C = c_out lanes, 64 / C rows per wavefront, lanes over channels: a row's sums are one chain per
// lane in entry order, its reductions over channels and its softmax statistics stay inside its own lane group.  The backward has NO
// floating-point atomic: what the forward gathers from the sources, the backward gathers a second time over the CSR by source, from the few
// per-row values the target pass left (maximum, denominator, softmax-backward dot, arg-min / arg-max entries).
// Built with -ffp-contract=off (the Makefile's default): every product is rounded before it is added.
#include <algorithm>

#include "mfma_rows.h"
#include "scratch_layouts.h"
#include "tlc_common.h"

#define ML_NODE_FEAT 1
#define ML_EDGE_ATTN 2
#define ML_AGG_SUM_MINMAX 0
#define ML_AGG_SUM_MIN 1
#define ML_SLOPE 0.2f             /* negative_slope of both leaky_relus (gat_conv.py:187,195; PD_conv.py:193) */

extern "C" int tlc_gemm_tn_f32(int32_t M, int32_t N, int64_t K, const float* d_A, const float* d_B, float* d_C, float* d_work, void* stream);

namespace {

__device__ __forceinline__ float ml_lrelu(float x) { return x > 0.0f ? x : ML_SLOPE * x; }
__device__ __forceinline__ float ml_dlrelu(float x) { return x > 0.0f ? 1.0f : ML_SLOPE; }
// over the C lanes of a row's group (C a power of two: lane ^ o stays inside the group); every lane ends with the same bits
template <int C>
__device__ __forceinline__ float ml_group_sum(float v) {
#pragma unroll
    for (int o = C / 2; o; o >>= 1) v = v + __shfl_xor(v, o);
    return v;
}
template <int C>
__device__ __forceinline__ float ml_group_max(float v) {
#pragma unroll
    for (int o = C / 2; o; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// ---- node rows on the MFMA -------------------------------------------------------------------------------------------------------------
// O1 = A1 W1 (+ A2 W2, when A2) (+ s (x) v, when s);  O2 = A1 W2 (when O2);  dot[i] = A1[i] . dv (when dot).   A1, A2 [n][kdim] row-major,
// W(k, c) = W[k * ldk + c * ldc] (kdim x cdim), the outputs [n][cdim].  Per output: the MFMA chain from a zero accumulator (all of A1 W1,
// then all of A2 W2), then + (s[i] * v[c]).  dot: per lane (l16, g) the chain over k = 16 q + 4 g + e (q, then e ascending) from +0, then
// + the lane 16 further, then + the lane 32 further.
struct MlProj {
    const float *A1, *A2, *W1, *W2, *s, *v, *dv;
    float *O1, *O2, *dot;
    int kdim, cdim, ldk, ldc;
};

template <int NT>
__global__ __launch_bounds__(GN_THREADS) void ml_proj_kernel(int n, MlProj p) {
    extern __shared__ __attribute__((aligned(16))) float ml_lds[];
    const int kq = (p.kdim + 15) >> 4;
    float* const w1 = ml_lds;
    float* const w2 = w1 + NT * kq * 256;
    if (p.W1) gn_stage(w1, NT, kq, p.W1, p.ldk, p.ldc, p.kdim, p.cdim);
    if (p.W2) gn_stage(w2, NT, kq, p.W2, p.ldk, p.ldc, p.kdim, p.cdim);
    __syncthreads();
    const bool vec = (p.kdim & 3) == 0;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l16 = lane & 15, g = lane >> 4;
    const long long n_groups = ((long long)n + GN_ROWS - 1) / GN_ROWS;
    for (long long grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
        const int r0 = (int)(grp * GN_ROWS);
        const int rows = n - r0 < GN_ROWS ? n - r0 : GN_ROWS;
        const int lrow = 16 * wave + l16;
        const bool live = lrow < rows;
        gn_f32x4 a1[GN_KQ], a2[GN_KQ];
#pragma unroll
        for (int q = 0; q < GN_KQ; ++q) {
            a1[q] = (gn_f32x4){0.f, 0.f, 0.f, 0.f};
            a2[q] = (gn_f32x4){0.f, 0.f, 0.f, 0.f};
            if (q < kq && live) {
                a1[q] = gn_load4(p.A1 + (size_t)(r0 + lrow) * p.kdim, 16 * q + 4 * g, p.kdim, vec);
                if (p.A2) a2[q] = gn_load4(p.A2 + (size_t)(r0 + lrow) * p.kdim, 16 * q + 4 * g, p.kdim, vec);
            }
        }
        if (p.dot) {
            float d = 0.0f;
#pragma unroll
            for (int q = 0; q < GN_KQ; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int k = 16 * q + 4 * g + e;
                    if (q < kq && k < p.kdim) d = d + a1[q][e] * p.dv[k];
                }
            d = d + __shfl_xor(d, 16);
            d = d + __shfl_xor(d, 32);
            if (live && g == 0) p.dot[r0 + lrow] = d;
        }
        if (!p.W1) continue;
        gn_f32x4 acc1[NT], acc2[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) { acc1[t] = (gn_f32x4){0.f, 0.f, 0.f, 0.f}; acc2[t] = (gn_f32x4){0.f, 0.f, 0.f, 0.f}; }
        gn_mma<NT>(a1, kq, w1, acc1);
        if (p.O2) gn_mma<NT>(a1, kq, w2, acc2);
        else if (p.A2) gn_mma<NT>(a2, kq, w2, acc1);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int c = 16 * t + l16;                                   // C/D layout: column = lane & 15, row = 4 (lane >> 4) + reg
            if (c < p.cdim) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int lr = 16 * wave + 4 * g + r;
                    if (lr < rows) {
                        const size_t at = (size_t)(r0 + lr) * p.cdim + c;
                        float v1 = acc1[t][r];
                        if (p.s) v1 = v1 + p.s[r0 + lr] * p.v[c];
                        p.O1[at] = v1;
                        if (p.O2) p.O2[at] = acc2[t][r];
                    }
                }
            }
        }
    }
}

// ---- the aggregation ---------------------------------------------------------------------------------------------------------------------
// What a lane needs of its row's softmax: the maximum of the logits and the denominator.  The group's lanes take the row's entries C apart,
// then meet in a butterfly; the denominator is + 1e-16 (PyG's softmax).  An entry whose source lies outside 0 .. n - 1 is left out.
template <int C>
__device__ __forceinline__ void ml_row_softmax(int n, int rb, int re, int ch, const int* __restrict__ src, const float* __restrict__ alpha, float ai,
                                               float& tmax, float& den) {
    float tm = -INFINITY;
    for (int e = rb + ch; e < re; e += C) {
        const int j = src[e];
        if ((unsigned)j < (unsigned)n) tm = fmaxf(tm, ml_lrelu(alpha[j] + ai));
    }
    tm = ml_group_max<C>(tm);
    float d = 0.0f;
    for (int e = rb + ch; e < re; e += C) {
        const int j = src[e];
        if ((unsigned)j < (unsigned)n) d = d + __expf(ml_lrelu(alpha[j] + ai) - tm);
    }
    tmax = tm;
    den = ml_group_sum<C>(d) + 1e-16f;
}

// the message of entry (j -> i) in this lane's channel, the same operations in the forward and in both backward passes
__device__ __forceinline__ float ml_message(bool nf, bool ea, float Pi, float qj, float t, float tmax, float den, float& a, float& z) {
    z = nf ? Pi + qj : qj;
    const float h = nf ? ml_lrelu(z) : qj;
    a = 1.0f;
    if (!ea) return h;
    a = __expf(ml_lrelu(t) - tmax) / den;
    return a * h;
}

template <int C>
__global__ __launch_bounds__(256) void ml_fwd_kernel(int n, const int* __restrict__ rowptr, const int* __restrict__ src, const float* __restrict__ P,
                                                     const float* __restrict__ Q, const float* __restrict__ alpha, const float* __restrict__ bias,
                                                     int mode, int agg, float slope, float* __restrict__ out) {
    constexpr int R = 64 / C;                                           // rows per wavefront
    const bool nf = mode & ML_NODE_FEAT, ea = mode & ML_EDGE_ATTN;
    const int lane = tlc_lane(), sub = lane / C, ch = lane % C;
    const long long n_waves = (long long)gridDim.x * 4;
    for (long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); w * R < n; w += n_waves) {
        const long long il = w * R + sub;
        if (il >= n) continue;
        const int i = (int)il;
        const int rb = rowptr[i], re = rowptr[i + 1];
        const float ai = ea ? alpha[i] : 0.0f, Pi = nf ? P[(size_t)i * C + ch] : 0.0f;
        float tmax = 0.0f, den = 1.0f;
        if (ea) ml_row_softmax<C>(n, rb, re, ch, src, alpha, ai, tmax, den);
        float acc = 0.0f, mn = INFINITY, mx = -INFINITY;
        bool bad = false;
        for (int e = rb; e < re; ++e) {
            const int j = src[e];
            if ((unsigned)j >= (unsigned)n) { bad = true; continue; }
            float a, z;
            const float m = ml_message(nf, ea, Pi, Q[(size_t)j * C + ch], ea ? alpha[j] + ai : 0.0f, tmax, den, a, z);
            acc = acc + m;
            if (m < mn) mn = m;
            if (m > mx) mx = m;
        }
        if (re <= rb) mn = mx = 0.0f;                                    // torch_scatter's value of an empty segment
        float o1 = acc + bias[ch], o2 = (agg == ML_AGG_SUM_MIN ? mn : mn + mx) + bias[C + ch];
        if (bad) o1 = o2 = __builtin_nanf("");
        if (slope >= 0.0f) { o1 = o1 > 0.0f ? o1 : slope * o1; o2 = o2 > 0.0f ? o2 : slope * o2; }
        out[(size_t)i * 2 * C + ch] = o1;
        out[(size_t)i * 2 * C + C + ch] = o2;
    }
}

// ---- backward, pass 1: a lane group per TARGET row -----------------------------------------------------------------------------------------
// Gz = gout * PReLU'(out) (`slope` at out <= 0, as torch).  The row again: softmax statistics, then per channel the FIRST entry that
// attains the minimum / the maximum (strict comparisons in entry order, the forward's own operations, so the same bits decide).  With
// gm_e = Gz_sum + Gz_mm * ([e is arg-min] + [e is arg-max]):  S = sum_e a_e * (sum_c gm_e h_e);  the logit gradient of entry e is
// gt_e = a_e (sum_c gm_e h_e - S) leaky'(t_e);  gtgt_i = sum_e gt_e;  gP_i = sum_e gm_e a_e leaky'(z_e) -- all chains in entry order.
template <int C>
__global__ __launch_bounds__(256) void ml_bwd_target_kernel(int n, const int* __restrict__ rowptr, const int* __restrict__ src,
                                                            const float* __restrict__ P, const float* __restrict__ Q, const float* __restrict__ alpha,
                                                            const float* __restrict__ out, const float* __restrict__ gout, int mode, int agg,
                                                            float slope, float* __restrict__ Gz, int* __restrict__ emn_o, int* __restrict__ emx_o,
                                                            float* __restrict__ stat, float* __restrict__ gtgt, float* __restrict__ gP) {
    constexpr int R = 64 / C;
    const bool nf = mode & ML_NODE_FEAT, ea = mode & ML_EDGE_ATTN;
    const int lane = tlc_lane(), sub = lane / C, ch = lane % C;
    const long long n_waves = (long long)gridDim.x * 4;
    for (long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); w * R < n; w += n_waves) {
        const long long il = w * R + sub;
        if (il >= n) continue;
        const int i = (int)il;
        const int rb = rowptr[i], re = rowptr[i + 1];
        const size_t o1 = (size_t)i * 2 * C + ch, o2 = o1 + C;
        float gs = gout[o1], gmm = gout[o2];
        if (slope >= 0.0f) {
            if (out[o1] <= 0.0f) gs = slope * gs;
            if (out[o2] <= 0.0f) gmm = slope * gmm;
        }
        Gz[o1] = gs; Gz[o2] = gmm;
        const float ai = ea ? alpha[i] : 0.0f, Pi = nf ? P[(size_t)i * C + ch] : 0.0f;
        float tmax = 0.0f, den = 1.0f;
        if (ea) ml_row_softmax<C>(n, rb, re, ch, src, alpha, ai, tmax, den);
        float mn = INFINITY, mx = -INFINITY;
        int emn = -1, emx = -1;
        for (int e = rb; e < re; ++e) {
            const int j = src[e];
            if ((unsigned)j >= (unsigned)n) continue;
            float a, z;
            const float m = ml_message(nf, ea, Pi, Q[(size_t)j * C + ch], ea ? alpha[j] + ai : 0.0f, tmax, den, a, z);
            if (m < mn) { mn = m; emn = e; }
            if (m > mx) { mx = m; emx = e; }
        }
        if (agg == ML_AGG_SUM_MIN) emx = -1;
        emn_o[(size_t)i * C + ch] = emn;
        emx_o[(size_t)i * C + ch] = emx;
        if (!nf && !ea) continue;                                        // m_e = x_l[j]: nothing flows to the target's own row
        float S = 0.0f;
        if (ea) {
            for (int e = rb; e < re; ++e) {
                const int j = src[e];
                if ((unsigned)j >= (unsigned)n) continue;
                float a, z;
                const float m = ml_message(nf, ea, Pi, Q[(size_t)j * C + ch], alpha[j] + ai, tmax, den, a, z);
                const float gm = gs + gmm * ((e == emn ? 1.0f : 0.0f) + (e == emx ? 1.0f : 0.0f));
                S = S + ml_group_sum<C>(gm * m);                         // a_e * (gm . h_e) = gm . m_e
            }
        }
        float gPi = 0.0f, gai = 0.0f;
        for (int e = rb; e < re; ++e) {
            const int j = src[e];
            if ((unsigned)j >= (unsigned)n) continue;
            const float t = ea ? alpha[j] + ai : 0.0f;
            float a, z;
            const float m = ml_message(nf, ea, Pi, Q[(size_t)j * C + ch], t, tmax, den, a, z);
            const float gm = gs + gmm * ((e == emn ? 1.0f : 0.0f) + (e == emx ? 1.0f : 0.0f));
            if (ea) gai = gai + (ml_group_sum<C>(gm * m) - a * S) * ml_dlrelu(t);
            if (nf) gPi = gPi + gm * a * ml_dlrelu(z);
        }
        if (nf) gP[(size_t)i * C + ch] = gPi;
        if (ea && ch == 0) {
            gtgt[i] = gai;
            stat[(size_t)4 * i] = tmax; stat[(size_t)4 * i + 1] = den; stat[(size_t)4 * i + 2] = S;
        }
    }
}

// ---- backward, pass 2: a lane group per SOURCE row ------------------------------------------------------------------------------------------
// Row j of the CSR by source lists the entries (j -> i) as (col_t = i, pos_t = the entry's position in the CSR by target), ascending.  Every
// entry's message and gradient are recomputed from the target's row scalars and arg entries; gQ_j = sum gm_e a_e leaky'(z_e) and
// galpha_j = (sum gt_e) + gtgt_j, chains in entry order.  Without NODE_FEAT the message part of gx_l is gQ itself, so the pass writes
// gx_l[j] = gQ_j + (galpha_j * att) at once.  A target outside 0 .. n - 1 is left out.
template <int C>
__global__ __launch_bounds__(256) void ml_bwd_source_kernel(int n, const int* __restrict__ rowptr_t, const int* __restrict__ col_t,
                                                            const int* __restrict__ pos_t, const float* __restrict__ P, const float* __restrict__ Q,
                                                            const float* __restrict__ alpha, const float* __restrict__ att, int mode,
                                                            const float* __restrict__ Gz, const int* __restrict__ emn, const int* __restrict__ emx,
                                                            const float* __restrict__ stat, const float* __restrict__ gtgt, float* __restrict__ gQ,
                                                            float* __restrict__ galpha) {
    constexpr int R = 64 / C;
    const bool nf = mode & ML_NODE_FEAT, ea = mode & ML_EDGE_ATTN;
    const int lane = tlc_lane(), sub = lane / C, ch = lane % C;
    const long long n_waves = (long long)gridDim.x * 4;
    for (long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); w * R < n; w += n_waves) {
        const long long jl = w * R + sub;
        if (jl >= n) continue;
        const int j = (int)jl;
        const int rb = rowptr_t[j], re = rowptr_t[j + 1];
        const float aj = ea ? alpha[j] : 0.0f, qj = Q[(size_t)j * C + ch];
        float gQj = 0.0f, gaj = 0.0f;
        for (int e = rb; e < re; ++e) {
            const int i = col_t[e], pos = pos_t[e];
            if ((unsigned)i >= (unsigned)n) continue;
            const size_t ic = (size_t)i * C + ch;
            const float gm = Gz[(size_t)i * 2 * C + ch] + Gz[(size_t)i * 2 * C + C + ch] * ((pos == emn[ic] ? 1.0f : 0.0f) + (pos == emx[ic] ? 1.0f : 0.0f));
            const float t = ea ? aj + alpha[i] : 0.0f;
            float tmax = 0.0f, den = 1.0f, S = 0.0f;
            if (ea) { tmax = stat[(size_t)4 * i]; den = stat[(size_t)4 * i + 1]; S = stat[(size_t)4 * i + 2]; }
            float a, z;
            const float m = ml_message(nf, ea, nf ? P[ic] : 0.0f, qj, t, tmax, den, a, z);
            if (ea) gaj = gaj + (ml_group_sum<C>(gm * m) - a * S) * ml_dlrelu(t);
            gQj = gQj + gm * a * (nf ? ml_dlrelu(z) : 1.0f);
        }
        if (ea) {
            gaj = gaj + gtgt[j];
            if (ch == 0) galpha[j] = gaj;
            if (!nf) gQj = gQj + gaj * att[ch];
        }
        gQ[(size_t)j * C + ch] = gQj;
    }
}

// gWij [C][2C] from its halves T[0] = gP^T x_l and T[1] = gQ^T x_l, [C][C] each
__global__ void ml_join_halves_kernel(int C, const float* __restrict__ T, float* __restrict__ gWij) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 2 * C * C) return;
    const int c = t / (2 * C), k = t % (2 * C);
    gWij[t] = k < C ? T[c * C + k] : T[C * C + c * C + (k - C)];
}

int ml_project(int n, int nt, const MlProj& p, int cus, hipStream_t s) {
    const int kq = (p.kdim + 15) / 16;
    const size_t lds = (size_t)2 * nt * kq * 256 * sizeof(float);                                              // at most 32 KiB
    const long long groups = ((long long)n + GN_ROWS - 1) / GN_ROWS;
    const unsigned grid = (unsigned)std::min<long long>(groups, (long long)cus * 4);
    GN_BY_TILES(nt, hipLaunchKernelGGL(ml_proj_kernel<NT>, dim3(grid), dim3(GN_THREADS), lds, s, n, p));
    TLC_HIP_CHECK(hipGetLastError());
    return TLC_OK;
}

unsigned ml_row_grid(int n, int C, int cus) {
    const long long waves = ((long long)n + 64 / C - 1) / (64 / C);
    return (unsigned)std::max<long long>(1, std::min<long long>((waves + 3) / 4, (long long)cus * 32));
}

#define ML_BY_WIDTH(C_, CALL)                           \
    do {                                                \
        if ((C_) == 8) { constexpr int C = 8; CALL; }   \
        else if ((C_) == 16) { constexpr int C = 16; CALL; } \
        else if ((C_) == 32) { constexpr int C = 32; CALL; } \
        else { constexpr int C = 64; CALL; }            \
    } while (0)

// x_l, then [P | Q] and alpha, into the rows of `f` inside work
int ml_node_rows(int n, const float* X, int c_in, int C, const float* Wl, const float* att, const float* Wij, bool nf, bool ea, float* work,
                 const TlcMsgLayerFwdScratch& f, int cus, hipStream_t s) {
    MlProj p = {};
    p.A1 = X; p.kdim = c_in; p.cdim = C; p.W1 = Wl; p.ldk = 1; p.ldc = c_in; p.O1 = work + f.xl;          // W(k, c) = Wl[c][k]
    if (int rc = ml_project(n, gn_tiles_of(C), p, cus, s)) return rc;
    if (!nf && !ea) return TLC_OK;
    MlProj r = {};
    r.A1 = work + f.xl; r.kdim = C; r.cdim = C;
    if (nf) { r.W1 = Wij; r.W2 = Wij + C; r.ldk = 1; r.ldc = 2 * C; r.O1 = work + f.p; r.O2 = work + f.q; }   // W(k, c) = Wij[c][k], Wij[c][C + k]
    if (ea) { r.dot = work + f.alpha; r.dv = att; }
    return ml_project(n, gn_tiles_of(C), r, cus, s);
}

bool ml_flags_ok(int mode, int agg) { return (mode & ~(ML_NODE_FEAT | ML_EDGE_ATTN)) == 0 && (agg == ML_AGG_SUM_MINMAX || agg == ML_AGG_SUM_MIN); }

}  // namespace

extern "C" int64_t tlc_msg_layer_fwd_work_bytes(int32_t n_nodes, int32_t c_in, int32_t c_out, int32_t mode) {
    if (n_nodes < 0 || c_in < 0 || c_out < 0 || !ml_flags_ok(mode, 0)) return -1;
    return TlcMsgLayerFwdScratch(n_nodes, c_out, mode & ML_NODE_FEAT, mode & ML_EDGE_ATTN).total * (int64_t)sizeof(float);
}

extern "C" int tlc_msg_layer_fwd(int32_t n_nodes, const int32_t* d_rowptr, const int32_t* d_src, const float* d_X, int32_t c_in, int32_t c_out,
                                 const float* d_Wl, const float* d_att, const float* d_Wij, const float* d_bias, int32_t mode, int32_t agg,
                                 float prelu_slope, void* d_work, int64_t work_bytes, float* d_out, void* stream) {
    TLC_REQUIRE(n_nodes >= 0, "n_nodes < 0");
    TLC_REQUIRE(ml_flags_ok(mode, agg), "unknown mode / agg bits");
    if (!gn_width_ok(c_in, c_out)) {
        tlc_set_error("tlc_msg_layer_fwd: c_in %d / c_out %d: built for c_in in 1 .. 64 and c_out in {8, 16, 32, 64}", c_in, c_out);
        return TLC_ERR_UNSUPPORTED;
    }
    const bool nf = mode & ML_NODE_FEAT, ea = mode & ML_EDGE_ATTN;
    TLC_REQUIRE(d_Wl && d_bias && (!ea || d_att) && (!nf || d_Wij), "null pointer");
    if (n_nodes == 0) return TLC_OK;
    TLC_REQUIRE(d_rowptr && d_src && d_X && d_out && d_work, "null pointer");
    const TlcMsgLayerFwdScratch f(n_nodes, c_out, nf, ea);
    TLC_REQUIRE(work_bytes >= f.total * (int64_t)sizeof(float) && ((uintptr_t)d_work & 15) == 0,
                "d_work below tlc_msg_layer_fwd_work_bytes() or not 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    float* const work = (float*)d_work;
    int cus = 0;
    if (int rc = gn_cus(&cus)) return rc;
    if (int rc = ml_node_rows(n_nodes, d_X, c_in, c_out, d_Wl, d_att, d_Wij, nf, ea, work, f, cus, s)) return rc;
    const float* const Q = nf ? work + f.q : work + f.xl;
    ML_BY_WIDTH(c_out, hipLaunchKernelGGL(ml_fwd_kernel<C>, dim3(ml_row_grid(n_nodes, C, cus)), dim3(256), 0, s, n_nodes, d_rowptr, d_src,
                                          (const float*)(work + f.p), Q, (const float*)(work + f.alpha), d_bias, mode, agg, prelu_slope, d_out));
    TLC_HIP_CHECK(hipGetLastError());
    return TLC_OK;
}

extern "C" int64_t tlc_msg_layer_bwd_work_bytes(int32_t n_nodes, int64_t n_entries, int32_t c_in, int32_t c_out, int32_t mode) {
    if (n_nodes < 0 || n_entries < 0 || c_in < 0 || c_out < 0 || !ml_flags_ok(mode, 0)) return -1;
    return TlcMsgLayerBwdScratch(n_nodes, c_in, c_out, mode & ML_NODE_FEAT, mode & ML_EDGE_ATTN).total * (int64_t)sizeof(float);
}

extern "C" int tlc_msg_layer_bwd(int32_t n_nodes, const int32_t* d_rowptr, const int32_t* d_src, const int32_t* d_rowptr_t, const int32_t* d_col_t,
                                 const int32_t* d_pos_t, const float* d_X, int32_t c_in, int32_t c_out, const float* d_Wl, const float* d_att,
                                 const float* d_Wij, int32_t mode, int32_t agg, float prelu_slope, const float* d_out, const float* d_gout,
                                 float* d_gX, float* d_gWl, float* d_gatt, float* d_gWij, float* d_gbias, void* d_work, int64_t work_bytes,
                                 void* stream) {
    TLC_REQUIRE(n_nodes >= 0, "n_nodes < 0");
    TLC_REQUIRE(ml_flags_ok(mode, agg), "unknown mode / agg bits");
    if (!gn_width_ok(c_in, c_out)) {
        tlc_set_error("tlc_msg_layer_bwd: c_in %d / c_out %d: built for c_in in 1 .. 64 and c_out in {8, 16, 32, 64}", c_in, c_out);
        return TLC_ERR_UNSUPPORTED;
    }
    const bool nf = mode & ML_NODE_FEAT, ea = mode & ML_EDGE_ATTN;
    const int C = c_out;
    TLC_REQUIRE(d_Wl && (!ea || d_att) && (!nf || d_Wij) && d_gWl && d_gbias && (!ea || d_gatt) && (!nf || d_gWij), "null pointer");
    TLC_REQUIRE(n_nodes == 0 || (d_rowptr && d_src && d_rowptr_t && d_col_t && d_pos_t && d_X && d_gout && d_work && (prelu_slope < 0.0f || d_out)),
                "null pointer");
    const TlcMsgLayerBwdScratch L(n_nodes, c_in, C, nf, ea);
    TLC_REQUIRE(n_nodes == 0 || (work_bytes >= L.total * (int64_t)sizeof(float) && ((uintptr_t)d_work & 15) == 0),
                "d_work below tlc_msg_layer_bwd_work_bytes() or not 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (n_nodes == 0) {
        TLC_HIP_CHECK(hipMemsetAsync(d_gWl, 0, (size_t)C * c_in * sizeof(float), s));
        TLC_HIP_CHECK(hipMemsetAsync(d_gbias, 0, (size_t)2 * C * sizeof(float), s));
        if (ea) TLC_HIP_CHECK(hipMemsetAsync(d_gatt, 0, (size_t)C * sizeof(float), s));
        if (nf) TLC_HIP_CHECK(hipMemsetAsync(d_gWij, 0, (size_t)2 * C * C * sizeof(float), s));
        return TLC_OK;
    }
    float* const work = (float*)d_work;
    int cus = 0;
    if (int rc = gn_cus(&cus)) return rc;
    // the forward's node rows again
    if (int rc = ml_node_rows(n_nodes, d_X, c_in, C, d_Wl, d_att, d_Wij, nf, ea, work, L.f, cus, s)) return rc;
    const float *xl = work + L.f.xl, *P = work + L.f.p, *Q = nf ? work + L.f.q : xl, *alpha = work + L.f.alpha;
    float *Gz = work + L.gz, *gxl = work + L.gxl, *stat = work + L.stat, *gtgt = work + L.gtgt, *gal = work + L.gal, *gP = work + L.gp,
          *gQ = nf ? work + L.gq : gxl, *tn = work + L.tn;
    int *emn = (int*)(work + L.emn), *emx = (int*)(work + L.emx);
    ML_BY_WIDTH(C, hipLaunchKernelGGL(ml_bwd_target_kernel<C>, dim3(ml_row_grid(n_nodes, C, cus)), dim3(256), 0, s, n_nodes, d_rowptr, d_src, P, Q,
                                      alpha, d_out, d_gout, mode, agg, prelu_slope, Gz, emn, emx, stat, gtgt, gP));
    TLC_HIP_CHECK(hipGetLastError());
    // (the weight gradients need the sums at the sources as well, so this pass runs for a first layer too; only gX = gx_l Wl is left out)
    ML_BY_WIDTH(C, hipLaunchKernelGGL(ml_bwd_source_kernel<C>, dim3(ml_row_grid(n_nodes, C, cus)), dim3(256), 0, s, n_nodes, d_rowptr_t, d_col_t,
                                      d_pos_t, P, Q, alpha, d_att, mode, (const float*)Gz, (const int*)emn, (const int*)emx, (const float*)stat,
                                      (const float*)gtgt, gQ, gal));
    TLC_HIP_CHECK(hipGetLastError());
    if (nf) {
        // gx_l = gP Wij[:, :C] + gQ Wij[:, C:] + galpha (x) att
        MlProj p = {};
        p.A1 = gP; p.A2 = gQ; p.kdim = C; p.cdim = C; p.W1 = d_Wij; p.W2 = d_Wij + C; p.ldk = 2 * C; p.ldc = 1; p.O1 = gxl;   // W(k, c) = Wij[k][c], Wij[k][C + c]
        if (ea) { p.s = gal; p.v = d_att; }
        if (int rc = ml_project(n_nodes, gn_tiles_of(C), p, cus, s)) return rc;
    }
    if (d_gX) {
        MlProj p = {};
        p.A1 = gxl; p.kdim = C; p.cdim = c_in; p.W1 = d_Wl; p.ldk = c_in; p.ldc = 1; p.O1 = d_gX;          // W(k, c) = Wl[k][c]
        if (int rc = ml_project(n_nodes, gn_tiles_of(c_in), p, cus, s)) return rc;
    }
    // the weight gradients: tlc_gemm_tn_f32's split-K, a partition that n_nodes and the widths alone fix, partials added in split order
    if (int rc = tlc_gemm_tn_f32(C, c_in, n_nodes, gxl, d_X, d_gWl, tn, stream)) return rc;                  // gWl = gx_l^T X
    if (int rc = tlc_gemm_tn_f32(1, 2 * C, n_nodes, nullptr, Gz, d_gbias, tn, stream)) return rc;            // gbias = column sums of Gz
    if (ea)
        if (int rc = tlc_gemm_tn_f32(1, C, n_nodes, gal, xl, d_gatt, tn, stream)) return rc;                 // gatt = galpha^T x_l
    if (nf) {
        float* const T = work + L.halves;
        if (int rc = tlc_gemm_tn_f32(C, C, n_nodes, gP, xl, T, tn, stream)) return rc;                       // gWij[:, :C] = gP^T x_l
        if (int rc = tlc_gemm_tn_f32(C, C, n_nodes, gQ, xl, T + C * C, tn, stream)) return rc;               // gWij[:, C:] = gQ^T x_l
        hipLaunchKernelGGL(ml_join_halves_kernel, dim3((2 * C * C + 255) / 256), dim3(256), 0, s, C, (const float*)T, d_gWij);
        TLC_HIP_CHECK(hipGetLastError());
    }
    return TLC_OK;
}

// gnn_layers.hip -- the sum-aggregating baselines of the PDGNN teacher (Knowledge_Distillation/Teacher_model.py:148-175,202-208:
// GINConv, GCNConv, SAGEConv) as ONE layer form on a CSR by target, forward and backward, and the four-layer inference stack of
// Base_Model.forward (:213-241) in one launch.  include/tlcgnn.h states the contract; DESIGN.md 6.14 the reasons.
//
//   agg_i = sum over the in-edges e of i, in CSR order, of coef[e] * x_src[e]   (+ self_scale * x_i, last)
//   z_i   = Wa agg_i + Ws x_i + b          y_i = act(z_i)
//
// A wavefront owns a block of 16 node rows.  Lane (l16, g) of it walks the in-edges of row l16 and sums, for q = 0 .. kq - 1, the four
// columns k = 16 q + 4 g .. + 3: exactly the values it feeds the f32 MFMA as the A operand (a sum over k does not care in which order the
// lanes hold k, as long as B is staged the same way), so the aggregate never leaves registers on its way into the projection.  The
// weights sit in LDS in MFMA operand layout for the workgroup's whole life.  No atomics: a row's sum is one chain in one lane, an MFMA
// output row depends on its own row of A alone, and the weight gradients are tlc_gemm_tn_f32's fixed split-K.
// Built with -ffp-contract=off (the Makefile's default): coef * x is rounded before it is added.
#include <algorithm>
#include <mutex>

#include "mfma_rows.h"
#include "scratch_layouts.h"
#include "tlc_common.h"

#define GN_TILE 192               /* most nodes of a tile of the stack kernel (tlc_gat_tile_cut's GT_TM) */
#define GN_HID 32                 /* the stack kernel's width */
#define GN_ACT_NONE 0
#define GN_ACT_RELU 1
#define GN_ACT_PRELU 2

// ---- shared device code -------------------------------------------------------------------------------------------------------------
// (gn_stage, gn_load4, gn_mma: mfma_rows.h)
// This lane's A operands of row `row` (ids relative to the first row that `xrow` serves, n_src rows): a_agg = the row's aggregate, a_x =
// the row itself.  The chain: acc = +0; for every in-edge e ascending: acc = acc + coef[e] * x_src[e] (the product rounded first; coef
// NULL: 1); then, with self_scale != 0, acc = acc + self_scale * x_row.  A source outside the served rows contributes NaN, reads nothing.
template <class Row>
__device__ __forceinline__ void gn_gather(bool live, int row, int eb, int ee, const int* __restrict__ src, int src_base, int n_src,
                                          const float* __restrict__ coef, float self_scale, int width, int kq, bool vec, Row xrow,
                                          gn_f32x4 (&a_agg)[GN_KQ], gn_f32x4 (&a_x)[GN_KQ]) {
    const int g = (threadIdx.x & 63) >> 4;
#pragma unroll
    for (int q = 0; q < GN_KQ; ++q) { a_agg[q] = (gn_f32x4){0.f, 0.f, 0.f, 0.f}; a_x[q] = (gn_f32x4){0.f, 0.f, 0.f, 0.f}; }
    if (!live) return;
    for (int e = eb; e < ee; ++e) {
        const int j = src[e] - src_base;
        const bool ok = (unsigned)j < (unsigned)n_src;
        const float c = coef ? coef[e] : 1.0f;
        const float* xr = xrow(ok ? j : 0);
#pragma unroll
        for (int q = 0; q < GN_KQ; ++q) {
            if (q < kq) {
                gn_f32x4 v = gn_load4(xr, 16 * q + 4 * g, width, vec);
                if (!ok) v = (gn_f32x4){__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""), __builtin_nanf("")};
                a_agg[q] = a_agg[q] + c * v;
            }
        }
    }
    const float* xi = xrow(row);
#pragma unroll
    for (int q = 0; q < GN_KQ; ++q) {
        if (q < kq) {
            a_x[q] = gn_load4(xi, 16 * q + 4 * g, width, vec);
            if (self_scale != 0.0f) a_agg[q] = a_agg[q] + self_scale * a_x[q];
        }
    }
}

__device__ __forceinline__ float gn_act(float z, int act, float slope) {
    if (act == GN_ACT_RELU) return z > 0.0f ? z : 0.0f;
    if (act == GN_ACT_PRELU) return z > 0.0f ? z : slope * z;
    return z;
}

// One 16-row block of the layer: gather, project (the Wa steps, then the Ws steps), + bias, activation, into dst (row stride ds, rows
// relative to the block's group or tile).  C/D layout of the MFMA: column = lane & 15, row = 4 (lane >> 4) + reg.
template <int NT, class Row>
__device__ __forceinline__ void gn_block(int lrow0, int rows, int row0, const int* __restrict__ rowptr, const int* __restrict__ src,
                                         int src_base, int n_src, const float* __restrict__ coef, float self_scale, int width, int kq, bool vec,
                                         Row xrow, const float* wa, const float* ws, const float* bias, int c_out, int act, float slope,
                                         float* dst, int ds, gn_f32x4 (&a_agg)[GN_KQ]) {
    const int lane = threadIdx.x & 63, l16 = lane & 15, g = lane >> 4;
    const int lrow = lrow0 + l16;                   // relative to the group / tile; row0 + lrow: the row of the CSR
    const bool live = lrow < rows;
    int eb = 0, ee = 0;
    if (live) { eb = rowptr[row0 + lrow]; ee = rowptr[row0 + lrow + 1]; }
    gn_f32x4 a_x[GN_KQ];
    gn_gather(live, row0 + lrow - src_base, eb, ee, src, src_base, n_src, coef, self_scale, width, kq, vec, xrow, a_agg, a_x);
    gn_f32x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = (gn_f32x4){0.f, 0.f, 0.f, 0.f};
    gn_mma<NT>(a_agg, kq, wa, acc);
    if (ws) gn_mma<NT>(a_x, kq, ws, acc);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int c = 16 * t + l16;
        if (c < c_out) {
            const float b = bias ? bias[c] : 0.0f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int lr = lrow0 + 4 * g + r;
                if (lr < rows) dst[lr * ds + c] = gn_act(acc[t][r] + b, act, slope);
            }
        }
    }
}

// ---- the layer, forward ---------------------------------------------------------------------------------------------------------------
// Persistent workgroups over groups of GN_ROWS rows.  LDS: Wa staged | Ws staged | the group's output rows [GN_ROWS][c_out].
template <int NT>
__global__ __launch_bounds__(GN_THREADS) void gnn_layer_kernel(int n, const int* __restrict__ rowptr, const int* __restrict__ src,
                                                               const float* __restrict__ coef, float self_scale, const float* __restrict__ X,
                                                               int c_in, int c_out, const float* __restrict__ Wa, const float* __restrict__ Ws,
                                                               const float* __restrict__ bias, int act, float slope, float* __restrict__ out,
                                                               float* __restrict__ aggout) {
    extern __shared__ __attribute__((aligned(16))) float gn_lds[];
    const int kq = (c_in + 15) >> 4;
    float* const wa = gn_lds;
    float* const ws = Ws ? wa + NT * kq * 256 : nullptr;
    float* const ot = wa + (Ws ? 2 : 1) * NT * kq * 256;
    gn_stage(wa, NT, kq, Wa, 1, c_in, c_in, c_out);                   // W(k, c) = Wa[c][k]
    if (Ws) gn_stage(ws, NT, kq, Ws, 1, c_in, c_in, c_out);
    __syncthreads();
    const bool vec = (c_in & 3) == 0;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l16 = lane & 15, g = lane >> 4;
    const long long n_groups = ((long long)n + GN_ROWS - 1) / GN_ROWS;
    auto xrow = [&](int j) -> const float* { return X + (size_t)j * c_in; };
    for (long long grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
        const int r0 = (int)(grp * GN_ROWS);
        const int rows = n - r0 < GN_ROWS ? n - r0 : GN_ROWS;
        gn_f32x4 a_agg[GN_KQ];
        gn_block<NT>(16 * wave, rows, r0, rowptr, src, 0, n, coef, self_scale, c_in, kq, vec, xrow, wa, ws, bias, c_out, act, slope, ot, c_out,
                     a_agg);
        if (aggout && 16 * wave + l16 < rows) {
            float* const ar = aggout + (size_t)(r0 + 16 * wave + l16) * c_in;
#pragma unroll
            for (int q = 0; q < GN_KQ; ++q) {
                const int k0 = 16 * q + 4 * g;
                if (q < kq) {
                    if (vec) { if (k0 < c_in) *reinterpret_cast<gn_f32x4*>(ar + k0) = a_agg[q]; }
                    else {
#pragma unroll
                        for (int e = 0; e < 4; ++e) if (k0 + e < c_in) ar[k0 + e] = a_agg[q][e];
                    }
                }
            }
        }
        __syncthreads();
        float* const og = out + (size_t)r0 * c_out;                     // the group's rows are one contiguous piece of `out`
        for (int i = threadIdx.x; i < rows * c_out; i += GN_THREADS) og[i] = ot[i];
        __syncthreads();
    }
}

// ---- the layer, backward --------------------------------------------------------------------------------------------------------------
// dZ = gout * act'(out) (the derivative read off the sign of `out`: ReLU 1 / 0, PReLU 1 / slope, 0 and `slope` at out == 0 like torch),
// written for the weight-gradient products; G = dZ Wa and H = dZ Ws on the MFMA when the input's gradient is wanted.
template <int NT>
__global__ __launch_bounds__(GN_THREADS) void gnn_bwd_rows_kernel(int n, const float* __restrict__ out, const float* __restrict__ gout, int c_in,
                                                                  int c_out, const float* __restrict__ Wa, const float* __restrict__ Ws, int act,
                                                                  float slope, float* __restrict__ dZ, float* __restrict__ G, float* __restrict__ H) {
    extern __shared__ __attribute__((aligned(16))) float gn_lds[];
    const int kq = (c_out + 15) >> 4;
    float* const wa = gn_lds;
    float* const ws = wa + NT * kq * 256;
    if (G) gn_stage(wa, NT, kq, Wa, c_in, 1, c_out, c_in);             // W(k, c) = Wa[k][c]
    if (H) gn_stage(ws, NT, kq, Ws, c_in, 1, c_out, c_in);
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l16 = lane & 15, g = lane >> 4;
    const long long n_groups = ((long long)n + GN_ROWS - 1) / GN_ROWS;
    for (long long grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
        const int r0 = (int)(grp * GN_ROWS);
        const int rows = n - r0 < GN_ROWS ? n - r0 : GN_ROWS;
        const int lrow = 16 * wave + l16;
        gn_f32x4 a[GN_KQ];
#pragma unroll
        for (int q = 0; q < GN_KQ; ++q) {
            a[q] = (gn_f32x4){0.f, 0.f, 0.f, 0.f};
            const int k0 = 16 * q + 4 * g;
            if (q < kq && lrow < rows && k0 < c_out) {                  // (c_out is a multiple of 4)
                const size_t at = (size_t)(r0 + lrow) * c_out + k0;
                gn_f32x4 d = *reinterpret_cast<const gn_f32x4*>(gout + at);
                if (act != GN_ACT_NONE) {
                    const gn_f32x4 o = *reinterpret_cast<const gn_f32x4*>(out + at);
                    const float neg = act == GN_ACT_PRELU ? slope : 0.0f;
#pragma unroll
                    for (int e = 0; e < 4; ++e) d[e] = o[e] > 0.0f ? d[e] : neg * d[e];
                }
                *reinterpret_cast<gn_f32x4*>(dZ + at) = d;
                a[q] = d;
            }
        }
        if (!G) continue;
        gn_f32x4 accg[NT], acch[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) { accg[t] = (gn_f32x4){0.f, 0.f, 0.f, 0.f}; acch[t] = (gn_f32x4){0.f, 0.f, 0.f, 0.f}; }
        gn_mma<NT>(a, kq, wa, accg);
        if (H) gn_mma<NT>(a, kq, ws, acch);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int c = 16 * t + l16;
            if (c < c_in) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int lr = 16 * wave + 4 * g + r;
                    if (lr < rows) {
                        G[(size_t)(r0 + lr) * c_in + c] = accg[t][r];
                        if (H) H[(size_t)(r0 + lr) * c_in + c] = acch[t][r];
                    }
                }
            }
        }
    }
}

// gX[i][c]: acc = +0; for every entry e of row i of the CSR by source, ascending: acc = acc + coef_t[e] * G[col_t[e]][c]; then, with
// self_scale != 0, acc = acc + self_scale * G[i][c]; then, with Ws, acc = acc + H[i][c].  A thread per element.
__global__ __launch_bounds__(256) void gnn_bwd_gather_kernel(long long total, int n, int c_in, const int* __restrict__ rowptr_t,
                                                             const int* __restrict__ col_t, const float* __restrict__ coef_t, float self_scale,
                                                             const float* __restrict__ G, const float* __restrict__ H, float* __restrict__ gX) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int row = (int)(i / c_in), c = (int)(i - (long long)row * c_in);
        float acc = 0.0f;
        const int eb = rowptr_t[row], ee = rowptr_t[row + 1];
        for (int e = eb; e < ee; ++e) {
            const int j = col_t[e];
            const float v = (unsigned)j < (unsigned)n ? G[(size_t)j * c_in + c] : __builtin_nanf("");
            acc = acc + (coef_t ? coef_t[e] : 1.0f) * v;
        }
        if (self_scale != 0.0f) acc = acc + self_scale * G[i];
        if (H) acc = acc + H[i];
        gX[i] = acc;
    }
}

// ---- the four-layer stack, one launch ---------------------------------------------------------------------------------------------------
// conv1 (1 -> 32) -> conv2 -> conv4 -> conv3 (32 -> 32 each) on a batch cut into self-contained tiles (tlc_gat_tile_cut).  LDS: two
// buffers of the tile's node rows [GN_TILE][GN_HID] | the four biases [4][GN_HID] | the four layers' weights staged for the MFMA
// (Wa: 512 + 3 x 1024 floats, as many again with Ws): 64 000 B without Ws, 78 336 B with it -- two workgroups per CU either way.
struct GnStackArgs {
    const float* wa[4];
    const float* ws[4];
    const float* b[4];
    int act[4];
    float slope[4];
};
#define GN_STACK_W1 (2 * 1 * 256)      /* staged floats of a 1 -> 32 matrix: NT 2, kq 1 */
#define GN_STACK_WH (2 * 2 * 256)      /* of a 32 -> 32 matrix: NT 2, kq 2 */
#define GN_STACK_WALL (GN_STACK_W1 + 3 * GN_STACK_WH)

__global__ __launch_bounds__(GN_THREADS) void gnn_stack_kernel(int n, int n_tiles, const int* __restrict__ tile_ptr, const int* __restrict__ rowptr,
                                                                  const int* __restrict__ src, const float* __restrict__ coef, float self_scale,
                                                                  const float* __restrict__ x, GnStackArgs a, bool has_ws, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float gn_lds[];
    float* const buf0 = gn_lds;
    float* const buf1 = buf0 + GN_TILE * GN_HID;
    float* const bs = buf1 + GN_TILE * GN_HID;
    float* const wa0 = bs + 4 * GN_HID;
    float* const ws0 = wa0 + GN_STACK_WALL;
    for (int l = 0; l < 4; ++l) {
        const int off = l == 0 ? 0 : GN_STACK_W1 + (l - 1) * GN_STACK_WH, cin = l == 0 ? 1 : GN_HID, kq = l == 0 ? 1 : 2;
        gn_stage(wa0 + off, 2, kq, a.wa[l], 1, cin, cin, GN_HID);
        if (has_ws) gn_stage(ws0 + off, 2, kq, a.ws[l], 1, cin, cin, GN_HID);
        if (threadIdx.x < GN_HID) bs[l * GN_HID + threadIdx.x] = a.b[l] ? a.b[l][threadIdx.x] : 0.0f;
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6;
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int base = tile_ptr[tile], raw = tile_ptr[tile + 1] - base;
        if (base < 0 || raw < 1 || raw > GN_TILE || base > n - raw) {
            // a caller-made cut with an empty tile, one of more rows than the LDS tile holds or one outside the batch: its rows inside
            // the batch come back as NaN (loud, nothing overrun).  A cut of tlc_gat_tile_cut never has one.
            const long long lo = base < 0 ? 0 : base, end = (long long)base + (raw < 0 ? 0 : raw), hi = end < n ? end : n;
            for (long long i = lo * GN_HID + threadIdx.x; i < hi * GN_HID; i += GN_THREADS) out[i] = __builtin_nanf("");
            continue;
        }
        const int tn = raw;
        for (int i = threadIdx.x; i < tn; i += GN_THREADS) buf1[i] = x[base + i];
        __syncthreads();
        float* in = buf1;
        float* dst = buf0;
        for (int l = 0; l < 4; ++l) {
            const int off = l == 0 ? 0 : GN_STACK_W1 + (l - 1) * GN_STACK_WH, cin = l == 0 ? 1 : GN_HID, kq = l == 0 ? 1 : 2;
            const float* const inl = in;
            auto xrow = [&](int j) -> const float* { return inl + j * cin; };
            for (int rb = wave; rb < ((tn + 15) >> 4); rb += GN_WAVES) {
                gn_f32x4 a_agg[GN_KQ];
                gn_block<2>(16 * rb, tn, base, rowptr, src, base, tn, coef, self_scale, cin, kq, l != 0, xrow, wa0 + off,
                            has_ws ? ws0 + off : nullptr, bs + l * GN_HID, GN_HID, a.act[l], a.slope[l], dst, GN_HID, a_agg);
            }
            __syncthreads();
            float* const t = in; in = dst; dst = t;
        }
        float* const og = out + (size_t)base * GN_HID;
        for (int i = threadIdx.x; i < tn * GN_HID; i += GN_THREADS) og[i] = in[i];
        __syncthreads();                                                 // (the next tile overwrites the buffers)
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
static bool gn_act_ok(int act, float slope) { return act == GN_ACT_NONE || act == GN_ACT_RELU || (act == GN_ACT_PRELU && slope > 0.0f); }

extern "C" int tlc_gnn_layer_fwd(int32_t n_nodes, const int32_t* d_rowptr, const int32_t* d_src, const float* d_coef, float self_scale,
                                 const float* d_X, int32_t c_in, int32_t c_out, const float* d_Wa, const float* d_Ws, const float* d_bias,
                                 int32_t act, float slope, float* d_out, float* d_agg, void* stream) {
    TLC_REQUIRE(n_nodes >= 0, "n_nodes < 0");
    if (!gn_width_ok(c_in, c_out)) {
        tlc_set_error("tlc_gnn_layer_fwd: c_in %d / c_out %d: built for c_in in 1 .. 64 and c_out in {8, 16, 32, 64}", c_in, c_out);
        return TLC_ERR_UNSUPPORTED;
    }
    TLC_REQUIRE(gn_act_ok(act, slope), "act: 0 none, 1 ReLU, 2 PReLU with a slope > 0");
    TLC_REQUIRE(d_rowptr && d_Wa && d_out && d_X, "null pointer");
    if (n_nodes == 0) return TLC_OK;
    int cus = 0;
    if (int rc = gn_cus(&cus)) return rc;
    const int nt = (c_out + 15) / 16 == 3 ? 4 : (c_out + 15) / 16, kq = (c_in + 15) / 16;
    const size_t lds = ((size_t)(d_Ws ? 2 : 1) * nt * kq * 256 + (size_t)GN_ROWS * c_out) * sizeof(float);   // at most 48 KiB
    const long long groups = ((long long)n_nodes + GN_ROWS - 1) / GN_ROWS;
    const unsigned grid = (unsigned)std::min<long long>(groups, (long long)cus * 4);
    GN_BY_TILES(nt, hipLaunchKernelGGL(gnn_layer_kernel<NT>, dim3(grid), dim3(GN_THREADS), lds, (hipStream_t)stream, n_nodes, d_rowptr, d_src, d_coef,
                                       self_scale, d_X, c_in, c_out, d_Wa, d_Ws, d_bias, act, slope, d_out, d_agg));
    TLC_HIP_CHECK(hipGetLastError());
    return TLC_OK;
}

extern "C" int64_t tlc_gnn_layer_bwd_work_bytes(int32_t n_nodes, int32_t c_in, int32_t c_out) {
    if (n_nodes < 0 || c_in < 0 || c_out < 0) return -1;
    return TlcGnnLayerBwdScratch(n_nodes, c_in, c_out).total * (int64_t)sizeof(float);
}

extern "C" int tlc_gnn_layer_bwd(int32_t n_nodes, const int32_t* d_rowptr_t, const int32_t* d_col_t, const float* d_coef_t, float self_scale,
                                 const float* d_X, const float* d_agg, const float* d_out, const float* d_gout, int32_t c_in, int32_t c_out,
                                 const float* d_Wa, const float* d_Ws, int32_t act, float slope, float* d_gX, float* d_gWa, float* d_gWs,
                                 float* d_gb, void* d_work, int64_t work_bytes, void* stream) {
    TLC_REQUIRE(n_nodes >= 0, "n_nodes < 0");
    if (!gn_width_ok(c_in, c_out)) {
        tlc_set_error("tlc_gnn_layer_bwd: c_in %d / c_out %d: built for c_in in 1 .. 64 and c_out in {8, 16, 32, 64}", c_in, c_out);
        return TLC_ERR_UNSUPPORTED;
    }
    TLC_REQUIRE(gn_act_ok(act, slope), "act: 0 none, 1 ReLU, 2 PReLU with a slope > 0");
    TLC_REQUIRE(d_gWa && d_Wa && (!d_gWs || d_Ws), "null pointer");
    TLC_REQUIRE(n_nodes == 0 || (d_gout && d_agg && d_work && (act == GN_ACT_NONE || d_out) && (!d_gWs || d_X)), "null pointer");
    TLC_REQUIRE(n_nodes == 0 || !d_gX || d_rowptr_t, "null pointer: d_gX needs the CSR by source");
    const TlcGnnLayerBwdScratch L(n_nodes, c_in, c_out);
    TLC_REQUIRE(n_nodes == 0 || (work_bytes >= L.total * (int64_t)sizeof(float) && ((uintptr_t)d_work & 15) == 0),
                "d_work below tlc_gnn_layer_bwd_work_bytes() or not 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    float* const work = (float*)d_work;
    float* const dZ = work ? work + L.dz : nullptr;
    if (n_nodes > 0) {
        int cus = 0;
        if (int rc = gn_cus(&cus)) return rc;
        float* const G = d_gX ? work + L.g : nullptr;
        float* const H = d_gX && d_Ws ? work + L.h : nullptr;
        const int nt = (c_in + 15) / 16 == 3 ? 4 : (c_in + 15) / 16, kq = (c_out + 15) / 16;
        const size_t lds = (size_t)2 * nt * kq * 256 * sizeof(float);                                         // at most 32 KiB
        const long long groups = ((long long)n_nodes + GN_ROWS - 1) / GN_ROWS;
        const unsigned grid = (unsigned)std::min<long long>(groups, (long long)cus * 4);
        GN_BY_TILES(nt, hipLaunchKernelGGL(gnn_bwd_rows_kernel<NT>, dim3(grid), dim3(GN_THREADS), lds, s, n_nodes, d_out, d_gout, c_in, c_out, d_Wa,
                                           d_Ws, act, slope, dZ, G, H));
        if (d_gX) {
            const long long total = (long long)n_nodes * c_in;
            hipLaunchKernelGGL(gnn_bwd_gather_kernel, dim3(tlc_grid_for(total, 256, cus * 16)), dim3(256), 0, s, total, n_nodes, c_in, d_rowptr_t,
                               d_col_t, d_coef_t, self_scale, (const float*)G, (const float*)H, d_gX);
        }
        TLC_HIP_CHECK(hipGetLastError());
    }
    // the weight gradients: tlc_gemm_tn_f32's split-K, a partition that n_nodes and the widths alone fix, partials added in split order
    float* const tn = work ? work + L.tn : nullptr;
    if (int rc = tlc_gemm_tn_f32(c_out, c_in, n_nodes, dZ, d_agg, d_gWa, tn, stream)) return rc;
    if (d_gWs)
        if (int rc = tlc_gemm_tn_f32(c_out, c_in, n_nodes, dZ, d_X, d_gWs, tn, stream)) return rc;
    if (d_gb)
        if (int rc = tlc_gemm_tn_f32(1, c_out, n_nodes, nullptr, dZ, d_gb, tn, stream)) return rc;
    return TLC_OK;
}

extern "C" int tlc_gnn_stack_fwd(int32_t n_nodes, const int32_t* d_rowptr, const int32_t* d_src, const float* d_coef, float self_scale,
                                 int32_t n_tiles, const int32_t* d_tile_ptr, const float* d_x, int32_t hidden, const float* const* params,
                                 const int32_t* acts, const float* slopes, float* d_out, void* stream) {
    TLC_REQUIRE(n_nodes >= 0 && n_tiles >= 0, "negative size");
    if (hidden != GN_HID) {
        tlc_set_error("tlc_gnn_stack_fwd: hidden %d: built for in_dim 1 and hidden 32 (run other widths layer by layer)", hidden);
        return TLC_ERR_UNSUPPORTED;
    }
    TLC_REQUIRE(params && acts && slopes, "null pointer");
    GnStackArgs a;
    bool any_ws = false, all_ws = true;
    for (int l = 0; l < 4; ++l) {
        a.wa[l] = params[3 * l]; a.ws[l] = params[3 * l + 1]; a.b[l] = params[3 * l + 2];
        a.act[l] = acts[l]; a.slope[l] = slopes[l];
        TLC_REQUIRE(a.wa[l], "null pointer (Wa)");
        TLC_REQUIRE(gn_act_ok(a.act[l], a.slope[l]), "act: 0 none, 1 ReLU, 2 PReLU with a slope > 0");
        any_ws = any_ws || a.ws[l]; all_ws = all_ws && a.ws[l];
    }
    TLC_REQUIRE(any_ws == all_ws, "Ws on all four layers or on none");
    if (n_nodes == 0 || n_tiles == 0) return TLC_OK;
    TLC_REQUIRE(d_rowptr && d_tile_ptr && d_x && d_out, "null pointer");
    const size_t lds = ((size_t)2 * GN_TILE * GN_HID + 4 * GN_HID + (size_t)(all_ws ? 2 : 1) * GN_STACK_WALL) * sizeof(float);
    constexpr size_t lds_max = ((size_t)2 * GN_TILE * GN_HID + 4 * GN_HID + (size_t)2 * GN_STACK_WALL) * sizeof(float);
    static std::mutex mu;
    static bool attr_set[64] = {};
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return TLC_ERR_HIP;
    {
        std::lock_guard<std::mutex> lock(mu);
        if (!attr_set[dev]) {
            TLC_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(gnn_stack_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max));
            attr_set[dev] = true;
        }
    }
    if (int rc = gn_cus(&cus)) return rc;
    const unsigned grid = (unsigned)std::min<long long>(n_tiles, (long long)cus * 2);
    hipLaunchKernelGGL(gnn_stack_kernel, dim3(grid), dim3(GN_THREADS), lds, (hipStream_t)stream, n_nodes, n_tiles, d_tile_ptr, d_rowptr, d_src, d_coef,
                       self_scale, d_x, a, all_ws, d_out);
    TLC_HIP_CHECK(hipGetLastError());
    return TLC_OK;
}

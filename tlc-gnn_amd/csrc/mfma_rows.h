// mfma_rows.h -- "16 node rows of a wavefront times a small weight matrix" on the f32 MFMA (v_mfma_f32_16x16x4f32), shared by the layer
// families that project node rows: gnn_layers.hip (GIN / GCN / SAGE) and msg_layers.hip (the PDGNN layer's ablations and PDConv).
// The weights are staged once per workgroup in MFMA operand layout, a lane's A operand is four consecutive floats of its row, and the
// steps run in one fixed order, so a row of the product depends on that row of A alone.
#pragma once
#include <mutex>

#include "tlc_common.h"

#define GN_THREADS 256
#define GN_WAVES (GN_THREADS / 64)
#define GN_ROWS (16 * GN_WAVES)   /* node rows per group of the layer kernels: one 16-row MFMA block per wavefront */
#define GN_KQ 4                   /* most 16-wide K blocks: widths up to 64 */
typedef float gn_f32x4 __attribute__((ext_vector_type(4)));

// W(k, c) = W[k * ldk + c * ldc] (zero outside kdim x cdim) into MFMA operand layout [t][q][e][lane]: lane (l16, g) of step (q, e)
// holds k = 16 q + 4 g + e of column 16 t + l16, so that a step's B operand is one conflict-free 256-byte row.
__device__ __forceinline__ void gn_stage(float* wt, int nt, int kq, const float* __restrict__ W, int ldk, int ldc, int kdim, int cdim) {
    const int total = nt * kq * 256;
    for (int i = threadIdx.x; i < total; i += GN_THREADS) {
        const int ln = i & 63, e = (i >> 6) & 3, q = (i >> 8) % kq, t = (i >> 8) / kq;
        const int k = 16 * q + 4 * (ln >> 4) + e, c = 16 * t + (ln & 15);
        wt[i] = (k < kdim && c < cdim) ? W[(size_t)k * ldk + (size_t)c * ldc] : 0.0f;
    }
}

// the four values k0 .. k0 + 3 of a row of `width` floats, zeros past the width (vec: width % 4 == 0 and the row 16-byte aligned)
__device__ __forceinline__ gn_f32x4 gn_load4(const float* row, int k0, int width, bool vec) {
    gn_f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (vec) {
        if (k0 < width) v = *reinterpret_cast<const gn_f32x4*>(row + k0);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (k0 + e < width) v[e] = row[k0 + e];
    }
    return v;
}

// acc[t] += A (16 x 16 kq) W (16 kq x 16 NT): steps q ascending, e = 0 .. 3 inside, the column tiles innermost
template <int NT>
__device__ __forceinline__ void gn_mma(const gn_f32x4 (&a)[GN_KQ], int kq, const float* wt, gn_f32x4 (&acc)[NT]) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int q = 0; q < GN_KQ; ++q) {
        if (q < kq) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int t = 0; t < NT; ++t)
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q][e], wt[((t * kq + q) * 4 + e) * 64 + lane], acc[t], 0, 0, 0);
        }
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
static inline int gn_cus(int* cus) {
    // per device, behind a lock: a process may drive several GPUs from several threads
    static std::mutex mu;
    static int cus_of[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return TLC_ERR_HIP;
    std::lock_guard<std::mutex> lock(mu);
    if (!cus_of[dev]) {
        int v = 0;
        TLC_HIP_CHECK(hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev));
        cus_of[dev] = v > 0 ? v : 1;
    }
    *cus = cus_of[dev];
    return TLC_OK;
}

static inline bool gn_width_ok(int c_in, int c_out) { return c_in >= 1 && c_in <= 64 && (c_out == 8 || c_out == 16 || c_out == 32 || c_out == 64); }
// column tiles of a product `width` columns wide (three tiles run as four)
static inline int gn_tiles_of(int width) { return (width + 15) / 16 == 3 ? 4 : (width + 15) / 16; }

#define GN_BY_TILES(NT_, CALL)                    \
    do {                                          \
        if ((NT_) == 1) { constexpr int NT = 1; CALL; } \
        else if ((NT_) == 2) { constexpr int NT = 2; CALL; } \
        else { constexpr int NT = 4; CALL; }      \
    } while (0)

// hks_large.hip -- tlc_hks_large_batch: heat-kernel signatures of the graphs tlc_hks_batch refuses (more than TLC_HKS_NMAX nodes, up to
// TLC_HKS_LARGE_NMAX), without eigenpairs.  hks_t(v) = [exp(-t L)]_vv, and with M = D^-1/2 A D^-1/2 (no negative entry) the normalised
// Laplacian is L = I' - M, I' the identity with a 0 for every node of degree 0, so
//   [exp(-t L)]_vv = exp(-t) [exp(t M)]_vv   for a node of degree > 0,        1 for a node of degree 0.
// Fixed parameters (they fix the bits):
//   s = the least integer >= 0 with t / 2^s <= 1/2 (at most 7 for t <= TLC_HKS_LARGE_TIME_MAX), X = (t / 2^s) M, ||X||_2 <= 1/2;
//   Taylor of degree HKSL_DEGREE = 14 by Horner:  P <- I + X / 14, then P <- I + (X P) / k for k = 13 .. 1    (0.5^15 / 15! = 2e-17);
//   the last Horner product is multiplied by exp(-t / 2^s) (the host's exp; exp(t) is never formed);
//   s - 1 squarings P <- P P; the signature is the row's sum of squares of the last P (= the diagonal of its square: P is symmetric),
//   with s = 0 the diagonal of P itself.
// Every matrix is a polynomial in the symmetric X with non-negative entries: nothing cancels, and the products compute only the tiles on
// and above the diagonal (inside a diagonal tile only the elements on and above it) and mirror them on store, so P is exactly symmetric
// and both operands of a product are read row-wise.
// Kernels: build (a workgroup per graph: checks, degrees, X), init (P <- I + X / 14), gemm (fp64 MFMA 16x16x4, HKSL_T x HKSL_T output
// tiles, K-steps of HKSL_KS through LDS, one fixed grid walking the group's list of (graph, tile row, tile column)), rows (a wavefront per
// node), norm (a workgroup per graph).  A K-sum runs in one fixed order inside one wavefront (partial sums of 64 k): no split-K, no atomics on values;
// the bits of a graph depend on the graph and the time alone.
// tlc_hks_large_batch_dt: the same products, then rows_dt / norm_dt in place of rows / norm -- the value as above and its derivative in t
// from the last P and the non-zeros of X (see hksl_rows_dt_kernel); the kernels and launches of tlc_hks_large_batch are unchanged.
#include "tlc_common.h"

#include <math.h>

#define HKSL_T 64           // side of an output tile (one 256-thread workgroup; a 32 x 32 quarter per wavefront = 2 x 2 MFMA tiles)
#define HKSL_KS 16          // K-step staged through LDS (four MFMA k-steps of 4)
#define HKSL_KCHUNK 64      // a K-sum is added up in partial sums of this many k (a multiple of HKSL_KS)
#define HKSL_LD 18          // leading dimension of a staged tile in LDS: 16-byte rows for the b128 writes, rows 16 apart on distinct banks
#define HKSL_DEGREE 14
#define HKSL_ALIGN 256

namespace {

typedef double hksl_f64x4 __attribute__((ext_vector_type(4)));

struct HkslDesc {               // one selected graph of a group (64 bytes)
    long long x_off, p0_off, p1_off;   // its three np x np matrices, in doubles from the group's matrix base
    int g;                      // index in the batch
    int n;                      // node count as the caller declared it
    int np;                     // n rounded up to HKSL_T (0: nothing to compute)
    int deg_off;                // its degrees, in ints from the group's degree base
    int pad[6];
};
static_assert(sizeof(HkslDesc) == 64, "HkslDesc is 64 bytes");

struct HkslGroup {
    const HkslDesc* descs;
    int* state;                 // per graph of the group: 1 = X is built, compute it; 0 = refused or empty
    int* deg;
    const int4* items;          // (graph of the group, tile row, tile column >= tile row, -)
    double* mats;
    int ng, n_items;
};

__device__ __forceinline__ double* hksl_mat(const HkslGroup& G, const HkslDesc& d, int sel) {
    return G.mats + (sel == 0 ? d.x_off : sel == 1 ? d.p0_off : d.p1_off);
}

// ---- setup: the group's descriptors and work items, from launch arguments (nothing is copied from host memory) -----------------------
#define HKSL_CHUNK 128
struct HkslChunk {              // HKSL_CHUNK consecutive graphs of a group and where their lists begin
    long long x_base, mat_doubles;
    int count, first, deg_base, item_base;
    int g[HKSL_CHUNK], n[HKSL_CHUNK];
};

__host__ __device__ inline int hksl_np_of(int n) { return n > TLC_HKS_LARGE_NMAX ? 0 : (n + HKSL_T - 1) / HKSL_T * HKSL_T; }

__global__ __launch_bounds__(256) void hksl_setup_kernel(HkslChunk C, HkslDesc* __restrict__ descs, int4* __restrict__ items) {
    const int k = blockIdx.x, tid = threadIdx.x;
    long long x = C.x_base;
    int dg = C.deg_base, it = C.item_base;
    for (int j = 0; j < k; ++j) {
        const int np = hksl_np_of(C.n[j]), nt = np / HKSL_T;
        x += (long long)np * np;
        dg += np;
        it += nt * (nt + 1) / 2;
    }
    const int np = hksl_np_of(C.n[k]), nt = np / HKSL_T, gi = C.first + k;
    if (tid == 0) {
        HkslDesc d;
        d.x_off = x; d.p0_off = C.mat_doubles + x; d.p1_off = 2 * C.mat_doubles + x;
        d.g = C.g[k]; d.n = C.n[k]; d.np = np; d.deg_off = dg;
        for (int i = 0; i < 6; ++i) d.pad[i] = 0;
        descs[gi] = d;
    }
    for (int a = 0; a < nt; ++a) {                             // row a of the upper triangle begins at a nt - a (a - 1) / 2
        const int base = it + a * nt - a * (a - 1) / 2 - a;
        for (int b = a + tid; b < nt; b += 256) items[base + b] = make_int4(gi, a, b, 0);
    }
}

// ---- build: one workgroup per selected graph ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hksl_build_kernel(HkslGroup G, long long total_nodes, long long total_edges, const long long* __restrict__ node_ptr,
                                                         const long long* __restrict__ edge_ptr, const int* __restrict__ edges, double scale,
                                                         unsigned char* __restrict__ status) {
    __shared__ int sdeg[TLC_HKS_LARGE_NMAX];
    __shared__ int flag[2];
    const int gi = blockIdx.x, tid = threadIdx.x;
    const HkslDesc d = G.descs[gi];
    const long long n0 = node_ptr[d.g], n1 = node_ptr[d.g + 1], e0 = edge_ptr[d.g], e1 = edge_ptr[d.g + 1];
    int st = TLC_ST_OK;
    if (n0 < 0 || n1 < n0 || n1 > total_nodes || e0 < 0 || e1 < e0 || e1 > total_edges) st = TLC_ST_BAD_INPUT;
    else if (d.n > TLC_HKS_LARGE_NMAX) st = TLC_ST_TOO_LARGE;
    else if (n1 - n0 != (long long)d.n) st = TLC_ST_BAD_INPUT;
    const int n = d.n, np = d.np;
    const long long m = e1 - e0;
    // a simple graph has at most n (n - 1) / 2 edges: more of them hold a repeat (and would be a long walk for nothing)
    if (st == TLC_ST_OK && m > (long long)n * (n - 1) / 2) st = TLC_ST_BAD_INPUT;
    if (st != TLC_ST_OK || n == 0) {
        if (tid == 0) { status[d.g] = (unsigned char)st; G.state[gi] = 0; }
        return;
    }
    for (int i = tid; i < n; i += 256) sdeg[i] = 0;
    if (tid < 2) flag[tid] = 0;
    __syncthreads();
    const int* E = edges + 2 * e0;
    for (long long e = tid; e < m; e += 256) {
        const int a = E[2 * e], b = E[2 * e + 1];
        if ((unsigned)a >= (unsigned)n || (unsigned)b >= (unsigned)n || a == b) flag[0] = 1;
        else { atomicAdd(&sdeg[a], 1); atomicAdd(&sdeg[b], 1); }
    }
    __syncthreads();
    if (flag[0]) {
        if (tid == 0) { status[d.g] = TLC_ST_BAD_INPUT; G.state[gi] = 0; }
        return;
    }
    // each unordered pair once: an integer exchange on the upper-triangle entry of the zero-filled X marks it; a mark found there is a
    // repeat, (a, b) (a, b) or (a, b) (b, a).  The marks are overwritten below (X of a refused graph is never read).
    double* X = G.mats + d.x_off;
    for (long long e = tid; e < m; e += 256) {
        const int a = E[2 * e], b = E[2 * e + 1];
        const int lo = a < b ? a : b, hi = a < b ? b : a;
        if (atomicExch(reinterpret_cast<unsigned long long*>(X + lo * np + hi), 0x3FF0000000000000ull) != 0ull) flag[1] = 1;
    }
    __syncthreads();
    if (flag[1]) {
        if (tid == 0) { status[d.g] = TLC_ST_BAD_INPUT; G.state[gi] = 0; }
        return;
    }
    for (long long e = tid; e < m; e += 256) {
        const int a = E[2 * e], b = E[2 * e + 1];
        const double v = scale * (1.0 / (sqrt((double)sdeg[a]) * sqrt((double)sdeg[b])));
        X[a * np + b] = v;
        X[b * np + a] = v;
    }
    for (int i = tid; i < n; i += 256) G.deg[d.deg_off + i] = sdeg[i];
    if (tid == 0) { status[d.g] = TLC_ST_OK; G.state[gi] = 1; }
}

// ---- init: P <- I + X / HKSL_DEGREE, tile by tile over the group's list ----------------------------------------------------------------
__global__ __launch_bounds__(256) void hksl_init_kernel(HkslGroup G, int c_sel) {
    for (int it = blockIdx.x; it < G.n_items; it += gridDim.x) {
        const int4 item = G.items[it];
        if (G.state[item.x] != 1) continue;
        const HkslDesc d = G.descs[item.x];
        const int np = d.np;
        const double* X = G.mats + d.x_off;
        double* P = hksl_mat(G, d, c_sel);
        for (int e = threadIdx.x; e < HKSL_T * HKSL_T; e += 256) {
            const int row = item.y * HKSL_T + (e >> 6), col = item.z * HKSL_T + (e & 63);
            double v = X[row * np + col] / (double)HKSL_DEGREE;
            if (row == col && row < d.n) v += 1.0;
            P[row * np + col] = v;
            if (item.y != item.z) P[col * np + row] = v;       // X is symmetric bit for bit: the build kernel wrote both entries
        }
    }
}

// ---- gemm: C <- ((A B) / div [+ I]) * mul on the tiles of the list, mirrored ------------------------------------------------------------
// A and B are symmetric, so B[k][j] is read as B[j][k]: both operands are staged as (64 rows) x (HKSL_KS of k), k contiguous.
// MFMA f64 16x16x4: lane l gives A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15]; result register r of lane l is
// D[row = (l >> 4) + 4 r][col = l & 15].
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void hksl_gemm_kernel(HkslGroup G, int a_sel, int b_sel, int c_sel, double div, double mul, int add_identity) {
    __shared__ __attribute__((aligned(16))) double As[HKSL_T * HKSL_LD];
    __shared__ __attribute__((aligned(16))) double Bs[HKSL_T * HKSL_LD];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wr = w >> 1, wc = w & 1, l16 = lane & 15, l4 = lane >> 4;
    const int srow = tid >> 2, sk = (tid & 3) * 4;             // staging: a row and four k per thread and operand
    for (int it = blockIdx.x; it < G.n_items; it += gridDim.x) {
        const int4 item = G.items[it];
        if (G.state[item.x] != 1) continue;                    // uniform over the workgroup
        const HkslDesc d = G.descs[item.x];
        const int np = d.np, ti = item.y, tj = item.z;
        const double* A = hksl_mat(G, d, a_sel) + (ti * HKSL_T + srow) * np + sk;
        const double* B = hksl_mat(G, d, b_sel) + (tj * HKSL_T + srow) * np + sk;
        double* Cm = hksl_mat(G, d, c_sel);
        const int kend = (d.n + HKSL_KS - 1) & ~(HKSL_KS - 1);  // columns n .. np-1 are zero
        // a K-sum is the sum, k ascending, of its HKSL_KCHUNK-long partial sums, each k ascending in the MFMA accumulator: one fixed
        // order, and the rounding errors of 4 096 equal terms (a star's leaves) do not pile up in one chain
        hksl_f64x4 acc[2][2], tot[2][2];
        for (int mi = 0; mi < 2; ++mi)
            for (int ni = 0; ni < 2; ++ni) { acc[mi][ni] = hksl_f64x4{0.0, 0.0, 0.0, 0.0}; tot[mi][ni] = hksl_f64x4{0.0, 0.0, 0.0, 0.0}; }
        double2 ra0 = *reinterpret_cast<const double2*>(A), ra1 = *reinterpret_cast<const double2*>(A + 2);
        double2 rb0 = *reinterpret_cast<const double2*>(B), rb1 = *reinterpret_cast<const double2*>(B + 2);
        for (int k0 = 0; k0 < kend; k0 += HKSL_KS) {
            __syncthreads();                                   // the step (or the item) before has read its tiles
            *reinterpret_cast<double2*>(&As[srow * HKSL_LD + sk]) = ra0;
            *reinterpret_cast<double2*>(&As[srow * HKSL_LD + sk + 2]) = ra1;
            *reinterpret_cast<double2*>(&Bs[srow * HKSL_LD + sk]) = rb0;
            *reinterpret_cast<double2*>(&Bs[srow * HKSL_LD + sk + 2]) = rb1;
            __syncthreads();
            if (k0 + HKSL_KS < kend) {                         // the next step's operands travel while this one multiplies
                ra0 = *reinterpret_cast<const double2*>(A + k0 + HKSL_KS);
                ra1 = *reinterpret_cast<const double2*>(A + k0 + HKSL_KS + 2);
                rb0 = *reinterpret_cast<const double2*>(B + k0 + HKSL_KS);
                rb1 = *reinterpret_cast<const double2*>(B + k0 + HKSL_KS + 2);
            }
#pragma unroll
            for (int kk = 0; kk < HKSL_KS; kk += 4) {
                double a[2], b[2];
                for (int mi = 0; mi < 2; ++mi) a[mi] = As[(wr * 32 + mi * 16 + l16) * HKSL_LD + kk + l4];
                for (int ni = 0; ni < 2; ++ni) b[ni] = Bs[(wc * 32 + ni * 16 + l16) * HKSL_LD + kk + l4];
                for (int mi = 0; mi < 2; ++mi)
                    for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[mi], b[ni], acc[mi][ni], 0, 0, 0);
            }
            if (((k0 + HKSL_KS) & (HKSL_KCHUNK - 1)) == 0 || k0 + HKSL_KS >= kend)
                for (int mi = 0; mi < 2; ++mi)
                    for (int ni = 0; ni < 2; ++ni) { tot[mi][ni] += acc[mi][ni]; acc[mi][ni] = hksl_f64x4{0.0, 0.0, 0.0, 0.0}; }
        }
        for (int mi = 0; mi < 2; ++mi)
            for (int ni = 0; ni < 2; ++ni)
                for (int r = 0; r < 4; ++r) {
                    const int row = ti * HKSL_T + wr * 32 + mi * 16 + l4 + 4 * r, col = tj * HKSL_T + wc * 32 + ni * 16 + l16;
                    if (col < row) continue;                   // a diagonal tile: its lower half is the mirror of its upper half
                    double v = tot[mi][ni][r] / div;
                    if (add_identity && row == col && row < d.n) v += 1.0;
                    v *= mul;
                    Cm[row * np + col] = v;
                    if (row != col) Cm[col * np + row] = v;
                }
    }
}

// ---- rows: a wavefront per node ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hksl_rows_kernel(HkslGroup G, const long long* __restrict__ node_ptr, int p_sel, int diag_only, double* __restrict__ out) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    for (int gi = blockIdx.y; gi < G.ng; gi += gridDim.y) {
        if (G.state[gi] != 1) continue;
        const HkslDesc d = G.descs[gi];
        if (row >= d.n) continue;
        const int np = d.np;
        const double* P = hksl_mat(G, d, p_sel) + row * np;
        double v;
        if (G.deg[d.deg_off + row] == 0) v = 1.0;
        else if (diag_only) v = P[row];
        else {
            v = 0.0;
            for (int c = lane; c < np; c += 64) { const double x = P[c]; v += x * x; }
            v += tlc_lane_xor_f64<1>(v);
            v += tlc_lane_xor_f64<2>(v);
            v += tlc_lane_xor_f64<4>(v);
            v += tlc_lane_xor_f64<8>(v);
            v += tlc_lane_xor_f64<16>(v);
            v += tlc_lane_xor_f64<32>(v);
        }
        if (lane == 0) out[node_ptr[d.g] + row] = v;
    }
}

// ---- norm: a workgroup per graph, values / (max + 1e-10) in place ---------------------------------------------------------------------
__global__ __launch_bounds__(256) void hksl_norm_kernel(HkslGroup G, const long long* __restrict__ node_ptr, double* __restrict__ out) {
    __shared__ double smax[256];
    const int gi = blockIdx.x, tid = threadIdx.x;
    if (G.state[gi] != 1) return;
    const HkslDesc d = G.descs[gi];
    double* o = out + node_ptr[d.g];
    double mx = o[0];
    for (int x = tid; x < d.n; x += 256) mx = o[x] > mx ? o[x] : mx;
    smax[tid] = mx;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) smax[tid] = smax[tid + h] > smax[tid] ? smax[tid + h] : smax[tid];
        __syncthreads();
    }
    mx = smax[0];
    for (int x = tid; x < d.n; x += 256) o[x] = o[x] / (mx + 1e-10);
}

// ---- rows with the derivative in t (tlc_hks_large_batch_dt): a wavefront per node -------------------------------------------------------
// d/dt [K_t]_vv = -[L K_t]_vv = -[K_t]_vv + sum over the neighbours u of v of [K_t]_uv / sqrt(d_u d_v), K_t = exp(-t L).  The last
// matrix P is K_t itself (diag_only: [K]_uv = P_vu) or K_t/2 ([K]_uv = sum_j P_vj P_uj, the lanes' strided sums and the butterfly of the
// value), so no further product is needed.  The neighbours are the non-zeros of row v of X (= scale * M until the next time's memset),
// walked u ascending: 64 columns at a time make one partial sum, the partial sums are added block after block -- an order the graph
// alone fixes.  at_zero (t = 0: X = 0 names no neighbour, K_0 = I'): -1 for a node of degree > 0.  Columns >= n are never a neighbour
// and are zero in P.  The value is formed exactly as in hksl_rows_kernel.
__global__ __launch_bounds__(256) void hksl_rows_dt_kernel(HkslGroup G, const long long* __restrict__ node_ptr, int p_sel, int diag_only, int at_zero,
                                                           double* __restrict__ out, double* __restrict__ dout) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    for (int gi = blockIdx.y; gi < G.ng; gi += gridDim.y) {
        if (G.state[gi] != 1) continue;
        const HkslDesc d = G.descs[gi];
        if (row >= d.n) continue;
        const int np = d.np;
        const double* Pm = hksl_mat(G, d, p_sel);
        const double* P = Pm + row * np;
        const int* deg = G.deg + d.deg_off;
        const int dv = deg[row];
        double v, dvdt = 0.0;
        if (dv == 0) v = 1.0;
        else if (diag_only) v = P[row];
        else {
            v = 0.0;
            for (int c = lane; c < np; c += 64) { const double x = P[c]; v += x * x; }
            v += tlc_lane_xor_f64<1>(v);
            v += tlc_lane_xor_f64<2>(v);
            v += tlc_lane_xor_f64<4>(v);
            v += tlc_lane_xor_f64<8>(v);
            v += tlc_lane_xor_f64<16>(v);
            v += tlc_lane_xor_f64<32>(v);
        }
        if (dv > 0 && at_zero) dvdt = -1.0;
        else if (dv > 0) {
            const double* X = G.mats + d.x_off + row * np;
            const double sv = sqrt((double)dv);
            double sum = 0.0;
            for (int c0 = 0; c0 < d.n; c0 += 64) {             // c0 + lane < np: np is a multiple of 64
                unsigned long long nb = __ballot(c0 + lane < d.n && X[c0 + lane] != 0.0);
                double part = 0.0;
                while (nb) {                                   // uniform over the wavefront
                    const int u = c0 + __ffsll((long long)nb) - 1;
                    nb &= nb - 1;
                    double k;
                    if (diag_only) k = P[u];
                    else {
                        const double* Q = Pm + u * np;
                        k = 0.0;
                        for (int c = lane; c < np; c += 64) k += P[c] * Q[c];
                        k += tlc_lane_xor_f64<1>(k);
                        k += tlc_lane_xor_f64<2>(k);
                        k += tlc_lane_xor_f64<4>(k);
                        k += tlc_lane_xor_f64<8>(k);
                        k += tlc_lane_xor_f64<16>(k);
                        k += tlc_lane_xor_f64<32>(k);
                    }
                    part += k / (sv * sqrt((double)deg[u]));
                }
                sum += part;
            }
            dvdt = sum - v;
        }
        if (lane == 0) {
            out[node_ptr[d.g] + row] = v;
            dout[node_ptr[d.g] + row] = dvdt;
        }
    }
}

// ---- norm with the derivative: a workgroup per graph.  f = hks / (mx + 1e-10), mx = hks(a) at the LOWEST index a of the maximum:
// f'(x) = (hks'(x) - f(x) hks'(a)) / (mx + 1e-10); `out` becomes what hksl_norm_kernel makes of it ---------------------------------------
__global__ __launch_bounds__(256) void hksl_norm_dt_kernel(HkslGroup G, const long long* __restrict__ node_ptr, double* __restrict__ out,
                                                           double* __restrict__ dout) {
    __shared__ double smax[256];
    __shared__ int sarg[256];
    const int gi = blockIdx.x, tid = threadIdx.x;
    if (G.state[gi] != 1) return;
    const HkslDesc d = G.descs[gi];
    double* o = out + node_ptr[d.g];
    double* dd = dout + node_ptr[d.g];
    double mx = o[0];
    int a = 0;
    for (int x = tid; x < d.n; x += 256)                       // x ascending: the first of equal values stays
        if (o[x] > mx) { mx = o[x]; a = x; }
    smax[tid] = mx;
    sarg[tid] = a;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) {
            const double m2 = smax[tid + h];
            const int a2 = sarg[tid + h];
            if (m2 > smax[tid] || (m2 == smax[tid] && a2 < sarg[tid])) { smax[tid] = m2; sarg[tid] = a2; }
        }
        __syncthreads();
    }
    mx = smax[0];
    const double da = dd[sarg[0]];
    __syncthreads();                                           // every thread holds hks'(a) before its owner overwrites it
    for (int x = tid; x < d.n; x += 256) {
        const double f = o[x] / (mx + 1e-10);
        o[x] = f;
        dd[x] = (dd[x] - f * da) / (mx + 1e-10);
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------
inline int64_t hksl_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }
inline int64_t hksl_np(int64_t n) { return n > TLC_HKS_LARGE_NMAX ? 0 : hksl_up(n, HKSL_T); }
inline int64_t hksl_tiles(int64_t np) { const int64_t nt = np / HKSL_T; return nt * (nt + 1) / 2; }
// what one selected graph adds to a group: descriptor, state, degrees, work items, three matrices
inline int64_t hksl_graph_bytes(int64_t n) {
    const int64_t np = hksl_np(n);
    return hksl_up((int64_t)sizeof(HkslDesc) + 16 + 4 * np + 16 * hksl_tiles(np), HKSL_ALIGN) + 3 * np * np * 8;
}
constexpr int64_t HKSL_GROUP_BYTES = 5 * HKSL_ALIGN;   // the alignment slack of a group's five regions

}  // namespace

extern "C" int tlc_hks_large_work_bytes(const int64_t* h_sel_nodes, int64_t n_sel, int32_t n_times, int64_t* min_bytes, int64_t* all_bytes) {
    TLC_REQUIRE(min_bytes && all_bytes, "null pointer");
    TLC_REQUIRE(n_sel >= 0 && n_sel < (1ll << 31), "bad sizes");
    TLC_REQUIRE(n_sel == 0 || h_sel_nodes, "null pointer");
    TLC_REQUIRE(n_times >= 1 && n_times <= TLC_HKS_TMAX, "n_times outside 1 .. TLC_HKS_TMAX");
    int64_t mx = 0, all = 0;
    for (int64_t i = 0; i < n_sel; ++i) {
        TLC_REQUIRE(h_sel_nodes[i] >= 0, "negative node count");
        const int64_t b = hksl_graph_bytes(h_sel_nodes[i]);
        mx = b > mx ? b : mx;
        all += b;
    }
    *min_bytes = n_sel ? mx + HKSL_GROUP_BYTES : 0;
    *all_bytes = n_sel ? all + HKSL_GROUP_BYTES : 0;
    return TLC_OK;
}

namespace {

#define HKSL_REQUIRE(cond, msg)                                                                                                                \
    do {                                                                                                                                       \
        if (!(cond)) { tlc_set_error("%s: %s", fn, msg); return TLC_ERR_INVALID_ARG; }                                                         \
    } while (0)

// tlc_hks_large_batch (d_dout == nullptr, DT false) and tlc_hks_large_batch_dt: the same checks, groups, workspace and products
template <bool DT>
int hksl_run(const char* fn, const int64_t* d_node_ptr, const int64_t* d_edge_ptr, const int32_t* d_edges, int64_t n_graphs, int64_t total_nodes,
             int64_t total_edges, const int64_t* h_sel, const int64_t* h_sel_nodes, int64_t n_sel, const double* h_times, int32_t n_times,
             uint32_t flags, double* d_out, double* d_dout, uint8_t* d_status, void* d_work, int64_t work_bytes, void* stream) {
    HKSL_REQUIRE(n_graphs >= 0 && n_graphs < (1ll << 31) && total_nodes >= 0 && total_edges >= 0, "bad sizes");
    HKSL_REQUIRE(n_sel >= 0 && n_sel <= n_graphs, "n_sel outside 0 .. n_graphs");
    HKSL_REQUIRE(h_times && n_times >= 1 && n_times <= TLC_HKS_TMAX, "n_times outside 1 .. TLC_HKS_TMAX");
    HKSL_REQUIRE((flags & ~TLC_HKS_NORMALISE) == 0, "unknown flag");
    for (int i = 0; i < n_times; ++i)
        HKSL_REQUIRE(isfinite(h_times[i]) && h_times[i] >= 0.0 && h_times[i] <= TLC_HKS_LARGE_TIME_MAX, "a time outside [0, TLC_HKS_LARGE_TIME_MAX]");
    if (DT) HKSL_REQUIRE(d_dout, "null d_dout");
    HKSL_REQUIRE(n_sel == 0 || (h_sel && h_sel_nodes), "null pointer");
    for (int64_t i = 0; i < n_sel; ++i) {
        HKSL_REQUIRE(h_sel[i] >= 0 && h_sel[i] < n_graphs && (i == 0 || h_sel[i] > h_sel[i - 1]), "h_sel is not strictly ascending inside 0 .. n_graphs-1");
        HKSL_REQUIRE(h_sel_nodes[i] >= 0, "negative node count");
    }
    if (n_sel == 0) return TLC_OK;
    HKSL_REQUIRE(d_node_ptr && d_edge_ptr && d_status && d_work && (total_nodes == 0 || d_out) && (total_edges == 0 || d_edges), "null pointer");
    int64_t min_bytes = 0, all_bytes = 0;
    const int rc = tlc_hks_large_work_bytes(h_sel_nodes, n_sel, n_times, &min_bytes, &all_bytes);
    if (rc != TLC_OK) return rc;
    HKSL_REQUIRE(work_bytes >= min_bytes, "d_work is smaller than tlc_hks_large_work_bytes()'s min_bytes");
    HKSL_REQUIRE((reinterpret_cast<uintptr_t>(d_work) & 15) == 0, "d_work must be 16-byte aligned");
    int dev = 0, cus = 0;
    TLC_HIP_CHECK(hipGetDevice(&dev));
    TLC_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    if (cus <= 0) cus = 256;
    hipStream_t s = (hipStream_t)stream;
    unsigned char* w = (unsigned char*)d_work;
    // 256-byte alignment of the regions, whatever the caller's pointer is
    const size_t skew = (size_t)((HKSL_ALIGN - (reinterpret_cast<uintptr_t>(w) & (HKSL_ALIGN - 1))) & (HKSL_ALIGN - 1));
    for (int64_t first = 0; first < n_sel;) {
        // the group: the graphs from `first` on that fit, in h_sel order (any single graph fits: work_bytes >= min_bytes)
        int64_t last = first, sum = HKSL_GROUP_BYTES, n_items = 0, deg_ints = 0, mat_doubles = 0, max_n = 0;
        while (last < n_sel && sum + hksl_graph_bytes(h_sel_nodes[last]) <= work_bytes) {
            const int64_t np = hksl_np(h_sel_nodes[last]);
            sum += hksl_graph_bytes(h_sel_nodes[last]);
            n_items += hksl_tiles(np);
            deg_ints += np;
            mat_doubles += np * np;
            if (np && h_sel_nodes[last] > max_n) max_n = h_sel_nodes[last];
            ++last;
            if (n_items > (1ll << 30) || deg_ints > (1ll << 30)) break;   // the lists are indexed with ints
        }
        const int64_t ng = last - first;
        // regions: descriptors | state | degrees | items | X of every graph | P0 of every graph | P1 of every graph
        const size_t desc_off = skew, state_off = (size_t)hksl_up(desc_off + ng * sizeof(HkslDesc), HKSL_ALIGN);
        const size_t deg_off = (size_t)hksl_up(state_off + ng * sizeof(int), HKSL_ALIGN);
        const size_t item_off = (size_t)hksl_up(deg_off + deg_ints * sizeof(int), HKSL_ALIGN);
        const size_t mat_off = (size_t)hksl_up(item_off + n_items * sizeof(int4), HKSL_ALIGN);
        if ((int64_t)(mat_off + 3 * mat_doubles * sizeof(double)) > work_bytes) {
            tlc_set_error("%s: internal: a group of %lld graphs does not fit its workspace", fn, (long long)ng);
            return TLC_ERR_INVALID_ARG;
        }
        {
            HkslChunk C;
            int64_t x = 0, dg = 0, it = 0;
            for (int64_t k0 = 0; k0 < ng; k0 += HKSL_CHUNK) {
                C.x_base = x; C.mat_doubles = mat_doubles;
                C.count = (int)(ng - k0 < HKSL_CHUNK ? ng - k0 : HKSL_CHUNK);
                C.first = (int)k0; C.deg_base = (int)dg; C.item_base = (int)it;
                for (int k = 0; k < HKSL_CHUNK; ++k) {
                    const int64_t n = k < C.count ? h_sel_nodes[first + k0 + k] : 0;
                    C.g[k] = k < C.count ? (int)h_sel[first + k0 + k] : 0;
                    C.n[k] = n > TLC_HKS_LARGE_NMAX ? TLC_HKS_LARGE_NMAX + 1 : (int)n;   // (the build kernel answers TLC_ST_TOO_LARGE)
                    const int64_t np = hksl_np(n);
                    x += np * np; dg += np; it += hksl_tiles(np);
                }
                hipLaunchKernelGGL(hksl_setup_kernel, dim3((unsigned)C.count), dim3(256), 0, s, C, reinterpret_cast<HkslDesc*>(w + desc_off),
                                   reinterpret_cast<int4*>(w + item_off));
                TLC_HIP_CHECK(hipGetLastError());
            }
        }
        HkslGroup G;
        G.descs = reinterpret_cast<const HkslDesc*>(w + desc_off);
        G.state = reinterpret_cast<int*>(w + state_off);
        G.deg = reinterpret_cast<int*>(w + deg_off);
        G.items = reinterpret_cast<const int4*>(w + item_off);
        G.mats = reinterpret_cast<double*>(w + mat_off);
        G.ng = (int)ng;
        G.n_items = (int)n_items;
        const unsigned grid_items = (unsigned)(n_items < 4ll * cus ? n_items : 4ll * cus);
        for (int t = 0; t < n_times; ++t) {
            const double time = h_times[t];
            int sq = 0;
            while (ldexp(time, -sq) > 0.5) ++sq;               // t / 2^sq <= 1/2, exact
            const double scale = ldexp(time, -sq), factor = exp(-scale);
            if (mat_doubles) TLC_HIP_CHECK(hipMemsetAsync(G.mats, 0, mat_doubles * sizeof(double), s));
            hipLaunchKernelGGL(hksl_build_kernel, dim3((unsigned)ng), dim3(256), 0, s, G, (long long)total_nodes, (long long)total_edges,
                               (const long long*)d_node_ptr, (const long long*)d_edge_ptr, (const int*)d_edges, scale, d_status);
            TLC_HIP_CHECK(hipGetLastError());
            if (!n_items) continue;
            int cur = 1;                                       // which of P0 (1) / P1 (2) holds P
            hipLaunchKernelGGL(hksl_init_kernel, dim3(grid_items), dim3(256), 0, s, G, cur);
            TLC_HIP_CHECK(hipGetLastError());
            for (int k = HKSL_DEGREE - 1; k >= 1; --k) {       // P <- I + (X P) / k; the last one times exp(-t / 2^sq)
                hipLaunchKernelGGL(hksl_gemm_kernel, dim3(grid_items), dim3(256), 0, s, G, 0, cur, 3 - cur, (double)k, k == 1 ? factor : 1.0, 1);
                TLC_HIP_CHECK(hipGetLastError());
                cur = 3 - cur;
            }
            for (int q = 0; q + 1 < sq; ++q) {                 // sq - 1 squarings; the last one is the rows kernel's sum of squares
                hipLaunchKernelGGL(hksl_gemm_kernel, dim3(grid_items), dim3(256), 0, s, G, cur, cur, 3 - cur, 1.0, 1.0, 0);
                TLC_HIP_CHECK(hipGetLastError());
                cur = 3 - cur;
            }
            double* out_t = d_out + (size_t)t * (size_t)total_nodes;
            const unsigned gy = (unsigned)(ng < 65535 ? ng : 65535);
            if (DT) {                                          // the value as below and its derivative in t, from the same last matrix
                double* dout_t = d_dout + (size_t)t * (size_t)total_nodes;
                hipLaunchKernelGGL(hksl_rows_dt_kernel, dim3((unsigned)((max_n + 3) / 4), gy), dim3(256), 0, s, G, (const long long*)d_node_ptr,
                                   cur, sq == 0 ? 1 : 0, time == 0.0 ? 1 : 0, out_t, dout_t);
                TLC_HIP_CHECK(hipGetLastError());
                if (flags & TLC_HKS_NORMALISE) {
                    hipLaunchKernelGGL(hksl_norm_dt_kernel, dim3((unsigned)ng), dim3(256), 0, s, G, (const long long*)d_node_ptr, out_t, dout_t);
                    TLC_HIP_CHECK(hipGetLastError());
                }
                continue;
            }
            hipLaunchKernelGGL(hksl_rows_kernel, dim3((unsigned)((max_n + 3) / 4), gy), dim3(256), 0, s, G, (const long long*)d_node_ptr, cur,
                               sq == 0 ? 1 : 0, out_t);
            TLC_HIP_CHECK(hipGetLastError());
            if (flags & TLC_HKS_NORMALISE) {
                hipLaunchKernelGGL(hksl_norm_kernel, dim3((unsigned)ng), dim3(256), 0, s, G, (const long long*)d_node_ptr, out_t);
                TLC_HIP_CHECK(hipGetLastError());
            }
        }
        first = last;
    }
    return TLC_OK;
}
#undef HKSL_REQUIRE

}  // namespace

extern "C" int tlc_hks_large_batch(const int64_t* d_node_ptr, const int64_t* d_edge_ptr, const int32_t* d_edges, int64_t n_graphs, int64_t total_nodes,
                                   int64_t total_edges, const int64_t* h_sel, const int64_t* h_sel_nodes, int64_t n_sel, const double* h_times,
                                   int32_t n_times, uint32_t flags, double* d_out, uint8_t* d_status, void* d_work, int64_t work_bytes, void* stream) {
    return hksl_run<false>(__func__, d_node_ptr, d_edge_ptr, d_edges, n_graphs, total_nodes, total_edges, h_sel, h_sel_nodes, n_sel, h_times, n_times,
                           flags, d_out, nullptr, d_status, d_work, work_bytes, stream);
}

extern "C" int tlc_hks_large_batch_dt(const int64_t* d_node_ptr, const int64_t* d_edge_ptr, const int32_t* d_edges, int64_t n_graphs,
                                      int64_t total_nodes, int64_t total_edges, const int64_t* h_sel, const int64_t* h_sel_nodes, int64_t n_sel,
                                      const double* h_times, int32_t n_times, uint32_t flags, double* d_out, double* d_dout, uint8_t* d_status,
                                      void* d_work, int64_t work_bytes, void* stream) {
    return hksl_run<true>(__func__, d_node_ptr, d_edge_ptr, d_edges, n_graphs, total_nodes, total_edges, h_sel, h_sel_nodes, n_sel, h_times, n_times,
                          flags, d_out, d_dout, d_status, d_work, work_bytes, stream);
}

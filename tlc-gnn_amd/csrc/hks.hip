// hks.hip -- tlc_hks_batch: the heat-kernel-signature filtration of a packed batch of graphs (Knowledge_Distillation/data_utils_LP.py:96-100,
// 128-130; data_utils_NC.py:88-92,120-122; data_utils_GC.py:90-94,114-116 of the reference: scipy's normalised Laplacian, a dense eigh and
// sum_k exp(-t lambda_k) phi_k(x)^2 per graph, then / (max + 1e-10)).
//
// Eigensolver: cyclic two-sided Jacobi with accumulated vectors in its parallel form.  The indices 0 .. ne-1 (ne = n rounded up to even; an
// odd graph gets one idle index whose row and column stay zero) are paired by the round-robin ("circle") schedule: ne/2 disjoint pairs per
// round, ne - 1 rounds per sweep, every pair once.  A round is
//   phase 1  one thread per pair (p, q): the rotation (c, s) that annihilates a_pq, from a_pp, a_qq, a_pq alone; the 2 x 2 diagonal block is
//            updated in closed form (a_pp - t a_pq, a_qq + t a_pq, 0);
//   phase 2  one thread per pair of pairs k < l: the 2 x 2 block A[{p_k,q_k}, {p_l,q_l}] <- J_k^T B J_l, written to both triangles (the
//            matrix stays exactly symmetric), and one thread per (pair, column) of V^T: rows p, q <- J_k^T rows.
// Every element is computed by ONE thread from a fixed formula, so the bits do not depend on the thread count, on the tier's memory
// (LDS or the workspace) or on what else is in the batch.  -ffp-contract=off (the Makefile's default): no FMA contraction either.
// Stop rule: a rotation is skipped when |a_pq| <= 1e-15 / ne; a sweep that skips all of them has found every off-diagonal entry at or
// below that, i.e. off-diagonal norm <= ne * max <= 1e-15 <= 1e-15 * ||L||_F (a graph with an edge has ||L||_F >= sqrt(2)).  Degenerate
// spectra need no care: only sum over an eigenspace of phi^2 enters the signature.  More than TLC_HKS_MAX_SWEEPS sweeps: status byte
// TLC_ST_NOT_CONVERGED, nothing written.
// Input check: ids outside 0 .. n-1 and self loops while the degrees are counted; an unordered pair listed twice (either orientation)
// after L is built, by counting the non-zeros of every column against the degree (integers only) -- TLC_ST_BAD_INPUT, nothing written.
//
// Tiers by node count, binned ON THE DEVICE from node_ptr (the host knows B and the two totals only); every tier is a persistent loop that
// draws graphs from its list by a ticket counter:
//   WAVE   n <= 32   one wavefront per graph, four per workgroup; A and V^T (32 x 33 fp64 each) in LDS, 17.4 KiB per wavefront
//   WG64   n <= 64   one 256-thread workgroup per graph, 67.2 KiB of LDS: two workgroups per CU
//   WG96   n <= 96   one workgroup per graph, 149.6 KiB of LDS (two 96 x 97 fp64 arrays are what fits the 160 KiB)
//   GLOBAL n <= TLC_HKS_NMAX = 256   one 1 024-thread workgroup per graph (its rounds wait on L2: more loads in flight), A and V^T in the
//                                     workgroup's slot of the caller's workspace (1.0 MiB), rotations and the pair table in LDS
// Leading dimension NMAX + 1 (odd): a column walk of the fp64 array touches every bank pair once.
//
// tlc_hks_batch_dt: the same tiers instantiated with DT, which add per time one more pass of the signature's loop with the weights
// -lambda_k exp(-t lambda_k) -- d/dt of the row just stored, into a second output; cs and vals are reused, no further LDS.  The kernels of
// tlc_hks_batch are the instantiations without DT and hold none of it.
#include "tlc_common.h"

#include <algorithm>

#define TLC_HKS_MAX_SWEEPS 40
#define HKS_WAVE_N 32
#define HKS_WG64_N 64
#define HKS_WG96_N TLC_HKS_LDS_NMAX
#define HKS_HEAD_BYTES 256          // tier counts [4], tickets [4]

namespace {

struct HksTimes { double t[TLC_HKS_TMAX]; };

template <bool WAVE>
__device__ __forceinline__ void hks_sync() {
    if (WAVE) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    } else {
        __syncthreads();
    }
}

// pair k of round r of the circle schedule over ne indices (ne even, M = ne - 1): index M stays, the others rotate
__device__ __forceinline__ void hks_pair(int k, int r, int M, int& p, int& q) {
    int a, b;
    if (k == 0) { a = M; b = r; }
    else {
        a = r + k; if (a >= M) a -= M;
        b = r - k; if (b < 0) b += M;
    }
    p = a < b ? a : b;
    q = a < b ? b : a;
}

constexpr int hks_tab_entries(int nmax) { return (nmax / 2) * (nmax / 2 - 1) / 2; }
// LDS of one unit (a wavefront of WAVE, a workgroup otherwise): [A, V^T unless GLOBAL] cs[NMAX] vals[NMAX] deg[NMAX] flag[4] tab[]
constexpr size_t hks_lds_bytes(int nmax, bool global) {
    return ((global ? 0 : 2 * (size_t)nmax * (nmax + 1) * 8) + 2 * (size_t)nmax * 8 + (size_t)nmax * 4 + 16 + (size_t)hks_tab_entries(nmax) * 2 + 15) & ~(size_t)15;
}

// One graph on NT threads (tid = 0 .. NT-1).  A, Vt: (NMAX) x (NMAX + 1) fp64 each, LDS or global.  Returns the status byte (uniform).
// DT: row ti of `dout` is d/dt of what row ti of `out` holds (tlc_hks_batch_dt); without it `dout` is unused and nothing below changes.
template <int NMAX, int NT, bool WAVE, bool DT>
__device__ __forceinline__ int hks_graph(double* A, double* Vt, double* cs, double* vals, int* deg, int* flag, unsigned short* tab, int tid,
                                         int n, int m, const int* __restrict__ edges, const HksTimes& times, int T, unsigned flags,
                                         double* __restrict__ out, double* __restrict__ dout, long long out_stride) {
    constexpr int ld = NMAX + 1;
    const int ne = (n + 1) & ~1, h = ne >> 1, M = ne - 1;
    for (int i = tid; i < ne * ld; i += NT) { A[i] = 0.0; Vt[i] = 0.0; }
    for (int i = tid; i < ne; i += NT) deg[i] = 0;
    if (tid == 0) flag[0] = 0;
    hks_sync<WAVE>();
    for (int e = tid; e < m; e += NT) {
        const int a = edges[2 * e], b = edges[2 * e + 1];
        if ((unsigned)a >= (unsigned)n || (unsigned)b >= (unsigned)n || a == b) flag[0] = 1;
        else { atomicAdd(&deg[a], 1); atomicAdd(&deg[b], 1); }
    }
    hks_sync<WAVE>();
    if (flag[0]) return TLC_ST_BAD_INPUT;
    // L = I - D^-1/2 A D^-1/2 as scipy.sparse.csgraph.laplacian(normed=True): a node of degree 0 has diagonal 0
    for (int e = tid; e < m; e += NT) {
        const int a = edges[2 * e], b = edges[2 * e + 1];
        const double v = -1.0 / (sqrt((double)deg[a]) * sqrt((double)deg[b]));
        A[a * ld + b] = v;
        A[b * ld + a] = v;
    }
    for (int i = tid; i < ne; i += NT) {
        Vt[i * ld + i] = 1.0;
        if (i < n && deg[i] > 0) A[i * ld + i] = 1.0;
    }
    for (int k = tid; k < h; k += NT) {                        // the pairs of pairs k < l, row by row
        const int base = k * h - k * (k + 1) / 2;
        for (int l = k + 1; l < h; ++l) tab[base + l - k - 1] = (unsigned short)(k | (l << 8));
    }
    hks_sync<WAVE>();
    // each edge once: a repeated pair {a, b} went into deg twice but is ONE entry of L (scipy would sum it into a multigraph weight), so
    // column i then holds fewer non-zeros than deg[i] off-diagonals plus its diagonal.  Counting only: no value of L changes.
    for (int i = tid; i < n; i += NT) {
        int cnt = 0;
        for (int j = 0; j < n; ++j) cnt += A[j * ld + i] != 0.0;
        if (cnt != deg[i] + (deg[i] > 0)) flag[0] = 1;
    }
    hks_sync<WAVE>();
    if (flag[0]) return TLC_ST_BAD_INPUT;

    const double tol = 1e-15 / (double)ne;
    const int nblocks = h * (h - 1) / 2, nvt = h * ne;
    const unsigned magic = 0xFFFFFFFFu / (unsigned)ne + 1u;   // t / ne = umulhi(t, magic), exact for t * ne < 2^32
    bool converged = false;
    for (int sweep = 0; sweep < TLC_HKS_MAX_SWEEPS; ++sweep) {
        if (tid == 0) flag[1] = 0;
        hks_sync<WAVE>();
        for (int r = 0; r < M; ++r) {
            for (int k = tid; k < h; k += NT) {
                int p, q;
                hks_pair(k, r, M, p, q);
                const double apq = A[p * ld + q];
                double c = 1.0, s = 0.0;
                if (fabs(apq) > tol) {
                    const double app = A[p * ld + p], aqq = A[q * ld + q];
                    const double theta = (aqq - app) / (2.0 * apq);
                    double t;
                    if (fabs(theta) > 1e150) t = 0.5 / theta;            // theta^2 would overflow
                    else t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                    c = 1.0 / sqrt(t * t + 1.0);
                    s = t * c;
                    A[p * ld + p] = app - t * apq;
                    A[q * ld + q] = aqq + t * apq;
                    A[p * ld + q] = 0.0;
                    A[q * ld + p] = 0.0;
                    flag[1] = 1;
                }
                cs[2 * k] = c;
                cs[2 * k + 1] = s;
            }
            hks_sync<WAVE>();
            for (int t = tid; t < nblocks; t += NT) {
                const int kl = tab[t], k = kl & 255, l = kl >> 8;
                const double ck = cs[2 * k], sk = cs[2 * k + 1], cl = cs[2 * l], sl = cs[2 * l + 1];
                if (sk == 0.0 && sl == 0.0) continue;                    // both rotations are the identity
                int pk, qk, pl, ql;
                hks_pair(k, r, M, pk, qk);
                hks_pair(l, r, M, pl, ql);
                const double b00 = A[pk * ld + pl], b01 = A[pk * ld + ql], b10 = A[qk * ld + pl], b11 = A[qk * ld + ql];
                const double t00 = ck * b00 - sk * b10, t01 = ck * b01 - sk * b11;
                const double t10 = sk * b00 + ck * b10, t11 = sk * b01 + ck * b11;
                const double o00 = cl * t00 - sl * t01, o01 = sl * t00 + cl * t01;
                const double o10 = cl * t10 - sl * t11, o11 = sl * t10 + cl * t11;
                A[pk * ld + pl] = o00; A[pl * ld + pk] = o00;
                A[pk * ld + ql] = o01; A[ql * ld + pk] = o01;
                A[qk * ld + pl] = o10; A[pl * ld + qk] = o10;
                A[qk * ld + ql] = o11; A[ql * ld + qk] = o11;
            }
            for (int t = tid; t < nvt; t += NT) {
                const int k = (int)__umulhi((unsigned)t, magic), i = t - k * ne;
                const double c = cs[2 * k], s = cs[2 * k + 1];
                if (s == 0.0) continue;
                int p, q;
                hks_pair(k, r, M, p, q);
                const double vp = Vt[p * ld + i], vq = Vt[q * ld + i];
                Vt[p * ld + i] = c * vp - s * vq;
                Vt[q * ld + i] = s * vp + c * vq;
            }
            hks_sync<WAVE>();
        }
        const int rotated = flag[1];
        hks_sync<WAVE>();
        if (!rotated) { converged = true; break; }
    }
    if (!converged) return TLC_ST_NOT_CONVERGED;

    // hks(x) = sum_k exp(-t lambda_k) phi_k(x)^2, k ascending; row k of V^T is phi_k (the idle index of an odd graph adds an exact 0)
    for (int ti = 0; ti < T; ++ti) {
        const double time = times.t[ti];
        for (int k = tid; k < ne; k += NT) cs[k] = exp(-time * A[k * ld + k]);
        hks_sync<WAVE>();
        for (int x = tid; x < n; x += NT) {
            double acc = 0.0;
            for (int k = 0; k < ne; ++k) {
                const double v = Vt[k * ld + x];
                acc += (v * v) * cs[k];
            }
            vals[x] = acc;
        }
        hks_sync<WAVE>();
        double mx = vals[0];
        if (flags & TLC_HKS_NORMALISE)
            for (int x = 1; x < n; ++x) mx = vals[x] > mx ? vals[x] : mx;
        for (int x = tid; x < n; x += NT)
            out[(long long)ti * out_stride + x] = (flags & TLC_HKS_NORMALISE) ? vals[x] / (mx + 1e-10) : vals[x];
        hks_sync<WAVE>();
        if constexpr (DT) {
            // d/dt hks(x) = - sum_k lambda_k exp(-t lambda_k) phi_k(x)^2: the same loop, k ascending, over cs and vals again.  Normalised,
            // f = hks / (mx + 1e-10) with mx = hks(a), a the LOWEST index of the maximum:  f'(x) = (hks'(x) - f(x) hks'(a)) / (mx + 1e-10)
            int a = 0;
            if (flags & TLC_HKS_NORMALISE) {
                double top = vals[0];
                for (int x = 1; x < n; ++x)
                    if (vals[x] > top) { top = vals[x]; a = x; }
            }
            hks_sync<WAVE>();                                  // every thread has read vals
            for (int k = tid; k < ne; k += NT) {
                const double lam = A[k * ld + k];
                cs[k] = -lam * exp(-time * lam);
            }
            hks_sync<WAVE>();
            for (int x = tid; x < n; x += NT) {
                double acc = 0.0;
                for (int k = 0; k < ne; ++k) {
                    const double v = Vt[k * ld + x];
                    acc += (v * v) * cs[k];
                }
                vals[x] = acc;
            }
            hks_sync<WAVE>();
            const double da = vals[a];
            for (int x = tid; x < n; x += NT) {
                const long long o = (long long)ti * out_stride + x;
                dout[o] = (flags & TLC_HKS_NORMALISE) ? (vals[x] - out[o] * da) / (mx + 1e-10) : vals[x];   // out[o]: this thread's store
            }
            hks_sync<WAVE>();
        }
    }
    return TLC_ST_OK;
}

// ---- binning: one thread per graph ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hks_bin_kernel(long long B, long long total_nodes, long long total_edges, const long long* __restrict__ node_ptr,
                                                      const long long* __restrict__ edge_ptr, int* __restrict__ head, int* __restrict__ lists,
                                                      unsigned char* __restrict__ status) {
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    int tier = -1;
    if (g < B) {
        const long long n0 = node_ptr[g], n1 = node_ptr[g + 1], e0 = edge_ptr[g], e1 = edge_ptr[g + 1];
        const long long n = n1 - n0;
        if (n0 < 0 || n1 < n0 || n1 > total_nodes || e0 < 0 || e1 < e0 || e1 > total_edges) status[g] = TLC_ST_BAD_INPUT;
        else if (n > TLC_HKS_NMAX) status[g] = TLC_ST_TOO_LARGE;
        else {
            status[g] = TLC_ST_OK;
            if (n > 0) tier = n <= HKS_WAVE_N ? 0 : n <= HKS_WG64_N ? 1 : n <= HKS_WG96_N ? 2 : 3;
        }
    }
    // one atomic per wavefront and tier (41 127 molecule graphs on one counter took 0.44 ms, a lane each)
    for (int t = 0; t < 4; ++t) {
        const unsigned long long mask = __ballot(tier == t);
        if (!mask) continue;
        int base = 0;
        if (tlc_lane() == __ffsll((long long)mask) - 1) base = atomicAdd(&head[t], __popcll(mask));
        base = __shfl(base, __ffsll((long long)mask) - 1);
        if (tier == t) lists[(long long)t * B + base + __popcll(mask & tlc_lanemask_lt())] = (int)g;
    }
}

// ---- tier kernels ------------------------------------------------------------------------------------------------------------------
constexpr int hks_threads(bool wave, bool global) { return wave ? 64 : global ? 1024 : 256; }
constexpr int hks_block(bool global) { return global ? 1024 : 256; }

template <int NMAX, bool WAVE, bool GLOBAL, bool DT>
__device__ __forceinline__ void hks_tier_body(int tier, long long B, const long long* __restrict__ node_ptr, const long long* __restrict__ edge_ptr,
                                              const int* __restrict__ edges, const HksTimes& times, int T, unsigned flags, double* __restrict__ out,
                                              double* __restrict__ dout, long long out_stride, unsigned char* __restrict__ status,
                                              int* __restrict__ head, const int* __restrict__ lists, double* __restrict__ slots) {
    extern __shared__ __attribute__((aligned(16))) unsigned char hks_smem[];
    constexpr int NT = hks_threads(WAVE, GLOBAL);
    constexpr size_t UNIT = hks_lds_bytes(NMAX, GLOBAL);
    constexpr size_t MAT = (size_t)NMAX * (NMAX + 1);
    const int tid = WAVE ? (int)(threadIdx.x & 63) : (int)threadIdx.x;
    unsigned char* base = hks_smem + (WAVE ? (size_t)(threadIdx.x >> 6) * UNIT : 0);
    double* A = GLOBAL ? slots + (size_t)blockIdx.x * 2 * MAT : reinterpret_cast<double*>(base);
    double* Vt = A + MAT;
    double* cs = reinterpret_cast<double*>(base + (GLOBAL ? 0 : 2 * MAT * 8));
    double* vals = cs + NMAX;
    int* deg = reinterpret_cast<int*>(vals + NMAX);
    int* flag = deg + NMAX;
    unsigned short* tab = reinterpret_cast<unsigned short*>(flag + 4);
    const int count = head[tier];
    const int* list = lists + (long long)tier * B;
    for (;;) {
        int i;
        if (WAVE) {
            i = tid == 0 ? atomicAdd(&head[4 + tier], 1) : 0;
            i = __builtin_amdgcn_readfirstlane(i);
        } else {
            if (tid == 0) flag[2] = atomicAdd(&head[4 + tier], 1);
            __syncthreads();
            i = flag[2];
            __syncthreads();
        }
        if (i >= count) break;
        const int g = list[i];
        const long long n0 = node_ptr[g], e0 = edge_ptr[g];
        const int n = (int)(node_ptr[g + 1] - n0), m = (int)(edge_ptr[g + 1] - e0);
        const int st = hks_graph<NMAX, NT, WAVE, DT>(A, Vt, cs, vals, deg, flag, tab, tid, n, m, edges + 2 * e0, times, T, flags, out + n0,
                                                     DT ? dout + n0 : nullptr, out_stride);
        if (tid == 0 && st != TLC_ST_OK) status[g] = (unsigned char)st;
        hks_sync<WAVE>();
    }
}

template <int NMAX, bool WAVE, bool GLOBAL>
__global__ __launch_bounds__(hks_block(GLOBAL)) void hks_tier_kernel(int tier, long long B, const long long* __restrict__ node_ptr, const long long* __restrict__ edge_ptr,
                                                       const int* __restrict__ edges, HksTimes times, int T, unsigned flags, double* __restrict__ out,
                                                       long long out_stride, unsigned char* __restrict__ status, int* __restrict__ head,
                                                       const int* __restrict__ lists, double* __restrict__ slots) {
    hks_tier_body<NMAX, WAVE, GLOBAL, false>(tier, B, node_ptr, edge_ptr, edges, times, T, flags, out, nullptr, out_stride, status, head, lists, slots);
}

// the same tiers with the derivative in t (tlc_hks_batch_dt): one more row per time, written to dout
template <int NMAX, bool WAVE, bool GLOBAL>
__global__ __launch_bounds__(hks_block(GLOBAL)) void hks_tier_dt_kernel(int tier, long long B, const long long* __restrict__ node_ptr, const long long* __restrict__ edge_ptr,
                                                       const int* __restrict__ edges, HksTimes times, int T, unsigned flags, double* __restrict__ out,
                                                       double* __restrict__ dout, long long out_stride, unsigned char* __restrict__ status,
                                                       int* __restrict__ head, const int* __restrict__ lists, double* __restrict__ slots) {
    hks_tier_body<NMAX, WAVE, GLOBAL, true>(tier, B, node_ptr, edge_ptr, edges, times, T, flags, out, dout, out_stride, status, head, lists, slots);
}

struct HksLayout {
    int cus, slots;
    size_t lists_off, slots_off, bytes;
};

int hks_layout(int64_t B, int64_t total_nodes, HksLayout* L) {
    int dev = 0, cus = 0;
    TLC_HIP_CHECK(hipGetDevice(&dev));
    TLC_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    if (cus <= 0) cus = 256;
    L->cus = cus;
    // one slot of matrices per resident workgroup of the GLOBAL tier; a batch of total_nodes nodes holds at most total_nodes / 97 such graphs
    const int64_t most = total_nodes / (HKS_WG96_N + 1);
    L->slots = (int)(most < cus ? most : cus);
    L->lists_off = HKS_HEAD_BYTES;
    L->slots_off = (L->lists_off + (size_t)4 * (size_t)B * sizeof(int) + 255) & ~(size_t)255;
    L->bytes = L->slots_off + (size_t)L->slots * 2 * TLC_HKS_NMAX * (TLC_HKS_NMAX + 1) * sizeof(double);
    return TLC_OK;
}

}  // namespace

extern "C" int tlc_hks_batch_work_bytes(int64_t n_graphs, int64_t total_nodes, int64_t total_edges, int32_t n_times, int64_t* bytes) {
    TLC_REQUIRE(bytes, "null pointer");
    TLC_REQUIRE(n_graphs >= 0 && n_graphs < (1ll << 31) && total_nodes >= 0 && total_edges >= 0, "bad sizes");
    TLC_REQUIRE(n_times >= 1 && n_times <= TLC_HKS_TMAX, "n_times outside 1 .. TLC_HKS_TMAX");
    HksLayout L;
    const int rc = hks_layout(n_graphs, total_nodes, &L);
    if (rc != TLC_OK) return rc;
    *bytes = (int64_t)L.bytes;
    return TLC_OK;
}

namespace {

// tlc_hks_batch (d_dout == nullptr, DT false) and tlc_hks_batch_dt: the same checks, workspace, binning and grids
template <bool DT>
int hks_run(const char* fn, const int64_t* d_node_ptr, const int64_t* d_edge_ptr, const int32_t* d_edges, int64_t n_graphs, int64_t total_nodes,
            int64_t total_edges, const double* h_times, int32_t n_times, uint32_t flags, double* d_out, double* d_dout, uint8_t* d_status,
            void* d_work, int64_t work_bytes, void* stream) {
#define HKS_REQUIRE(cond, msg)                                                                                                                 \
    do {                                                                                                                                       \
        if (!(cond)) { tlc_set_error("%s: %s", fn, msg); return TLC_ERR_INVALID_ARG; }                                                         \
    } while (0)
    HKS_REQUIRE(n_graphs >= 0 && n_graphs < (1ll << 31) && total_nodes >= 0 && total_edges >= 0, "bad sizes");
    HKS_REQUIRE(h_times && n_times >= 1 && n_times <= TLC_HKS_TMAX, "n_times outside 1 .. TLC_HKS_TMAX");
    HKS_REQUIRE((flags & ~TLC_HKS_NORMALISE) == 0, "unknown flag");
    if (DT) HKS_REQUIRE(d_dout, "null d_dout");
    if (n_graphs == 0) return TLC_OK;
    HKS_REQUIRE(d_node_ptr && d_edge_ptr && d_status && d_work && (total_nodes == 0 || d_out) && (total_edges == 0 || d_edges), "null pointer");
    HksLayout L;
    const int rc = hks_layout(n_graphs, total_nodes, &L);
    if (rc != TLC_OK) return rc;
    HKS_REQUIRE(work_bytes >= (int64_t)L.bytes, "d_work is smaller than tlc_hks_batch_work_bytes()");
    HKS_REQUIRE((reinterpret_cast<uintptr_t>(d_work) & 15) == 0, "d_work must be 16-byte aligned");
#undef HKS_REQUIRE
    HksTimes times;
    for (int i = 0; i < TLC_HKS_TMAX; ++i) times.t[i] = i < n_times ? h_times[i] : 0.0;
    hipStream_t s = (hipStream_t)stream;
    unsigned char* w = (unsigned char*)d_work;
    int* head = (int*)w;
    int* lists = (int*)(w + L.lists_off);
    double* slots = (double*)(w + L.slots_off);
    const long long B = n_graphs;
    TLC_HIP_CHECK(hipMemsetAsync(head, 0, HKS_HEAD_BYTES, s));
    hipLaunchKernelGGL(hks_bin_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, B, (long long)total_nodes, (long long)total_edges,
                       (const long long*)d_node_ptr, (const long long*)d_edge_ptr, head, lists, d_status);
    TLC_HIP_CHECK(hipGetLastError());

    constexpr size_t lds_wave = 4 * hks_lds_bytes(HKS_WAVE_N, false), lds64 = hks_lds_bytes(HKS_WG64_N, false);
    constexpr size_t lds96 = hks_lds_bytes(HKS_WG96_N, false), lds_gl = hks_lds_bytes(TLC_HKS_NMAX, true);
    static_assert(2 * lds_wave <= 160 * 1024 && 2 * lds64 <= 160 * 1024 && lds96 <= 160 * 1024, "LDS budget of a gfx950 CU");
    if (DT) {
        TLC_HIP_CHECK(hipFuncSetAttribute((const void*)hks_tier_dt_kernel<HKS_WAVE_N, true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_wave));
        TLC_HIP_CHECK(hipFuncSetAttribute((const void*)hks_tier_dt_kernel<HKS_WG64_N, false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds64));
        TLC_HIP_CHECK(hipFuncSetAttribute((const void*)hks_tier_dt_kernel<HKS_WG96_N, false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds96));
    } else {
        TLC_HIP_CHECK(hipFuncSetAttribute((const void*)hks_tier_kernel<HKS_WAVE_N, true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_wave));
        TLC_HIP_CHECK(hipFuncSetAttribute((const void*)hks_tier_kernel<HKS_WG64_N, false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds64));
        TLC_HIP_CHECK(hipFuncSetAttribute((const void*)hks_tier_kernel<HKS_WG96_N, false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds96));
    }
    const long long cus = L.cus;
    // a graph of the WG tiers has at least 33 / 65 nodes: no more workgroups than the batch can hold such graphs
    const long long g_wave = std::min<long long>((B + 3) / 4, 2 * cus);
    const long long g64 = std::min<long long>(std::min<long long>(B, total_nodes / (HKS_WAVE_N + 1)), 2 * cus);
    const long long g96 = std::min<long long>(std::min<long long>(B, total_nodes / (HKS_WG64_N + 1)), cus);
    const long long stride = total_nodes;
#define HKS_LAUNCH(NMAX, WAVE, GLOBAL, tier, grid, lds)                                                                                        \
    if ((grid) > 0) {                                                                                                                          \
        if (DT)                                                                                                                                \
            hipLaunchKernelGGL((hks_tier_dt_kernel<NMAX, WAVE, GLOBAL>), dim3((unsigned)(grid)), dim3(hks_block(GLOBAL)), lds, s, tier, B,     \
                               (const long long*)d_node_ptr, (const long long*)d_edge_ptr, d_edges, times, (int)n_times, flags, d_out, d_dout, \
                               stride, d_status, head, lists, slots);                                                                          \
        else                                                                                                                                   \
            hipLaunchKernelGGL((hks_tier_kernel<NMAX, WAVE, GLOBAL>), dim3((unsigned)(grid)), dim3(hks_block(GLOBAL)), lds, s, tier, B, (const long long*)d_node_ptr, \
                               (const long long*)d_edge_ptr, d_edges, times, (int)n_times, flags, d_out, stride, d_status, head, lists, slots); \
        TLC_HIP_CHECK(hipGetLastError());                                                                                                      \
    }
    HKS_LAUNCH(HKS_WAVE_N, true, false, 0, g_wave, lds_wave)
    HKS_LAUNCH(HKS_WG64_N, false, false, 1, g64, lds64)
    HKS_LAUNCH(HKS_WG96_N, false, false, 2, g96, lds96)
    HKS_LAUNCH(TLC_HKS_NMAX, false, true, 3, (long long)L.slots, lds_gl)
#undef HKS_LAUNCH
    return TLC_OK;
}

}  // namespace

extern "C" int tlc_hks_batch(const int64_t* d_node_ptr, const int64_t* d_edge_ptr, const int32_t* d_edges, int64_t n_graphs, int64_t total_nodes,
                             int64_t total_edges, const double* h_times, int32_t n_times, uint32_t flags, double* d_out, uint8_t* d_status,
                             void* d_work, int64_t work_bytes, void* stream) {
    return hks_run<false>(__func__, d_node_ptr, d_edge_ptr, d_edges, n_graphs, total_nodes, total_edges, h_times, n_times, flags, d_out, nullptr,
                          d_status, d_work, work_bytes, stream);
}

extern "C" int tlc_hks_batch_dt(const int64_t* d_node_ptr, const int64_t* d_edge_ptr, const int32_t* d_edges, int64_t n_graphs, int64_t total_nodes,
                                int64_t total_edges, const double* h_times, int32_t n_times, uint32_t flags, double* d_out, double* d_dout,
                                uint8_t* d_status, void* d_work, int64_t work_bytes, void* stream) {
    return hks_run<true>(__func__, d_node_ptr, d_edge_ptr, d_edges, n_graphs, total_nodes, total_edges, h_times, n_times, flags, d_out, d_dout,
                         d_status, d_work, work_bytes, stream);
}

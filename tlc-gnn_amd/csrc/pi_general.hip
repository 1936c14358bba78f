// pi_general.hip -- the general persistence imager (tlc_pi_image, tlc_pi_image_vjp): any grid up to TLC_PI_MAX_RES lines
// a side, any ramp, any positive-definite 2 x 2 covariance with |r| < 0.925, explicit weights, with or without the skew.
//
// Replaces PersistenceImager.transform of Knowledge_Distillation/pimg.py:354-414 (and of sg2dgm/PersistenceImager.pyx:352-403) beyond the
// one configuration tlc_pi_raster computes.  The image is always row-major [birth_bin, pers_bin].
//
//   cov == 0   a point contributes w * outer(dPhi_b, dPhi_p), so a diagram's image is U^T V with U[i, :] = w_i dPhi_b(i) and
//              V[i, :] = dPhi_p(i).  Work item = (diagram, image tile, slice of PIG_SLICE points).  Images up to 32 x 32 take one
//              wavefront per item (one 32 x 32 tile), larger ones a 256-thread workgroup per 64 x 64 tile.  Per chunk of PIG_C
//              points the two factor tables go to LDS -- one erfc per (point, grid line), not per pixel: thread (point, axis,
//              segment of lines) walks its lines and keeps the CDF of the line before in a register -- and the rank-PIG_C update of
//              the tile is v_mfma_f64_16x16x4_f64, 2 x 2 MFMA tiles per wavefront, accumulators in registers across the slice.
//   cov != 0   the bivariate normal CDF at every grid corner (Drezner-Wesolowsky: Gauss-Legendre over the correlation, 6, 12 or 20
//              nodes for |r| < 0.3, < 0.75, beyond), the four-corner inclusion-exclusion per point BEFORE the sum over the points.
//              Work item = (diagram, 32 x 32 tile, slice): per point the lines' (z, Phi), then the 33 x 33 corners into LDS, then
//              four pixels per thread.
// Summation order of a pixel: the points of a slice ascending (inside the MFMA, groups of four ascending), the slices ascending in
// a second pass (pig_reduce_kernel).  A slice is PIG_SLICE points whatever the batch, the grid of workgroups or the workspace, and
// there is no floating-point atomic: a diagram's bits depend on its points and the specification alone.
//
// The grid lines travel by value (the host's linspace bits, no uniform step assumed); so do the specification and the list of
// K-split diagrams of a launch (at most PIG_GROUP): the entries read nothing back and upload nothing.
#include "scratch_layouts.h"
#include "tlc_common.h"

#include <math.h>

namespace {

#define PIG_SLICE TlcPiImageScratch::SLICE
#define PIG_GROUP TlcPiImageScratch::MAX_GROUP
#define PIG_C 32                      // points per chunk (eight MFMA k-steps)
#define PIG_LD (PIG_C + 2)            // a table row in LDS: 16 rows x 2 k of a half-wavefront's operand read fall on distinct banks
#define PIG_MAX_GRID 8192
#define PIG_CT 32                     // tile side of the correlated path
#define PIG_MAXQ 20
static_assert(PIG_SLICE % PIG_C == 0, "whole chunks");

typedef double pig_f64x4 __attribute__((ext_vector_type(4)));

struct PigGrid {
    double b[TLC_PI_MAX_RES + 1], p[TLC_PI_MAX_RES + 1];
};
struct PigSpec {
    int Rb, Rp, skew, nq;                       // nq: quadrature terms of the correlated path (0: separable)
    double low, high, start, end, slope;        // the ramp and its slope inside [start, end]
    double sd_b, sd_p, asr;                     // square roots of the variances; asin(r)
    double sn[PIG_MAXQ], den[PIG_MAXQ], qw[PIG_MAXQ];   // sin(asr (1 -+ x) / 2), 1 - sn^2, the node's weight
};
struct PigArgs {
    int n_dgms;
    long long n_pts;
    const long long* offs;
    const double *pts, *wts;
    double *out, *partial;
    PigSpec S;
};
// the K-split diagrams of one launch (n == 0: the launch of the diagrams up to PIG_SLICE points)
struct PigGroup {
    int n;
    int dgm[PIG_GROUP], cnt[PIG_GROUP], slice0[PIG_GROUP + 1];
    long long p0[PIG_GROUP];
};
struct PigItem {
    int tb, tp, cnt;
    long long p0;
    double* dst;          // the image (or partial image) the tile belongs to, row-major [Rb, Rp]
};

__device__ __forceinline__ double pig_phi(double z) { return 0.5 * erfc(-z / 1.4142135623730951); }
__device__ __forceinline__ double pig_ramp(const PigSpec& S, double x) {
    return x < S.start ? S.low : (x > S.end ? S.high : (x - S.start) * (S.high - S.low) / (S.end - S.start) + S.low);
}
__device__ __forceinline__ void pig_point(const PigArgs& A, long long i, double& b, double& x) {
    b = A.pts[2 * i];
    const double d = A.pts[2 * i + 1];
    x = A.S.skew ? d - b : d;
}
__device__ __forceinline__ double pig_weight(const PigArgs& A, long long i, double x) { return A.wts ? A.wts[i] : pig_ramp(A.S, x); }
__device__ __forceinline__ long long pig_clamp(long long v, long long hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// item `it` of a launch over tiles of side T; false: nothing to do (a K-split diagram in the plain launch)
template <int T>
__device__ __forceinline__ bool pig_item(const PigArgs& A, const PigGroup& Gp, long long it, PigItem& I) {
    const int ntp = (A.S.Rp + T - 1) / T, nt = ((A.S.Rb + T - 1) / T) * ntp;
    const long long RR = (long long)A.S.Rb * A.S.Rp;
    const long long q = it / nt;
    const int tile = (int)(it - q * nt);
    I.tb = tile / ntp;
    I.tp = tile - I.tb * ntp;
    if (Gp.n == 0) {
        const long long a = pig_clamp(A.offs[q], A.n_pts), e = pig_clamp(A.offs[q + 1], A.n_pts);
        if (e - a > PIG_SLICE) return false;
        I.p0 = a;
        I.cnt = e > a ? (int)(e - a) : 0;
        I.dst = A.out + q * RR;
        return true;
    }
    int j = 0;
    while (j + 1 < Gp.n && Gp.slice0[j + 1] <= q) ++j;
    const int s = (int)q - Gp.slice0[j];
    const long long done = (long long)s * PIG_SLICE;
    I.p0 = Gp.p0[j] + done;
    I.cnt = Gp.cnt[j] - done < PIG_SLICE ? (int)(Gp.cnt[j] - done) : (int)PIG_SLICE;
    I.dst = A.partial + q * RR;
    return true;
}
__host__ __device__ inline long long pig_n_items(int n_dgms, const PigGroup& Gp, int Rb, int Rp, int T) {
    const long long nt = (long long)((Rb + T - 1) / T) * ((Rp + T - 1) / T);
    return (Gp.n ? (long long)Gp.slice0[Gp.n] : (long long)n_dgms) * nt;
}

// ---- cov == 0 ----------------------------------------------------------------------------------------------------------------------
// NW x NW wavefronts, a 32 x 32 quarter of the (32 NW)-sided tile each.  MFMA f64 16x16x4: lane l gives A[i = l & 15][k = l >> 4] and
// B[k = l >> 4][j = l & 15]; result register r of lane l is D[row = (l >> 4) + 4 r][col = l & 15] (as in hks_large.hip).
template <int NW>
__global__ __launch_bounds__(64 * NW * NW) void pig_sep_kernel(PigArgs A, PigGrid G, PigGroup Gp) {
    constexpr int T = 32 * NW, NSEG = NW * NW, SL = T / NSEG;
    __shared__ double Us[T * PIG_LD], Vs[T * PIG_LD];
    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wr = w / NW, wc = w % NW, l16 = lane & 15, l4 = lane >> 4;
    const int pi = tid & 31, axis = (tid >> 5) & 1, seg = tid >> 6;       // stage 1: a point of the chunk, an axis, a segment of lines
    const long long n_items = pig_n_items(A.n_dgms, Gp, A.S.Rb, A.S.Rp, T);
    for (long long it = blockIdx.x; it < n_items; it += gridDim.x) {
        PigItem I;
        if (!pig_item<T>(A, Gp, it, I)) continue;                          // uniform over the workgroup
        const int r0 = I.tb * T, c0 = I.tp * T;
        const int nr = A.S.Rb - r0 < T ? A.S.Rb - r0 : T, nc = A.S.Rp - c0 < T ? A.S.Rp - c0 : T;
        pig_f64x4 acc[2][2];
        for (int mi = 0; mi < 2; ++mi)
            for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = pig_f64x4{0.0, 0.0, 0.0, 0.0};
        for (int base = 0; base < I.cnt; base += PIG_C) {
            const int m = I.cnt - base < PIG_C ? I.cnt - base : PIG_C;
            __syncthreads();                                               // the chunk (or the item) before has read its tables
            {
                double* Tab = axis ? Vs : Us;
                const int nl = axis ? nc : nr, g0 = seg * SL;
                if (pi < m) {
                    double b, x;
                    pig_point(A, I.p0 + base + pi, b, x);
                    const double wgt = axis ? 1.0 : pig_weight(A, I.p0 + base + pi, x);
                    const double c = axis ? x : b, sd = axis ? A.S.sd_p : A.S.sd_b;
                    const double* gl = axis ? G.p + c0 : G.b + r0;
                    double prev = g0 < nl ? pig_phi((gl[g0] - c) / sd) : 0.0;
                    for (int g = g0; g < g0 + SL; ++g) {
                        double v = 0.0;
                        if (g < nl) {
                            const double cur = pig_phi((gl[g + 1] - c) / sd);
                            v = wgt * (cur - prev);
                            prev = cur;
                        }
                        Tab[g * PIG_LD + pi] = v;
                    }
                } else {
                    for (int g = g0; g < g0 + SL; ++g) Tab[g * PIG_LD + pi] = 0.0;   // (0 x NaN of a table row is not wanted)
                }
            }
            __syncthreads();
            const int kmax = (m + 3) & ~3;
            for (int kk = 0; kk < kmax; kk += 4) {
                double a[2], b[2];
                for (int mi = 0; mi < 2; ++mi) a[mi] = Us[(wr * 32 + mi * 16 + l16) * PIG_LD + kk + l4];
                for (int ni = 0; ni < 2; ++ni) b[ni] = Vs[(wc * 32 + ni * 16 + l16) * PIG_LD + kk + l4];
                for (int mi = 0; mi < 2; ++mi)
                    for (int ni = 0; ni < 2; ++ni)
                        if (wr * 32 + mi * 16 < nr && wc * 32 + ni * 16 < nc)      // uniform over the wavefront
                            acc[mi][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[mi], b[ni], acc[mi][ni], 0, 0, 0);
            }
        }
        for (int mi = 0; mi < 2; ++mi)
            for (int ni = 0; ni < 2; ++ni)
                for (int r = 0; r < 4; ++r) {
                    const int row = wr * 32 + mi * 16 + l4 + 4 * r, col = wc * 32 + ni * 16 + l16;
                    if (row < nr && col < nc) I.dst[(long long)(r0 + row) * A.S.Rp + c0 + col] = acc[mi][ni][r];
                }
    }
}

// ---- cov != 0 ----------------------------------------------------------------------------------------------------------------------
// P(X <= x, Y <= y) of the standardised pair with correlation r = sin(asr), from zb = (x - mu_x) / sd_x, zp = (y - mu_y) / sd_y and
// their univariate CDFs:  Phi(zb) Phi(zp) + asr / (4 pi) * sum_t w_t exp((sn_t zb zp - (zb^2 + zp^2) / 2) / (1 - sn_t^2))
__device__ __forceinline__ double pig_bvn(const PigSpec& S, double zb, double zp, double Pb, double Pp) {
    const double hk = zb * zp, hs = (zb * zb + zp * zp) / 2.0;
    double s = 0.0;
    for (int t = 0; t < S.nq; ++t) s += S.qw[t] * exp((S.sn[t] * hk - hs) / S.den[t]);
    return S.asr * s / (4.0 * 3.14159265358979323846) + Pb * Pp;
}

__global__ __launch_bounds__(256) void pig_corr_kernel(PigArgs A, PigGrid G, PigGroup Gp) {
    constexpr int T = PIG_CT, L = PIG_CT + 1;
    __shared__ double sZ[2][2][L], sP[2][2][L];          // [buffer][axis][line]
    __shared__ double sC[2][L * L];                      // [buffer][corner]
    const int tid = (int)threadIdx.x;
    const long long n_items = pig_n_items(A.n_dgms, Gp, A.S.Rb, A.S.Rp, T);
    for (long long it = blockIdx.x; it < n_items; it += gridDim.x) {
        PigItem I;
        if (!pig_item<T>(A, Gp, it, I)) continue;
        const int r0 = I.tb * T, c0 = I.tp * T;
        const int nr = A.S.Rb - r0 < T ? A.S.Rb - r0 : T, nc = A.S.Rp - c0 < T ? A.S.Rp - c0 : T;
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        __syncthreads();                                 // the item before has read its last corners
        for (int i = 0; i < I.cnt; ++i) {
            const int buf = i & 1;
            double b, x;
            pig_point(A, I.p0 + i, b, x);
            const double wgt = pig_weight(A, I.p0 + i, x);
            if (tid <= nr) {
                const double z = (G.b[r0 + tid] - b) / A.S.sd_b;
                sZ[buf][0][tid] = z; sP[buf][0][tid] = pig_phi(z);
            } else if (tid >= 64 && tid - 64 <= nc) {
                const double z = (G.p[c0 + tid - 64] - x) / A.S.sd_p;
                sZ[buf][1][tid - 64] = z; sP[buf][1][tid - 64] = pig_phi(z);
            }
            __syncthreads();
            for (int e = tid; e < (nr + 1) * (nc + 1); e += 256) {
                const int gr = e / (nc + 1), gc = e - gr * (nc + 1);
                sC[buf][gr * L + gc] = pig_bvn(A.S, sZ[buf][0][gr], sZ[buf][1][gc], sP[buf][0][gr], sP[buf][1][gc]);
            }
            __syncthreads();
            // (two buffers: the lines and corners of point i + 1 are written while a slower wavefront still reads those of point i;
            //  point i + 2 reuses them behind the two barriers of point i + 1)
            const double* Cn = sC[buf];
            for (int q = 0; q < 4; ++q) {
                const int pix = tid + 256 * q, pr = pix >> 5, pc = pix & 31;
                if (pr < nr && pc < nc)
                    acc[q] += wgt * (Cn[(pr + 1) * L + pc + 1] - Cn[pr * L + pc + 1] - Cn[(pr + 1) * L + pc] + Cn[pr * L + pc]);
            }
        }
        for (int q = 0; q < 4; ++q) {
            const int pix = tid + 256 * q, pr = pix >> 5, pc = pix & 31;
            if (pr < nr && pc < nc) I.dst[(long long)(r0 + pr) * A.S.Rp + c0 + pc] = acc[q];
        }
    }
}

// ---- the second pass of the K-split diagrams: a pixel's slices ascending ----------------------------------------------------------
__global__ __launch_bounds__(256) void pig_reduce_kernel(PigGroup Gp, int RR, const double* __restrict__ partial, double* __restrict__ out) {
    const long long total = (long long)Gp.n * RR;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const int j = (int)(e / RR), pix = (int)(e - (long long)j * RR);
        const int s0 = Gp.slice0[j], s1 = Gp.slice0[j + 1];
        double v = partial[(long long)s0 * RR + pix];
        for (int s = s0 + 1; s < s1; ++s) v += partial[(long long)s * RR + pix];
        out[(long long)Gp.dgm[j] * RR + pix] = v;
    }
}

// ---- backward: one wavefront per point ----------------------------------------------------------------------------------------------
// The point's line tables go to LDS (Phi, and the density / sd of TLC_PI_GRAD_FULL or z of the correlated path); lane l contracts the
// pixels l, l + 64, ... ascending with grad_img, the lanes are folded by the butterfly l ^ 1, l ^ 2, ... l ^ 32: one fixed order.
__device__ __forceinline__ double pig_wave_sum(double v) {
    v += tlc_lane_xor_f64<1>(v);
    v += tlc_lane_xor_f64<2>(v);
    v += tlc_lane_xor_f64<4>(v);
    v += tlc_lane_xor_f64<8>(v);
    v += tlc_lane_xor_f64<16>(v);
    v += tlc_lane_xor_f64<32>(v);
    return v;
}

__global__ __launch_bounds__(64) void pig_vjp_kernel(PigArgs A, PigGrid G, int full, const double* __restrict__ gimg, double* __restrict__ gpts) {
    constexpr int L = TLC_PI_MAX_RES + 1;
    __shared__ double sPb[L], sPp[L], sQb[L], sQp[L];
    const int lane = (int)threadIdx.x;
    const int Rb = A.S.Rb, Rp = A.S.Rp, RR = Rb * Rp;
    const bool corr = A.S.nq != 0;
    for (long long i = blockIdx.x; i < A.n_pts; i += gridDim.x) {
        double b, x;
        pig_point(A, i, b, x);
        const double slope = (x >= A.S.start && x <= A.S.end) ? A.S.slope : 0.0;
        if (!full && !(slope != 0.0)) {                  // uniform over the workgroup: the weight does not move
            if (lane == 0) { gpts[2 * i] = 0.0; gpts[2 * i + 1] = 0.0; }
            continue;
        }
        int lo = 0, hi = A.n_dgms;                       // offs[lo] <= i < offs[hi]
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (A.offs[mid] <= i) lo = mid; else hi = mid; }
        const double* gi = gimg + (long long)lo * RR;
        __syncthreads();                                 // the point before has read its tables
        for (int g = lane; g <= Rb; g += 64) {
            const double z = (G.b[g] - b) / A.S.sd_b;
            sPb[g] = pig_phi(z);
            sQb[g] = corr ? z : exp(-0.5 * (z * z)) * 0.3989422804014327 / A.S.sd_b;
        }
        for (int g = lane; g <= Rp; g += 64) {
            const double z = (G.p[g] - x) / A.S.sd_p;
            sPp[g] = pig_phi(z);
            sQp[g] = corr ? z : exp(-0.5 * (z * z)) * 0.3989422804014327 / A.S.sd_p;
        }
        __syncthreads();
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        for (int p = lane; p < RR; p += 64) {
            const int r = p / Rp, c = p - r * Rp;
            const double gv = gi[p];
            if (!corr) {
                const double db = sPb[r + 1] - sPb[r], dp = sPp[c + 1] - sPp[c];
                s0 += gv * (db * dp);
                if (full) {
                    s1 += gv * ((sQb[r + 1] - sQb[r]) * dp);
                    s2 += gv * (db * (sQp[c + 1] - sQp[c]));
                }
            } else {
                const double c11 = pig_bvn(A.S, sQb[r + 1], sQp[c + 1], sPb[r + 1], sPp[c + 1]);
                const double c01 = pig_bvn(A.S, sQb[r], sQp[c + 1], sPb[r], sPp[c + 1]);
                const double c10 = pig_bvn(A.S, sQb[r + 1], sQp[c], sPb[r + 1], sPp[c]);
                const double c00 = pig_bvn(A.S, sQb[r], sQp[c], sPb[r], sPp[c]);
                s0 += gv * (c11 - c01 - c10 + c00);
            }
        }
        s0 = pig_wave_sum(s0);
        if (full) { s1 = pig_wave_sum(s1); s2 = pig_wave_sum(s2); }
        if (lane == 0) {
            // d Phi((g - c) / sd) / d c = -density / sd: the tables hold +density / sd
            double gb = 0.0, gx = slope * s0;
            if (full) {
                const double wgt = pig_ramp(A.S, x);
                gb = -(wgt * s1);
                gx -= wgt * s2;
            }
            gpts[2 * i] = A.S.skew ? gb - gx : gb;       // x = death - birth under the skew
            gpts[2 * i + 1] = gx;
        }
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------------
// the positive nodes (descending) and their weights of the 6-, 12- and 20-point Gauss-Legendre rules (numpy.polynomial.legendre.leggauss)
const double PIG_GL6_X[3] = {0.93246951420315205, 0.66120938646626448, 0.23861918608319693};
const double PIG_GL6_W[3] = {0.17132449237916975, 0.36076157304813894, 0.46791393457269137};
const double PIG_GL12_X[6] = {0.98156063424671924, 0.9041172563704748, 0.76990267419430469, 0.58731795428661748, 0.36783149899818018,
                              0.12523340851146891};
const double PIG_GL12_W[6] = {0.047175336386512022, 0.10693932599531888, 0.16007832854334611, 0.20316742672306565, 0.23349253653835464,
                              0.24914704581340269};
const double PIG_GL20_X[10] = {0.99312859918509488, 0.96397192727791381, 0.91223442825132584, 0.83911697182221878, 0.7463319064601508,
                               0.63605368072651502, 0.51086700195082713, 0.37370608871541955, 0.2277858511416451,  0.076526521133497338};
const double PIG_GL20_W[10] = {0.017614007139153273, 0.040601429800386217, 0.062672048334109443, 0.083276741576704671, 0.10193011981724026,
                               0.11819453196151825,  0.13168863844917653,  0.14209610931838187,  0.14917298647260366,  0.15275338713072578};

#define PIG_REFUSE(cond, ...)                   \
    do {                                        \
        if (!(cond)) {                          \
            tlc_set_error(__VA_ARGS__);         \
            return TLC_ERR_INVALID_ARG;         \
        }                                       \
    } while (0)

// the specification of both entries, checked: every refusal of the header
int pig_make_spec(const char* fn, int32_t res_b, int32_t res_p, const double* h_bpnts, const double* h_ppnts, const double* h_ramp,
                  const double* h_sigma, int32_t skew, PigSpec& S, PigGrid& G) {
    PIG_REFUSE(res_b >= 1 && res_b <= TLC_PI_MAX_RES && res_p >= 1 && res_p <= TLC_PI_MAX_RES,
               "%s: resolution (%d, %d) outside 1 .. TLC_PI_MAX_RES = %d", fn, (int)res_b, (int)res_p, TLC_PI_MAX_RES);
    PIG_REFUSE(h_bpnts && h_ppnts && h_ramp && h_sigma, "%s: null pointer in the specification", fn);
    for (int a = 0; a < 2; ++a) {
        const double* src = a ? h_ppnts : h_bpnts;
        double* dst = a ? G.p : G.b;
        const int n = (a ? res_p : res_b) + 1;
        for (int g = 0; g < n; ++g) {
            PIG_REFUSE(isfinite(src[g]), "%s: %s grid line %d is not finite", fn, a ? "persistence" : "birth", g);
            PIG_REFUSE(g == 0 || src[g] > src[g - 1], "%s: the %s grid lines are not strictly increasing at line %d", fn,
                       a ? "persistence" : "birth", g);
            dst[g] = src[g];
        }
        for (int g = n; g <= TLC_PI_MAX_RES; ++g) dst[g] = dst[n - 1];
    }
    const double low = h_ramp[0], high = h_ramp[1], start = h_ramp[2], end = h_ramp[3];
    PIG_REFUSE(isfinite(low) && isfinite(high) && isfinite(start) && isfinite(end), "%s: the ramp (low, high, start, end) is not finite", fn);
    PIG_REFUSE(end > start, "%s: the ramp needs end > start (start %g, end %g)", fn, start, end);
    const double vb = h_sigma[0], vp = h_sigma[1], cov = h_sigma[2];
    PIG_REFUSE(isfinite(vb) && isfinite(vp) && isfinite(cov), "%s: sigma is not finite", fn);
    PIG_REFUSE(vb > 0.0 && vp > 0.0 && vb * vp - cov * cov > 0.0,
               "%s: sigma [[%g, %g], [%g, %g]] is singular or not positive definite", fn, vb, cov, cov, vp);
    S.Rb = res_b; S.Rp = res_p; S.skew = skew ? 1 : 0; S.nq = 0;
    S.low = low; S.high = high; S.start = start; S.end = end; S.slope = (high - low) / (end - start);
    S.sd_b = sqrt(vb); S.sd_p = sqrt(vp); S.asr = 0.0;
    for (int t = 0; t < PIG_MAXQ; ++t) { S.sn[t] = 0.0; S.den[t] = 1.0; S.qw[t] = 0.0; }
    PIG_REFUSE(isfinite(S.slope) && isfinite(S.sd_b) && isfinite(S.sd_p), "%s: the ramp's slope or sigma's square roots overflow", fn);
    if (cov != 0.0) {
        const double r = cov / sqrt(vb * vp);
        PIG_REFUSE(fabs(r) < 0.925,
                   "%s: correlation r = %g: |r| >= 0.925 is refused (the reference's branch for it is wrong by 0.15 at |r| = 0.95 and "
                   "is not reproduced)", fn, r);
        const int lg = fabs(r) < 0.3 ? 3 : (fabs(r) < 0.75 ? 6 : 10);
        const double* X = lg == 3 ? PIG_GL6_X : (lg == 6 ? PIG_GL12_X : PIG_GL20_X);
        const double* W = lg == 3 ? PIG_GL6_W : (lg == 6 ? PIG_GL12_W : PIG_GL20_W);
        S.asr = asin(r);
        S.nq = 2 * lg;
        for (int j = 0; j < lg; ++j)
            for (int h = 0; h < 2; ++h) {
                const double sn = sin(S.asr * (h ? 1.0 + X[j] : 1.0 - X[j]) / 2.0);
                S.sn[2 * j + h] = sn; S.den[2 * j + h] = 1.0 - sn * sn; S.qw[2 * j + h] = W[j];
            }
    }
    return TLC_OK;
}

int64_t pig_bytes(int64_t doubles) { return doubles > 0 ? doubles * 8 + 256 : 0; }     // (room for tlc_align256)

}  // namespace

extern "C" int64_t tlc_pi_image_work_bytes(int32_t n_dgms, int64_t max_points, int32_t res_b, int32_t res_p, int64_t* least) {
    if (n_dgms < 0 || max_points < 0 || res_b < 1 || res_b > TLC_PI_MAX_RES || res_p < 1 || res_p > TLC_PI_MAX_RES) {
        tlc_set_error("%s: negative size or a resolution outside 1 .. %d", __func__, TLC_PI_MAX_RES);
        return -1;
    }
    const TlcPiImageScratch L(n_dgms, max_points, res_b, res_p);
    if (least) *least = pig_bytes(L.least);
    return pig_bytes(L.total);
}

extern "C" int tlc_pi_image(int32_t n_dgms, int64_t n_pts, const int64_t* d_offs, const int64_t* h_offs, const double* d_pts,
                            const double* d_weights, int32_t res_b, int32_t res_p, const double* h_bpnts, const double* h_ppnts,
                            const double* h_ramp, const double* h_sigma, int32_t skew, double* d_out, void* d_work, int64_t work_bytes,
                            void* stream) {
    TLC_REQUIRE(n_dgms >= 0 && n_pts >= 0 && work_bytes >= 0, "negative size");
    PigArgs A;
    PigGrid G;
    const int rc = pig_make_spec(__func__, res_b, res_p, h_bpnts, h_ppnts, h_ramp, h_sigma, skew, A.S, G);
    if (rc != TLC_OK) return rc;
    if (n_dgms == 0) return TLC_OK;
    TLC_REQUIRE(d_offs && h_offs && d_out && (n_pts == 0 || d_pts), "null pointer");
    TLC_REQUIRE(h_offs[0] >= 0 && h_offs[n_dgms] <= n_pts, "the offsets leave 0 .. n_pts");
    int64_t max_points = 0;
    for (int32_t q = 0; q < n_dgms; ++q) {
        const int64_t n = h_offs[q + 1] - h_offs[q];
        if (n < 0) { tlc_set_error("%s: the offsets of diagram %d decrease", __func__, (int)q); return TLC_ERR_INVALID_ARG; }
        if (n > max_points) max_points = n;
    }
    if (max_points > 0x7FFFFFFF) { tlc_set_error("%s: a diagram of 2^31 points or more", __func__); return TLC_ERR_UNSUPPORTED; }
    const TlcPiImageScratch L(n_dgms, max_points, res_b, res_p);
    if (L.least > 0 && (!d_work || work_bytes < pig_bytes(L.least))) {
        tlc_set_error("%s: d_work holds %lld bytes; a diagram of %lld points at %d x %d needs %lld (tlc_pi_image_work_bytes)", __func__,
                      (long long)(d_work ? work_bytes : 0), (long long)max_points, (int)res_b, (int)res_p, (long long)pig_bytes(L.least));
        return TLC_ERR_INVALID_ARG;
    }
    hipStream_t st = (hipStream_t)stream;
    A.n_dgms = n_dgms; A.n_pts = n_pts;
    A.offs = (const long long*)d_offs; A.pts = d_pts; A.wts = d_weights;
    A.out = d_out; A.partial = L.least > 0 ? (double*)tlc_align256(d_work) : nullptr;
    const bool corr = A.S.nq != 0, small = res_b <= 32 && res_p <= 32;
    auto launch = [&](const PigGroup& Gp) {
        const int T = corr ? PIG_CT : (small ? 32 : 64);
        const long long items = pig_n_items(n_dgms, Gp, res_b, res_p, T);
        const unsigned grid = (unsigned)(items < 1 ? 1 : (items > PIG_MAX_GRID ? PIG_MAX_GRID : items));
        if (corr) hipLaunchKernelGGL(pig_corr_kernel, dim3(grid), dim3(256), 0, st, A, G, Gp);
        else if (small) hipLaunchKernelGGL(pig_sep_kernel<1>, dim3(grid), dim3(64), 0, st, A, G, Gp);
        else hipLaunchKernelGGL(pig_sep_kernel<2>, dim3(grid), dim3(256), 0, st, A, G, Gp);
    };
    PigGroup Gp;
    memset(&Gp, 0, sizeof(Gp));
    launch(Gp);                                              // every diagram of up to PIG_SLICE points (the others are skipped)
    if (L.least > 0) {
        // the K-split diagrams, as many per launch as the workspace holds slices for (at most PIG_GROUP)
        const int64_t RR = (int64_t)res_b * res_p;
        const int64_t cap = (work_bytes - 256) / 8 / RR;     // slices of room (>= those of the largest diagram: checked above)
        auto flush = [&]() {
            if (!Gp.n) return;
            launch(Gp);
            hipLaunchKernelGGL(pig_reduce_kernel, dim3(tlc_grid_for((long long)Gp.n * RR, 256, 2048)), dim3(256), 0, st, Gp, (int)RR,
                               (const double*)A.partial, d_out);
            memset(&Gp, 0, sizeof(Gp));
        };
        for (int32_t q = 0; q < n_dgms; ++q) {
            const int64_t n = h_offs[q + 1] - h_offs[q];
            const int64_t ns = TlcPiImageScratch::slices_of(n);
            if (!ns) continue;
            if (Gp.n == PIG_GROUP || Gp.slice0[Gp.n] + ns > cap) flush();
            Gp.dgm[Gp.n] = q; Gp.p0[Gp.n] = h_offs[q]; Gp.cnt[Gp.n] = (int)n;
            Gp.slice0[Gp.n + 1] = Gp.slice0[Gp.n] + (int)ns;
            ++Gp.n;
        }
        flush();
    }
    TLC_HIP_CHECK(hipGetLastError());
    return TLC_OK;
}

extern "C" int tlc_pi_image_vjp(int32_t n_dgms, int64_t n_pts, const int64_t* d_offs, const double* d_pts, int32_t res_b, int32_t res_p,
                                const double* h_bpnts, const double* h_ppnts, const double* h_ramp, const double* h_sigma, int32_t skew,
                                int32_t mode, const double* d_grad_img, double* d_grad_pts, void* stream) {
    TLC_REQUIRE(n_dgms >= 0 && n_pts >= 0, "negative size");
    TLC_REQUIRE(mode == TLC_PI_GRAD_WEIGHT || mode == TLC_PI_GRAD_FULL, "mode is neither TLC_PI_GRAD_WEIGHT nor TLC_PI_GRAD_FULL");
    PigArgs A;
    PigGrid G;
    const int rc = pig_make_spec(__func__, res_b, res_p, h_bpnts, h_ppnts, h_ramp, h_sigma, skew, A.S, G);
    if (rc != TLC_OK) return rc;
    if (mode == TLC_PI_GRAD_FULL && A.S.nq != 0) {
        tlc_set_error("%s: TLC_PI_GRAD_FULL needs a separable sigma (cov == 0); the correlated kernel has the weight gradient only", __func__);
        return TLC_ERR_INVALID_ARG;
    }
    if (n_pts == 0) return TLC_OK;
    TLC_REQUIRE(n_dgms >= 1 && d_offs && d_pts && d_grad_img && d_grad_pts, "null pointer or points without a diagram");
    A.n_dgms = n_dgms; A.n_pts = n_pts;
    A.offs = (const long long*)d_offs; A.pts = d_pts; A.wts = nullptr;
    A.out = nullptr; A.partial = nullptr;
    const unsigned grid = (unsigned)(n_pts > 65536 ? 65536 : n_pts);
    hipLaunchKernelGGL(pig_vjp_kernel, dim3(grid), dim3(64), 0, (hipStream_t)stream, A, G, (int)(mode == TLC_PI_GRAD_FULL), d_grad_img,
                       d_grad_pts);
    TLC_HIP_CHECK(hipGetLastError());
    return TLC_OK;
}

// scratch_layouts.h -- the layout of every caller-sized scratch buffer of the link-prediction and PDGNN entry points, once.
// Host arithmetic only.  A struct is built from its entry's size arguments and holds the offset of every sub-array and `total`, in
// elements of the scratch's type (float32 or int32).  The exported tlc_*_work_floats / tlc_*_work_ints return `total`, the launch code
// takes its pointers from the same struct (work + L.pqa), and PdgnnWork (pdgnn_forward.hip) composes them: a size has one definition.
// These entries take a bare d_work without its size, so a `total` below what the launch writes is an out-of-bounds device write.
#pragma once
#include <stdint.h>

#include <algorithm>

inline int64_t tlc_up4(int64_t v) { return (v + 3) & ~(int64_t)3; }      // float counts whose successor stays 16-byte aligned

// tlc_gemm_tn_f32: the split-K partials [splits <= MAX_SPLITS][M][N]; one split writes d_C directly
struct TlcGemmTnScratch {
    static constexpr int MAX_SPLITS = 32;
    int64_t part = 0, total;
    TlcGemmTnScratch(int64_t M, int64_t N) : total(MAX_SPLITS * M * N) {}
};

// tlc_nc_linear_bwd_f32: its two tlc_gemm_tn_f32 products (dW [N,K], db [1,N]) one after the other in the same scratch
struct TlcNcLinearBwdScratch {
    int64_t tn = 0, total;
    TlcNcLinearBwdScratch(int64_t N, int64_t K) : total(std::max(TlcGemmTnScratch(N, K).total, TlcGemmTnScratch(1, N).total)) {}
};

// tlc_lp_decode_bwd_f32: d e_u per pair [n_pairs][ED] | the workgroups' weight-gradient partials [MAX_WG][NW]
struct TlcLpDecodeBwdScratch {
    static constexpr int ED = 16, NW = 1076, MAX_WG = 512;
    int64_t gpair = 0, part, total;
    explicit TlcLpDecodeBwdScratch(int64_t n_pairs) : part(n_pairs * ED), total(part + (int64_t)NW * MAX_WG) {}
};

// tlc_gcn2_encode_f32 / _csr_f32: x W1 [n][hidden] | conv1's output [n][hidden] | its projection [n][out_dim], each on a multiple of
// four floats.  The 12 floats behind them cover the two roundings (at most 3 floats each).
struct TlcGcn2EncodeScratch {
    int64_t t1 = 0, t2, t3, total;
    TlcGcn2EncodeScratch(int64_t n, int64_t hidden, int64_t out_dim)
        : t2(tlc_up4(n * hidden)), t3(t2 + tlc_up4(n * hidden)), total((2 * hidden + out_dim) * n + 12) {}
};

// tlc_csr_by_target (and the one-off builds of tlc_gcn_norm_csr / _t): the rows' counts [n], later the list of the long rows |
// [n] unused | the entries as they arrive [n_edges + n]
struct TlcCsrByTargetScratch {
    int64_t cnt = 0, raw, total;
    TlcCsrByTargetScratch(int64_t n, int64_t n_edges) : raw(2 * n), total(raw + n_edges + n) {}
};

// tlc_gat_tile_cut: the state words [HEAD] | the bitmap of the forbidden positions 0 .. n, [n / 32 + 2] words
struct TlcGatTileCutScratch {
    static constexpr int HEAD = 4;
    int64_t st = 0, bits = HEAD, words, total;
    explicit TlcGatTileCutScratch(int64_t n) : words(n / 32 + 2), total(bits + words) {}
    // room of d_tile_ptr: one tile start per multiple of tile_nodes - gap >= tile_nodes / 2, and the end
    static int64_t max_tiles(int64_t n, int64_t tile_nodes) { return 2 * n / tile_nodes + 3; }
};

// tlc_gat_layer_fwd.  On the f32 MFMA (c_out <= 32): x_l [n][C] | [P | Q | alpha | 0 0 0] [n][2C + 4] | Bt1 = Wl^T [c_in][C] |
// Bt2 [C][2C + 4]; with fused weights Wf [c_in][2C + 4] lies where x_l would (launch_gat takes that path only when it fits).
// c_in == 1 writes vec [2C + 1] only, c_out == 64 the node rows [n][3C + 1] only: both lie inside the x_l and pqa regions.
struct TlcGatLayerFwdScratch {
    int64_t xl = 0, vec = 0, rows = 0, pqa, bt1, bt2, total;
    TlcGatLayerFwdScratch(int64_t n, int64_t c_in, int64_t C)
        : pqa(xl + n * C), bt1(pqa + n * (2 * C + 4)), bt2(bt1 + c_in * C), total(bt2 + C * (2 * C + 4)) {}
};

// tlc_gat_layer_tiled_fwd.  Only the combined weights prep [c_in][2C + 4] (TlcGatPrepLayer of gat_internal.h) are written; `total`
// still counts the packed Wl^T, Bt2 and att / bias rows of the layer's earlier two-product form, because callers and
// tlc_pdgnn_forward_work_bytes size by it.
struct TlcGatLayerTiledFwdScratch {
    int64_t prep = 0, prep_floats, total;
    TlcGatLayerTiledFwdScratch(int64_t c_in, int64_t C)
        : prep_floats(c_in * (2 * C + 4)), total(c_in * C + C * (2 * C + 4) + prep_floats + 2 * C + 8) {}
};

// tlc_gat_layer_bwd: x_l [n][C] | pqa [n][2C + 4] | gP, gQ, gxl [n][C] each | Gz [n][2C] | tmp [2][C][C] | Bt1 [c_in][C], rounded
// up to four floats so that Bt2 [C][2C + 4] stays 16-byte aligned | gAlpha [n] (last: n floats would misalign what follows).
// `total` leaves the whole 4 floats of the contract for that rounding.
struct TlcGatLayerBwdScratch {
    int64_t xl = 0, pqa, gp, gq, gxl, gz, tmp, bt1, bt2, gal, total;
    TlcGatLayerBwdScratch(int64_t n, int64_t c_in, int64_t C)
        : pqa(xl + n * C), gp(pqa + n * (2 * C + 4)), gq(gp + n * C), gxl(gq + n * C), gz(gxl + n * C), tmp(gz + n * 2 * C),
          bt1(tmp + 2 * C * C), bt2(bt1 + tlc_up4(c_in * C)), gal(bt2 + C * (2 * C + 4)),
          total(gal + n + (c_in * C + 4 - tlc_up4(c_in * C))) {}
};

// tlc_edge_head_fwd (optional): the per-node projections U | V [n_nodes][2 hidden] | W5 packed for the GEMM [c][2 hidden].  The MFMA
// kernel (c = hidden = 32) and the per-edge kernel (d_work NULL) use none of it.
struct TlcEdgeHeadFwdScratch {
    int64_t uv = 0, bt, total;
    TlcEdgeHeadFwdScratch(int64_t n_nodes, int64_t c, int64_t hidden) : bt(n_nodes * 2 * hidden), total(bt + c * 2 * hidden) {}
};

// tlc_edge_head_bwd: [x_s || x_t] [n_edges][2c] | h [n_edges][hidden] | d pre [n_edges][hidden]
struct TlcEdgeHeadBwdScratch {
    int64_t cat = 0, hbuf, gpre, total;
    TlcEdgeHeadBwdScratch(int64_t n_edges, int64_t c, int64_t hidden)
        : hbuf(n_edges * 2 * c), gpre(hbuf + n_edges * hidden), total(gpre + n_edges * hidden) {}
};

// tlc_gnn_layer_bwd (gnn_layers.hip).  In floats, every array on a multiple of four: dZ [n][c_out] | G = dZ Wa [n][c_in] | H = dZ Ws
// [n][c_in] | the split-K partials of its tlc_gemm_tn_f32 products (gWa and gWs [c_out][c_in], gb [1][c_out]) one after the other in the
// same room.  tlc_gnn_layer_bwd_work_bytes returns `total` in BYTES (the entry takes work_bytes and checks it).
struct TlcGnnLayerBwdScratch {
    int64_t dz = 0, g, h, tn, total;
    TlcGnnLayerBwdScratch(int64_t n, int64_t c_in, int64_t c_out)
        : g(tlc_up4(n * c_out)), h(g + tlc_up4(n * c_in)), tn(h + tlc_up4(n * c_in)),
          total(tn + std::max(TlcGemmTnScratch(c_out, c_in).total, TlcGemmTnScratch(1, c_out).total)) {}
};

// tlc_msg_layer_fwd (msg_layers.hip).  In floats, every array on a multiple of four: x_l [n][C] | alpha [n] (EDGE_ATTN) | P, Q [n][C]
// each (NODE_FEAT; without it x_l is the message part).  tlc_msg_layer_fwd_work_bytes returns `total` in BYTES.
struct TlcMsgLayerFwdScratch {
    int64_t xl = 0, alpha, p, q, total;
    TlcMsgLayerFwdScratch(int64_t n, int64_t C, bool node_feat, bool edge_attn)
        : alpha(tlc_up4(n * C)), p(alpha + (edge_attn ? tlc_up4(n) : 0)), q(p + (node_feat ? tlc_up4(n * C) : 0)),
          total(q + (node_feat ? tlc_up4(n * C) : 0)) {}
};

// tlc_msg_layer_bwd (msg_layers.hip).  In floats, every array on a multiple of four: the forward's node rows again (`f`) | Gz [n][2C] |
// the arg-min and arg-max entries int[n][C] each | gx_l [n][C] | with EDGE_ATTN the row scalars (maximum, denominator, softmax-backward
// dot) [n][4], the target-side logit sums [n] and galpha [n] | with NODE_FEAT gP, gQ [n][C] each and the two halves of gWij [2][C][C] |
// the split-K partials of its tlc_gemm_tn_f32 products one after the other in the same room.  Nothing of the size of the entries.
// tlc_msg_layer_bwd_work_bytes returns `total` in BYTES.
struct TlcMsgLayerBwdScratch {
    TlcMsgLayerFwdScratch f;
    int64_t gz, emn, emx, gxl, stat, gtgt, gal, gp, gq, halves, tn, total;
    TlcMsgLayerBwdScratch(int64_t n, int64_t c_in, int64_t C, bool node_feat, bool edge_attn) : f(n, C, node_feat, edge_attn) {
        int64_t o = f.total;
        auto take = [&](int64_t count) { const int64_t at = o; o += tlc_up4(count); return at; };
        gz = take(n * 2 * C); emn = take(n * C); emx = take(n * C); gxl = take(n * C);
        stat = take(edge_attn ? 4 * n : 0); gtgt = take(edge_attn ? n : 0); gal = take(edge_attn ? n : 0);
        gp = take(node_feat ? n * C : 0); gq = take(node_feat ? n * C : 0); halves = take(node_feat ? 2 * C * C : 0);
        tn = o;
        total = o + std::max(std::max(TlcGemmTnScratch(C, C).total, TlcGemmTnScratch(C, c_in).total), TlcGemmTnScratch(1, 2 * C).total);
    }
};

// tlc_graph_components (gc_prep.hip).  In BYTES, every array on a multiple of 256: the control words [HEAD bytes] | the WAVE class's
// graph list int[B] | and, only when the batch can hold a WIDE graph (total_nodes > wave_nmax): per graph the class byte u8[B], the
// winner u64[B], the component count int[B], the first sorted key int[B]; per node the label u32[N], the component size int[N], the
// keep-flag scan u64[N + 1]; per raw edge the keys' two halves, each twice for the radix sort's ping-pong, u32[M] x 4, and the
// "distinct | kept" scan u64[M + 1]; the scans' chunk sums u64[chunks + 1]; the radix sort's hist and tot (ints: the caller passes
// rk_hist_ints(M) and RK_TOT_INTS of radix_passes.h, which is device code and stays out of this header).
struct TlcGraphComponentsScratch {
    static constexpr int64_t HEAD = 256, SCAN_CHUNK = 2048;
    static int64_t up256(int64_t v) { return (v + 255) & ~(int64_t)255; }
    bool wide;
    int64_t head = 0, list, cls, best, comps, first, parent, size, nscan, klo_a, klo_b, khi_a, khi_b, escan, sums, hist, tot, total;
    TlcGraphComponentsScratch(int64_t B, int64_t N, int64_t M, int64_t wave_nmax, int64_t hist_ints, int64_t tot_ints) : wide(N > wave_nmax) {
        int64_t o = HEAD;
        auto take = [&](int64_t count, int64_t size_of) { const int64_t at = o; o += up256((wide ? count : 0) * size_of); return at; };
        list = o; o += up256(B * 4);
        cls = take(B, 1); best = take(B, 8); comps = take(B, 4); first = take(B, 4);
        parent = take(N, 4); size = take(N, 4); nscan = take(N + 1, 8);
        klo_a = take(M, 4); klo_b = take(M, 4); khi_a = take(M, 4); khi_b = take(M, 4); escan = take(M + 1, 8);
        sums = take(std::max(N, M) / SCAN_CHUNK + 2, 8);
        hist = take(hist_ints, 4); tot = take(tot_ints, 4);
        total = o;
    }
};

// tlc_dist_filtration / tlc_dist_filtration_vjp (dist_filt.hip).  In BYTES, every array on a multiple of 256: the control words [HEAD
// bytes] | the three classes' graph lists int[3][B] | the repeated-edge hash u64[2 M] (graph g owns the slots 2 e0 .. 2 e1) | the
// owner graph of every edge int[M] (-1 unless its graph is of the whole-device class) | and, only when the batch can hold a graph of
// that class (N > wg_nmax or M > wg_mmax) or for the VJP (which keeps its per-node state in d_work in every class), per node PER_NODE
// bytes, per graph PER_GRAPH bytes.  The forward then needs at least one fallback slice u64[N]; a larger d_work holds up to
// MAX_GROUPS of them (`groups_in`).  `least` is what the entry requires and the *_work_bytes call returns.
struct TlcDistFiltScratch {
    static constexpr int64_t HEAD = 2048, MAX_GROUPS = 256;
    // forward: R u64[2] | q f64 | cnt u32[2] | nxt u32[2] | the fallback list int | the owner graph int  (9 arrays)
    // VJP:     T f64[2] | S f64[2] | depth, tree edge, child count, row start, children int[2] each        (14 arrays)
    // per graph: the largest distance u64 | the divisor u64 | the status int                               (3 arrays)
    static constexpr int64_t FWD_PER_NODE = 8 * 2 + 8 + 4 * 2 + 4 * 2 + 4 + 4, VJP_PER_NODE = 8 * 2 + 8 * 2 + 4 * 2 * 5, PER_GRAPH = 8 * 2 + 4;
    static constexpr int64_t NODE_ARRAYS = 16, GRAPH_ARRAYS = 3;      // room for each array's rounding up to 256 bytes
    static int64_t up256(int64_t v) { return (v + 255) & ~(int64_t)255; }
    bool wide;
    int64_t head = 0, lists, hash, egraph, node, graph, slices, slice_bytes, least;
    TlcDistFiltScratch(int64_t B, int64_t N, int64_t M, int64_t wg_nmax, int64_t wg_mmax, bool vjp)
        : wide(vjp || N > wg_nmax || M > wg_mmax) {
        int64_t o = HEAD;
        lists = o; o += up256(3 * B * 4);
        hash = o; o += up256(2 * M * 8);
        egraph = o; o += up256(M * 4);
        node = o; o += wide ? up256(N * (vjp ? VJP_PER_NODE : FWD_PER_NODE)) + 256 * NODE_ARRAYS : 0;
        graph = o; o += wide ? up256(B * PER_GRAPH) + 256 * GRAPH_ARRAYS : 0;
        slices = o;
        slice_bytes = (wide && !vjp) ? up256(N * 8) : 0;
        least = o + slice_bytes;
    }
    int64_t groups_in(int64_t work_bytes) const {
        if (!slice_bytes) return 0;
        return std::min<int64_t>(MAX_GROUPS, (work_bytes - slices) / slice_bytes);
    }
};

// tlc_segment_index (vic_grad.hip).  In BYTES, every array on a multiple of 256: the sort keys u32[n_items], twice for the radix sort's
// ping-pong | the second buffer of the positions u32[n_items] (the first is d_seg_pos itself) | the radix sort's hist and tot (ints: the
// caller passes rk_hist_ints(n_items) and RK_TOT_INTS of radix_passes.h, which is device code and stays out of this header).
struct TlcSegmentIndexScratch {
    static int64_t up256(int64_t v) { return (v + 255) & ~(int64_t)255; }
    int64_t key_a = 0, key_b, pos_b, hist, tot, total;
    TlcSegmentIndexScratch(int64_t n_items, int64_t hist_ints, int64_t tot_ints)
        : key_b(up256(n_items * 4)), pos_b(key_b + up256(n_items * 4)), hist(pos_b + up256(n_items * 4)), tot(hist + up256(hist_ints * 4)),
          total(tot + up256(tot_ints * 4)) {}
};

// tlc_segment_sum_f64 (vic_grad.hip).  In BYTES: the control words [HEAD bytes]: the lengths of the two lists, int each | the segments
// of the wavefront class int[n_keys] | those of the workgroup class int[n_keys].  The lists' order is the order of arrival and decides
// which wavefront sums a segment, never the order of a sum.
struct TlcSegmentSumScratch {
    static constexpr int64_t HEAD = 256;
    static int64_t up256(int64_t v) { return (v + 255) & ~(int64_t)255; }
    int64_t head = 0, wave_list = HEAD, wg_list, total;
    explicit TlcSegmentSumScratch(int64_t n_keys) : wg_list(wave_list + up256(n_keys * 4)), total(wg_list + up256(n_keys * 4)) {}
};

// tlc_pi_image: the partial images [slices][res_b * res_p] of the diagrams above SLICE points, one per slice of SLICE points (the second
// pass adds a pixel's slices ascending).  In float64 elements.  `least` holds the slices of the largest diagram, `total` those of
// MAX_GROUP such diagrams (the most one launch takes); diagrams of up to SLICE points need none.
struct TlcPiImageScratch {
    static constexpr int64_t SLICE = 1024, MAX_GROUP = 32;
    static int64_t slices_of(int64_t n_points) { return n_points > SLICE ? (n_points + SLICE - 1) / SLICE : 0; }
    int64_t partial = 0, least, total;
    TlcPiImageScratch(int64_t n_dgms, int64_t max_points, int64_t res_b, int64_t res_p)
        : least(slices_of(max_points) * res_b * res_p), total(std::min<int64_t>(n_dgms, MAX_GROUP) * least) {}
};

// tlc_landscape (landscape.hip): only the diagrams above SLICE points use it, one after the other.  In BYTES, carved by the shared carver
// (TlcCarver of tlc_common.h, handed in: this header stays host arithmetic): the control word | `slots` equal slots, each the K-lists
// of one slice of SLICE points -- the values f64[K * T] | the indices int[K * T].  Slot 0 is the running list (the K best per cell over
// the slices merged so far), slots 1 .. G the slices in flight.  `least` holds the running list and one slice, `total` as many slices
// as the largest diagram has (at most MAX_GROUP at once).
struct TlcLandscapeScratch {
    static constexpr int64_t SLICE = 4096, MAX_GROUP = 64;
    static int64_t slices_of(int64_t n_points) { return n_points > SLICE ? (n_points + SLICE - 1) / SLICE : 0; }
    int64_t ctl = 0, slots = 0, val = 0, idx = 0, slot_bytes = 0, group = 0, least = 0, total = 0;
    // in_flight: the slices of one launch; slots_for(g) is the size that runs g of them
    template <class Carver>
    static int64_t bytes_for(int64_t cells, int64_t in_flight, TlcLandscapeScratch* L) {
        Carver W;
        L->ctl = (int64_t)W.take(1, 4);
        L->slots = (int64_t)W.bytes() - 256;
        Carver S;
        L->val = (int64_t)S.take(cells, 8);
        L->idx = (int64_t)S.take(cells, 4);
        L->slot_bytes = (int64_t)S.bytes() - 256;
        return L->slots + (1 + in_flight) * L->slot_bytes + 256;      // (256: tlc_align256 of the caller's pointer)
    }
    template <class Carver>
    TlcLandscapeScratch(int64_t max_points, int64_t K, int64_t T, Carver) {
        const int64_t s = slices_of(max_points);
        if (!s) return;
        group = std::min(s, MAX_GROUP);
        least = bytes_for<Carver>(K * T, 1, this);
        total = bytes_for<Carver>(K * T, group, this);
    }
    int64_t groups_in(int64_t work_bytes) const {
        if (!slot_bytes) return 0;
        return std::min<int64_t>(MAX_GROUP, (work_bytes - 256 - slots) / slot_bytes - 1);
    }
};

// tlc_w2_large_matching (w2_large.hip).  In BYTES.  The workspace is `slots` equal slots and nothing else; a workgroup owns one slot for
// the whole launch.  A slot for problems of up to max_rows rows / columns, every array on a multiple of 256: the control words [HEAD
// bytes]: the counters int64[COUNTERS] (steps, augmentations, rows the start assigned, problems) | the row duals u f64[R] | the column
// duals v f64[R] | the columns' path lengths minv f64[R] | the column -> row map pcol int[R] | the path links way int[R] | the columns'
// used marks u8[R] | the rows' "the start assigned it" marks u8[R]: 34 bytes per row.  Rows above NMAX are refused and need no state.
struct TlcW2LargeScratch {
    static constexpr int64_t HEAD = 256, COUNTERS = 4, NMAX = 65536, PER_ROW = 8 * 3 + 4 * 2 + 1 * 2;
    static int64_t up256(int64_t v) { return (v + 255) & ~(int64_t)255; }
    int64_t rows, head = 0, u, v, minv, pcol, way, used, rdone, slot_bytes;
    explicit TlcW2LargeScratch(int64_t max_rows = 0) : rows(std::min(std::max<int64_t>(max_rows, 0), NMAX)) {
        int64_t o = HEAD;
        auto take = [&](int64_t size_of) { const int64_t at = o; o += up256(rows * size_of); return at; };
        u = take(8); v = take(8); minv = take(8); pcol = take(4); way = take(4); used = take(1); rdone = take(1);
        slot_bytes = o;
    }
    int64_t total(int64_t slots) const { return slots * slot_bytes; }
    int64_t slots_in(int64_t work_bytes) const { return work_bytes / slot_bytes; }
};

// tlc_hks_sparse_batch / _dt (hks_sparse.hip).  In BYTES, every array on a multiple of 256.  Once per call, from the declared node and
// edge counts of the selection (R = their nodes, E = 2 x their edges, the CSR entries): the descriptors [n_sel][DESC] | the graphs'
// states int[n_sel] | the sort keys u64[E], twice for the radix sort's ping-pong | its payload u8[E], twice | the columns int[E] | the
// row starts int[R + 1] | r_u f64[R] | the row of every chunk slot of the split rows int[slots] (a graph of e entries owns
// slots_of(e) of them) | the radix sort's hist and tot (ints: the caller passes rk_hist_ints(E) and RK_TOT_INTS of radix_passes.h,
// which is device code and stays out of this header).  Then the panels: a panel of a graph of n nodes and e entries holds, in float64,
// PANEL x (S [n] | s [n] | s' [n] | the split rows' partial sums [slots_of(e)] | the row blocks' partial sums [2][blocks_of(n)]).
// `least` holds the largest panel, `total` every panel of every graph.  (The three constexpr sizes are also what the setup kernel calls.)
struct TlcHksSparseScratch {
    static constexpr int64_t PANEL = 64, DESC = 64, LONG_ROW = 256, SAT = INT64_MAX / 4;
    static int64_t up256(int64_t v) { return (v + 255) & ~(int64_t)255; }
    static constexpr int64_t slots_of(int64_t entries) { return entries / PANEL + entries / LONG_ROW + 1; }
    static constexpr int64_t blocks_of(int64_t n) { return (n + PANEL - 1) / PANEL; }
    static constexpr int64_t panel_doubles(int64_t n, int64_t entries) { return PANEL * (3 * n + slots_of(entries) + 2 * blocks_of(n)); }
    static int64_t entries_of(const int64_t* sel_edges, int64_t n_sel) {
        int64_t e = 0;
        for (int64_t i = 0; i < n_sel; ++i) e += 2 * sel_edges[i];
        return e;
    }
    int64_t rows = 0, entries = 0, slots = 0, max_n = 0;
    int64_t descs = 0, state, key_a, key_b, lab_a, lab_b, col, rowptr, rinv, slotrow, hist, tot, panels, max_panel_bytes = 0, all_panel_bytes = 0,
            least, total;
    TlcHksSparseScratch(const int64_t* sel_nodes, const int64_t* sel_edges, int64_t n_sel, int64_t hist_ints, int64_t tot_ints) {
        for (int64_t i = 0; i < n_sel; ++i) {
            const int64_t n = sel_nodes[i], e = 2 * sel_edges[i], pb = panel_doubles(n, e) * 8;
            rows += n; entries += e; slots += slots_of(e);
            max_n = std::max(max_n, n);
            if (n) max_panel_bytes = std::max(max_panel_bytes, pb);
            const int64_t nb = blocks_of(n);                 // (saturating: 2^25 panels of 3e12 bytes do not fit an int64)
            all_panel_bytes = std::min(SAT, all_panel_bytes + (nb && pb > SAT / nb ? SAT : nb * pb));
        }
        int64_t o = up256(n_sel * DESC);
        auto take = [&](int64_t count, int64_t size_of) { const int64_t at = o; o += up256(count * size_of); return at; };
        state = take(n_sel, 4);
        key_a = take(entries, 8); key_b = take(entries, 8); lab_a = take(entries, 1); lab_b = take(entries, 1); col = take(entries, 4);
        rowptr = take(rows + 1, 4); rinv = take(rows, 8); slotrow = take(slots, 4);
        hist = take(hist_ints, 4); tot = take(tot_ints, 4);
        panels = o;
        least = o + max_panel_bytes;
        total = o + all_panel_bytes;
    }
};

// tlc_dgm_gram / tlc_dgm_gram_vjp (dgm_gram.hip).  In BYTES, carved by the shared carver (handed in, as for the landscape).  A diagram of
// n points is cut into slices_of(n) slices of SLICE points as the first argument and into groups_of(n) groups of GROUP points as the
// second; a unit is one (slice, group) of one diagram pair.  The unit-prefix arrays int64[nx + 1] | int64[ny + 1], contiguous (uploaded by the entry;
// the VJP keeps the 64-point chunk prefix of X in the first) exist when a declared size leaves the one-unit case (max_nx_points > CHUNK
// or max_ny_points > GROUP); the unit partials f64[slots] behind them when a pair can have more than one unit (max_nx_points > SLICE
// or max_ny_points > GROUP).  `least` holds the partials of the rows of one X diagram (ALL: against every Y diagram; PAIRED: its one
// pair), `total` those of every diagram, at most FULL_CAP bytes of them (but never below `least`).  Saturating: -1 sizes are the entry's.
struct TlcDgmGramScratch {
    static constexpr int64_t SLICE = 1024, GROUP = 1024, CHUNK = 64, SAT = INT64_MAX / 64, FULL_CAP = (int64_t)1 << 30;
    static int64_t slices_of(int64_t n) { return n > SLICE ? (n + SLICE - 1) / SLICE : 1; }
    static int64_t groups_of(int64_t n) { return n > GROUP ? (n + GROUP - 1) / GROUP : 1; }
    static int64_t chunks_of(int64_t n) { return (n + CHUNK - 1) / CHUNK; }
    static int64_t sat_mul(int64_t a, int64_t b) { return a && b > SAT / a ? SAT : std::min(SAT, a * b); }
    int64_t xpre = 0, ypre = 0, partial = 0, head = 0, row_slots = 0, least = 0, total = 0;
    bool prefixes = false, wide = false;
    template <class Carver>
    TlcDgmGramScratch(int64_t nx, int64_t ny, int64_t max_nx_points, int64_t max_ny_points, bool paired, Carver) {
        prefixes = max_nx_points > CHUNK || max_ny_points > GROUP;
        wide = max_nx_points > SLICE || max_ny_points > GROUP;
        if (!prefixes || nx < 1 || ny < 1) { prefixes = wide = false; return; }
        Carver W;
        xpre = (int64_t)W.take(nx + ny + 1, 8);                 // (one block of nx + 1 and ny + 1 entries: one upload)
        ypre = xpre + (nx + 1) * 8;
        partial = (int64_t)W.bytes() - 256;
        head = (int64_t)W.bytes();                               // (with the 256 of tlc_align256)
        least = total = head;
        if (!wide) return;
        const int64_t per_pair = sat_mul(slices_of(max_nx_points), groups_of(max_ny_points));
        row_slots = paired ? per_pair : sat_mul(per_pair, ny);
        const int64_t all = sat_mul(row_slots, nx);
        least = std::min(SAT, head + sat_mul(row_slots, 8));
        total = std::max(least, head + std::min(sat_mul(all, 8), FULL_CAP));
    }
    int64_t slots_in(int64_t work_bytes) const { return wide ? (work_bytes - head) / 8 : 0; }
};

/*
 * tlcgnn.h -- C ABI of libtlcgnn_hip.so: the MI355X (gfx950) implementation of TLC-GNN / PDGNN's
 * per-edge topological-feature hot path (vicinity subgraph -> extended persistence diagram ->
 * persistence image -> link-prediction forward).
 *
 * The reference (pkuyzy/TLC-GNN) has no FFI layer of its own: its boundary is a set of Python call
 * signatures.  Each entry point below names the reference interface (file:line under /root/reference)
 * that it replaces; INTEGRATION.md shows the ctypes stub a maintainer of the reference would add.
 *
 * Conventions
 *   - plain pointers and sizes only; no torch / HIP types in signatures (`stream` is a hipStream_t
 *     passed as void*, NULL = the default stream);
 *   - pointers prefixed d_ are DEVICE pointers, h_ are HOST pointers;
 *   - the caller allocates every buffer; the library keeps nothing beyond the call except the
 *     `tlc_graph` handle (which owns a device copy of the CSR and the kernels' scratch);
 *   - every call is stream-ordered: its work is ordered after what `stream` holds and later work on `stream` sees its
 *     outputs.  The calls RETURN before that work is done, with one documented exception: tlc_pd_pi_batch,
 *     tlc_pd_pi_batch_async and tlc_vicinity_filtration hold the calling thread, once per chunk of 2^20 pairs, until a
 *     chunk's extraction and size scan have run on the device (~0.3 ms for 37 676 pairs; the sizes come back through
 *     mapped host memory and size the tier launches that follow) -- nothing is synchronised and `stream` is not drained,
 *     but the call is not free of host waiting.  A pipelined chunk (tlc_pd_pi_batch_async, or a list of several chunks) waits
 *     for the PREVIOUS chunk's sizes, after it has submitted its own first half: the tier launches of a chunk go in one call
 *     later, those of the last chunk with the join.  The statistics / timing / sizes getters synchronise `stream`.  Outputs are fully
 *     overwritten (zero rows are written explicitly, mirroring `pi_sg = np.zeros(...)`,
 *     sg2dgm/riccidist2dgm.py:363);
 *   - a tlc_graph handle owns mutable scratch: calls on the SAME handle must not overlap (use one handle per
 *     host thread / per concurrent stream); different handles are independent;
 *   - return value: TLC_OK or a TLC_ERR_* code for API misuse / runtime failure.  Per-pair conditions
 *     that the reference swallows into a zero row (`except BaseException`, riccidist2dgm.py:352-357)
 *     are reported in the per-pair status byte, never as a return code.
 */
#ifndef TLCGNN_H
#define TLCGNN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- return codes ------------------------------------------------------------------------------ */
#define TLC_OK                 0
#define TLC_ERR_INVALID_ARG    1
#define TLC_ERR_HIP            2   /* a HIP runtime call failed; see tlc_last_error() */
#define TLC_ERR_NO_DEVICE      3
#define TLC_ERR_UNSUPPORTED    4   /* e.g. graph too large for the LDS-resident vicinity bitmaps */
#define TLC_ERR_OUT_OF_MEMORY  5

/* ---- per-pair status byte (the reference's swallowed exception classes) ---------- */
#define TLC_ST_OK              0   /* row computed (may still be all zero: d(u,v) > hop)            */
#define TLC_ST_MISSING_NODE    1   /* KeyError: endpoint has no edge (graph is built from edges)    */
#define TLC_ST_DISCONNECTED    2   /* AssertionError: vicinity empty or not connected (:318)        */
#define TLC_ST_ZERO_RANGE      3   /* ZeroDivisionError: all filtration values 0 (:54)              */
#define TLC_ST_NO_TREE_EDGE    4   /* IndexError: single-node vicinity (accelerated_PD.py:122)      */
#define TLC_ST_TOO_LARGE       5   /* not a reference class: the vicinity has more than 65 535 nodes or
                                      2^24-2 edges (packed local ids / edge ranks); zero row, never silent.
                                      tlc_hks_batch: the graph has more than TLC_HKS_NMAX nodes; its slice of
                                      the output is left untouched */
#define TLC_ST_NOT_CONVERGED   6   /* tlc_hks_batch: the Jacobi sweeps did not converge within their bound; slice untouched */
#define TLC_ST_BAD_INPUT       7   /* tlc_hks_batch, tlc_struct_batch: offsets out of order / beyond the totals, an edge with an id outside
                                      0 .. n-1, a self loop (nothing of it is dereferenced) or an unordered pair listed
                                      more than once, in either orientation; slice untouched.  tlc_graph_components: the
                                      offsets and the ids only (loops and repeats are its input) */

/* ---- variant flags (one kernel family serves the TLC-GNN and the PDGNN forks) ---- */
#define TLC_KEEP_ZERO_PERS   0x01u /* Knowledge_Distillation/accelerated_PD.py:68-69,108-109,169-170 */
#define TLC_INCLUDE_ROOTS    0x02u /* Knowledge_Distillation/data_utils_LP.py:111                    */
#define TLC_NORM_EPS         0x04u /* divide by (max + 1e-10): data_utils_LP.py:64                   */
#define TLC_PI_ORD0_EXT1     0x08u /* image over Ord0 ++ Ext1 only: data_utils_GC.py:155-163         */
#define TLC_NO_EXT1          0x10u /* extended_flag=False: riccidist2dgm.py:323-326                  */
#define TLC_UNREACHABLE_100  0x20u /* no connectivity assert; an unreachable root costs the sentinel 100:
                                      Knowledge_Distillation/data_utils_LP.py:41-49 (filtration only)  */
/* which of the three node values of filtration.build_fv (riccidist2dgm.py:47-49) is the filtration: 'sum' = d1 + d2 (the
 * pipeline's choice, loaddatas.py:101; flag value 0), 'min', 'max' (get_pimg_for_all_edges' own default is 'min', :362) --
 * 'min' and 'max' are both divided by max_S max(d1, d2), 'sum' by max_S (d1 + d2) (:51-56) -- or the distance to the FIRST
 * root alone, the single-root filtration of the node-centred PDGNN vicinities (Knowledge_Distillation/data_utils_NC.py:27-50;
 * hand the node in as the pair (u, u): ball(u) & ball(u) is its ball) */
#define TLC_DESC_MIN         0x40u
#define TLC_DESC_MAX         0x80u
#define TLC_DESC_ROOT1       0xC0u
#define TLC_DESC_MASK        0xC0u
/* norm=False of build_fv (:50): raw distances, no division, no ZeroDivisionError.  tlc_vicinity_filtration only: the image
 * stage of tlc_pd_pi_batch assumes values in [0, 1] (TLC_ERR_UNSUPPORTED there); unnormalised images are
 * tlc_vicinity_filtration -> tlc_pd_from_filtration -> tlc_pi_raster (what the sg2dgm_accelerate drop-in does) */
#define TLC_NO_NORM          0x100u

typedef struct tlc_graph tlc_graph;   /* opaque: device CSR + scratch, bound to one device */

/* ---- library ------------------------------------------------------------------------------------ */
const char* tlc_version(void);
const char* tlc_last_error(void);          /* thread-local text of the last TLC_ERR_* */
int  tlc_device_count(void);

/* ---- P1: graph2pi.__init__ (sg2dgm/riccidist2dgm.py:216-226) ------------------------------------
 * Symmetric CSR of the weighted graph: node ids 0..n_nodes-1, h_w[e] = kappa_e + 1 (must be > 0),
 * both directions present.  Nodes with an empty row are "missing" (TLC_ST_MISSING_NODE), exactly as
 * the reference's graph is built from edges only (loaddatas.py:88-92).  Synchronous (uploads). */
int tlc_graph_create(int32_t n_nodes, const int32_t* h_rowptr, const int32_t* h_col, const double* h_w,
                     int device, tlc_graph** out);
int tlc_graph_destroy(tlc_graph* g);

/* ---- P2-P9: graph2pi.get_pimg_for_all_edges (sg2dgm/riccidist2dgm.py:348-370) ------------------
 * For every pair (u,v): S = ball_hop(u) & ball_hop(v) on the unweighted graph (:311-316), induced
 * subgraph, filtration f = (d(x,u)+d(x,v)) / max with node-sourced weighted shortest paths (:20-61),
 * perturbed keys + two union-find passes + spanning-tree cycle swap (accelerated_PD.py:6-178),
 * res x res Gaussian persistence image (PersistenceImager.pyx:352-388).
 *   d_pairs      int32[n_pairs,2]
 *   d_out_pi     float64[n_pairs, res*res], row-major [birth_bin*res + pers_bin]
 *   d_out_status uint8[n_pairs] (may be NULL)
 * hop >= 1; res in 1..8. */
int tlc_pd_pi_batch(tlc_graph* g, const int32_t* d_pairs, int64_t n_pairs, int hop, uint32_t flags,
                    int res, double* d_out_pi, uint8_t* d_out_status, void* stream);

/* Same pipeline, stopping after the filtration (used by tests and by the PDGNN 'filtration' mode,
 * Knowledge_Distillation/data_utils_LP.py:105-200 mode='filtration'):
 *   d_node_offs  int64[n_pairs+1]  (caller-provided capacity layout: slot i holds up to
 *                                   node_offs[i+1]-node_offs[i] nodes)
 *   d_out_ids    int32[cap]  ascending node ids of S;  d_out_f float64[cap];  d_out_n int32[n_pairs]
 * A vicinity larger than its slot sets d_out_n[i] = -(size).
 * Optional (all three or none): d_edge_offs int64[n_pairs+1] capacity layout, d_out_edges int32[cap,2] = the induced
 * undirected edges as LOCAL ids (position in the pair's id list, lower id first), d_out_m int32[n_pairs] (-(m) if the slot is
 * too small): the (filtration_val, edge_index) pair that data_utils_LP.compute_persistence_image(mode='filtration') returns. */
int tlc_vicinity_filtration(tlc_graph* g, const int32_t* d_pairs, int64_t n_pairs, int hop, uint32_t flags,
                            const int64_t* d_node_offs, int32_t* d_out_ids, double* d_out_f,
                            int32_t* d_out_n, uint8_t* d_out_status,
                            const int64_t* d_edge_offs, int32_t* d_out_edges, int32_t* d_out_m, void* stream);

/* The same batch WITHOUT the final join -- for a caller that submits batch after batch (the reference's sweep over its pair
 * lists, sg2dgm/riccidist2dgm.py:362-370 over loaddatas.py:44-53) and wants them to overlap: the batch is ordered after what
 * `stream` holds at the time of the call (its inputs may be produced there), runs on streams of the handle, and `stream` does
 * NOT wait for it.  The outputs are complete for work that follows a tlc_pd_pi_batch_join() on its stream -- and only then:
 * the second half of the most recent batch (the launches sized by its vicinity counts) is submitted by the next
 * tlc_pd_pi_batch_async, by the join, or by any other call on the handle, whichever comes first.  A handle keeps three
 * batches in flight; submitting a fourth waits ON THE HOST for the first.  tlc_pd_pi_batch == async + join.
 * Buffers (pairs, out_pi, out_status) of a batch in flight must stay valid and must not be written until joined. */
int tlc_pd_pi_batch_async(tlc_graph* g, const int32_t* d_pairs, int64_t n_pairs, int hop, uint32_t flags,
                          int res, double* d_out_pi, uint8_t* d_out_status, void* stream);
int tlc_pd_pi_batch_join(tlc_graph* g, void* stream);

/* Counters of the last tlc_pd_pi_batch on this handle (synchronises the stream):
 * h_out[0..3] = pairs in tier small / medium / large / huge, [4] = induced directed entries (arena size),
 * [5] = sources that needed the exact tie fallback, [6] = chunks, [7] = pairs in tier mid (between small and medium),
 * [8] = pairs of tier small that took the lane-per-subgraph kernel (at most 16 nodes / 24 edges), [9] = pairs of tier medium with many Pos edges (launched first).  h_out: 10 entries. */
int tlc_pd_pi_batch_stats(tlc_graph* g, int64_t* h_out, void* stream);

/* Measurement helpers used by bench.py (no reference counterpart: the reference only prints time.time() deltas,
 * riccidist2dgm.py:349-350).  set_timing(1) makes every later tlc_pd_pi_batch bracket each of its kernels with HIP
 * events on the stream that kernel runs on (set_timing(1 << (k+1)), or a sum of such bits: only the kernels of slots k -- the
 * event records themselves cost time, 48 us of the 1.06 ms PubMed batch for all eight); timings() returns the last chunk's
 * durations in ms:
 * h_ms[0..7] = COUNT, scan+binning, FILL, PD tier SMALL, MEDIUM, LARGE, HUGE, MID (-1 = not launched).  Synchronises.
 * sizes(): per pair of the last chunk, |S| and the induced directed entry count.
 * algorithmic_bytes(): SURVEY.md 8(d) per-pair byte model, evaluated on the HOST CSR (pure accounting). */
int tlc_pd_pi_batch_set_timing(tlc_graph* g, int enable);
int tlc_pd_pi_batch_timings(tlc_graph* g, double* h_ms, void* stream);
/* The same for a caller that enqueues chunk after chunk WITHOUT synchronising (the shape of the reference's sweep over
 * total_edges, riccidist2dgm.py:362-370): the events of the last 64 chunks are kept; history() synchronises once, afterwards,
 * and returns timing slot `slot` (index into h_ms above) of the most recent min(cap, 64, chunks so far) chunks, oldest
 * first, -1 where the kernel did not run; *n_out = entries written. */
int tlc_pd_pi_batch_timing_history(tlc_graph* g, int slot, double* h_ms, int32_t cap, int32_t* n_out, void* stream);
int tlc_pd_pi_batch_sizes(tlc_graph* g, int32_t* h_n, int32_t* h_m2, int64_t cap, void* stream);
int tlc_pd_pi_algorithmic_bytes(int32_t n_nodes, const int32_t* h_rowptr, const int32_t* h_col, const int32_t* h_pairs,
                                int64_t n_pairs, int hop, int res, double* h_out_bytes);

/* Diagnostics (development tools and the tests of the divide-and-conquer cycle swap; no reference counterpart).
 * dc_stats(): of the chunks since the last tlc_pd_pi_batch call began, h_out[0] = subgraphs whose cycle swap ran as the divide
 * and conquer of tlc_pd_dc_kernel, h_out[1] = subgraphs it gave back to the serial walk (ranks that are no minimum-spanning-tree
 * order).  Synchronises the stream.
 * phase_profile(): per-phase cycle counters of the tier kernels in a library built with `make PHASE_DEBUG=1` (all zero
 * otherwise): rows of 32 u64, one per tier and one for the early pass; at most cap_u64 values are written to h_out (may be
 * null), *n_rows (may be null) = rows kept.  enable != 0 starts counting, 0 stops and frees the counters.
 * set_option(): the seventeen switches of one handle, each exercised by a test that checks that results do not depend on it
 * (tests/test_gpu_extract.py, tests/test_gpu_tiers.py, tests/test_gpu_pd_parity.py, tests/test_gpu_pipelined.py); 1 = on is the default of the first eight:
 *   "extract"      ball-list extraction of the vicinities (any hop since round 5; 0: the breadth-first kernels; TLC_EXTRACT=0 at creation)
 *   "heavy"        its hub-row skipping (TLC_HEAVY=0)
 *   "tiny"         lane-per-subgraph kernel for vicinities of at most 16 nodes / 24 edges (TLC_TINY=0)
 *   "ball_edges"   vicinities of pairs whose smaller ball has <= 128 nodes from that ball's subgraph list (TLC_BALL_EDGES=0)
 *   "fast_split"   ... in a launch of their own beside the classification and the early pass (TLC_FAST_SPLIT=0)
 *   "ball_bits"    ... which tests membership in the larger ball against per-node ball bitmaps (N^2 / 8 bytes, built up to 1 GiB)
 *                  instead of marking that ball in an LDS bitmap per pair (round 6; TLC_BALL_BITS=0)
 *   "plain_kernels" the tier / swap kernel instances that have a plain image batch's parameters (flags 0, resolution 5, no filtration
 *                  outputs) as compile-time constants (round 6; 0: the general instances; TLC_PLAIN_KERNELS=0)
 *   "dc_inplace"   the LARGE tier's divide and conquer by the tier kernel's own workgroup (0: tlc_pd_dc_kernel; TLC_DC_INPLACE=0)
 *   "dc_force_fail" every divide-and-conquer solve given back to the serial walk (test hook)
 *   "spec_cap"     slots reserved for the speculative tier launches (test hook: beyond them the second-launch / in-kernel paths)
 *   "x_arena"      arena entries per extraction workgroup and of the bump area (test hook: reach the overflow paths; 0 = defaults)
 *   "tier_mask"    bit t: tier t's kernels are launched at all (cost tables under profiles/)
 *   "n_ws"         workspaces taken in turn by pipelined chunks (2..4, default 3)
 *   "timing_every" kernel events on every n-th chunk only
 *   "mh_front_pos" pipelined plain chunks: compact MEDIUM vicinities with at least this many Pos edges go in front of their list
 *                  (default 64; 0: no front list)
 *   "main_beside_early" pipelined chunks: the general extraction waits for the classification only and runs beside the early pass
 *                  (default 1; 0: it waits for the whole early pass, as a chunk on its own does)
 *   "poison"       test hook: each chunk fills its workspace's float64 payload scratch with 7.25 before its first kernel (default 0)
 * An unknown name is TLC_ERR_INVALID_ARG. */
int tlc_debug_set_option(tlc_graph* g, const char* name, int value);
int tlc_debug_dc_stats(tlc_graph* g, long long* h_out, void* stream);
/* Counters for tests, h_out[0 .. min(n, 12)): [0] front-list vicinities (option mh_front_pos) of the last tlc_pd_pi_batch call; since the
 * handle was created: [1] front-list vicinities, [2] pipelined chunks, [3] chunks with the early pass, [4] speculative list positions
 * beyond their reserved slots, [5] poisoned chunks, [6] bytes poisoned; [7..9] bytes the last poisoned chunk filled in the arena's,
 * the early arena's and the SMALL slots' weights; [10] second halves submitted behind the next chunk's first half (not by a join or a
 * drain), [11] the most workspaces with a chunk not yet waited for on the host at a chunk's submission.  Submits a deferred second
 * half and synchronises `stream`. */
int tlc_debug_chunk_counters(tlc_graph* g, long long* h_out, int32_t n, void* stream);
/* The tier lists of the last tlc_pd_pi_batch call as the device cut them, h_out[8]: small, medium (the compact kernel configuration,
 * <= 384 nodes / 512 edges), large, huge, mid, tiny, medium with many Pos edges, medium beyond the compact configuration (<= 512 /
 * 1024).  tlc_pd_pi_batch_stats reports tiny with small and the three medium lists as one. */
int tlc_debug_tier_counts(tlc_graph* g, long long* h_out, void* stream);
int tlc_debug_phase_profile(tlc_graph* g, int enable, unsigned long long* h_out, int64_t cap_u64, int32_t* n_rows);
/* (builds with PAIR_TIMES=1 only: wall-clock stamps of the extraction, h_out[n_pairs][16] ticks of 10 ns; zeros otherwise) */
int tlc_debug_pair_times(tlc_graph* g, unsigned long long* h_out, int64_t n_pairs);

/* ---- P6-P8: perturb_filter_function / Union_find / Accelerate_PD ---------------------------------
 * (sg2dgm/accelerated_PD.py:6-178 and the Knowledge_Distillation fork, selected by TLC_KEEP_ZERO_PERS)
 * Batch of n_graphs independent graphs with caller-supplied filtration values.
 *   d_node_offs int64[n_graphs+1], d_edge_offs int64[n_graphs+1]
 *   d_edges     int32[sum m, 2] local node ids;  d_f float64[sum n]
 * Outputs (slot of graph g starts at node_offs[g] resp. edge_offs[g]):
 *   d_pd_up    float64[sum n, 2]  Ord0 points   (ascending pass, :46-68)
 *   d_pd_down  float64[sum n, 2]  Rel1 points   (descending pass, :83-109)
 *   d_pd_one   float64[sum m, 2]  Ext1 points   (:115-178)
 *   d_ext0     float64[n_graphs, 2]  [min f, max f] (:110)
 *   d_counts   int32[n_graphs, 4] = {#up, #down, #one, #connected components}; all four -1 for a graph with more than
 *              65 535 nodes or 2^24-2 edges (not computed)
 *   d_edge_rank int32[sum m] (may be NULL): >= 0: position among the Pos edges, in descending-pass
 *               order (:109); < 0: -(position among the Neg edges)-1 (:99). */
int tlc_pd_from_filtration(int32_t n_graphs, const int64_t* d_node_offs, const int64_t* d_edge_offs,
                           const int32_t* d_edges, const double* d_f, uint32_t flags,
                           double* d_pd_up, double* d_pd_down, double* d_pd_one, double* d_ext0,
                           int32_t* d_counts, int32_t* d_edge_rank, void* stream);

/* ---- the same diagrams for a few BIG graphs, on the whole device (csrc/pd_wide.hip) --------------------------
 * The packed layout, TLC_KEEP_ZERO_PERS / TLC_NO_EXT1 and the output slots of tlc_pd_from_filtration; 32-bit ids, no node cap.
 * h_sel int64[n_sel] (HOST): the graphs to compute, in any order; they run one after the other on the stream.  The rows and slots
 * of every other graph are not touched.  d_work: the caller's, at least tlc_pd_wide_work_bytes of the largest selected graph
 * (host arithmetic, no device needed; 0 for an empty selection); a smaller one is TLC_ERR_INVALID_ARG and the message names the
 * bytes needed.  The call reads the selected graphs' offsets back once before it launches anything.
 * Size limit: n >= 0 nodes, m >= 0 edges, n + m <= TLC_PD_WIDE_MAX_ITEMS = 2^27 -- the level loop numbers the copies of up to
 * 4 m + 4 supernodes in a doubled id space with 32-bit ints, and the sort's positions and payloads are 32-bit.  Beyond it:
 * TLC_ERR_UNSUPPORTED, nothing launched.  Filtration values of nodes that have an edge lie inside [-1, 101], the domain of the
 * reference's key perturbation: there every node enters the filtration before its edges, and the edges are sorted without the nodes.
 * Per-graph refusal (the convention of tlc_struct_batch): offsets out of order or negative, an id outside 0 .. n-1, a self loop, or
 * an edge with an end whose value is outside [-1, 101] or not a number (the reference's merged order is not computed there)
 * make that graph's d_counts row TLC_PD_WIDE_BAD_INPUT_ROW in all four entries (TLC_ST_BAD_INPUT; its slots are left untouched, no
 * other graph is affected).
 * Among equal descending keys the edge with the higher ascending rank comes first (the contract of fix_desc_ties, for runs of any
 * length): this may make another one of several equal edges Pos than the reference's stable sort does; the diagrams are the same
 * multisets.  d_edge_rank (may be NULL) holds the positions in THIS order: a valid permutation, under ties not the reference's.
 * Points are written by prefix-sum compaction: two runs give the same bits.
 * TLC_PD_WIDE_FORCE_FALLBACK (debug; tlc_pd_from_filtration refuses it): skip the divide and conquer and take the exact serial
 * cycle swap that otherwise runs only when the end checks fail.  The fallback walks the Pos edges in this tier's order and compares
 * fp64 ascending keys, first maximum of the loop, as the reference does.
 * h_stats int64[TLC_PD_WIDE_N_STATS] (HOST, may be NULL; costs one synchronisation), for the last selected graph: divide-and-conquer
 * levels, Boruvka rounds in total, kernel launches, 1 if the fallback ran, the graph's TLC_ST_* status. */
#define TLC_PD_WIDE_MAX_ITEMS       (1ll << 27)
#define TLC_PD_WIDE_FORCE_FALLBACK  0x40000000u
#define TLC_PD_WIDE_BAD_INPUT_ROW   (-2)
#define TLC_PD_WIDE_N_STATS         5
#define TLC_PD_WIDE_BLOCK           256    /* threads per workgroup of the grid-stride kernels */
#define TLC_PD_WIDE_SORT_TILE       4096   /* edges per workgroup of a radix pass */
#define TLC_PD_WIDE_SCAN_CHUNK      2048   /* flags per workgroup of a prefix sum */
#define TLC_PD_WIDE_LDS_NODES       40000  /* up to this many nodes the union-find array of an elder-rule pass lives in LDS */
int tlc_pd_wide_work_bytes(const int64_t* h_sel_nodes, const int64_t* h_sel_edges, int64_t n_sel, int64_t* bytes);
int tlc_pd_wide(int64_t n_graphs, const int64_t* d_node_offs, const int64_t* d_edge_offs, const int32_t* d_edges,
                const double* d_f, uint32_t flags, const int64_t* h_sel, int64_t n_sel,
                double* d_pd_up, double* d_pd_down, double* d_pd_one, double* d_ext0, int32_t* d_counts,
                int32_t* d_edge_rank, void* d_work, int64_t work_bytes, int64_t* h_stats, void* stream);

/* ---- d diagram / d filtration of the two entries above (csrc/pd_grad.hip) --------------------------------------
 * Every coordinate of every point those entries write is a copy of one f[v]: the Jacobian is a 0/1 selection matrix.  They return
 * the values only; tlc_pd_point_vertices recovers the vertices from them, after the forward, by one rule:
 *     the vertex of a coordinate c of graph g is the LOWEST local id v in 0 .. n_g-1 with f[node_offs[g] + v] == c
 * (IEEE ==: -0.0 matches +0.0, a NaN matches nothing).  Where the values of a graph are pairwise distinct this is the critical vertex
 * of the pairing.  Under ties the map from f to the diagram is not differentiable, and the rule is a fixed CONVENTION: the same in
 * every size class and for both forward entries, and independent of tlc_pd_wide's own Pos / Neg choice among equal keys.
 * Both entries take the packed layout and the slots of tlc_pd_from_filtration and its d_counts rows as the source of truth: rows
 * 0 .. counts[g,k)-1 of a slot are points, the rows behind them are not.
 *
 * tlc_pd_point_vertices: d_vert_up / d_vert_down int32[sum n, 2], d_vert_one int32[sum m, 2], d_vert_ext0 int32[n_graphs, 2] (the
 * vertices of [min f, max f]): local ids in the point rows of every computed graph, -1 in the slot's rows behind the points.
 * d_status uint8[n_graphs]: TLC_ST_OK; TLC_ST_TOO_LARGE for a d_counts row of -1 (or n + m above TLC_PD_WIDE_MAX_ITEMS), rows
 * untouched; TLC_ST_BAD_INPUT for a row of TLC_PD_WIDE_BAD_INPUT_ROW, counts that do not fit the slot, offsets out of order or
 * negative (rows untouched), or a coordinate that no vertex of the graph holds -- a diagram of another f, a NaN -- whose entry is
 * then -1.  No other graph is affected.  A graph without nodes: TLC_ST_OK, nothing written.
 *
 * tlc_pd_filtration_grad: d_grad_f float64[sum n].  Every entry of a graph whose d_status is TLC_ST_OK is written, zeros included;
 * the slices of the other graphs are left untouched.  grad_f[v] = the sum of the gradients d_g_* (each float64 in the layout of its
 * slot; NULL = zeros) of the coordinates whose vertex is v, in fp64 from +0.0, left to right in this order: up rows ascending (birth,
 * then death of a row), then down rows, then one rows, then ext0 (birth, death).  Gradients in rows behind the points are ignored.
 * No floating-point atomics: the bits of a graph's slice depend neither on the run, nor on the batch around it, nor on d_work.
 *
 * Size classes by node count, cut on the device: up to TLC_PD_VERT_WAVE_NMAX one wavefront per graph; up to TLC_PD_VERT_LDS_NMAX
 * (= the forward's TLC_L_NMAX) one workgroup per graph; above, the whole device, one graph after the other, in d_work.
 * d_work: tlc_pd_grad_work_bytes(largest node count, largest edge count of the batch) bytes -- host arithmetic, no device; 0 (and
 * d_work may be NULL) when no graph exceeds TLC_PD_VERT_LDS_NMAX nodes.  Both entries read the batch's offsets back once and
 * synchronise the stream before they launch anything.
 * TLC_ERR_INVALID_ARG, nothing launched: null required pointers, n_graphs < 0, work_bytes < 0, or a d_work too small for a graph of
 * the batch -- the message names the bytes held and the bytes needed.  n_graphs == 0: TLC_OK, nothing read. */
#define TLC_PD_VERT_WAVE_NMAX  64
#define TLC_PD_VERT_LDS_NMAX   2048
int tlc_pd_grad_work_bytes(int64_t max_nodes, int64_t max_edges, int64_t* bytes);
int tlc_pd_point_vertices(int64_t n_graphs, const int64_t* d_node_offs, const int64_t* d_edge_offs, const double* d_f,
                          const double* d_pd_up, const double* d_pd_down, const double* d_pd_one, const double* d_ext0,
                          const int32_t* d_counts, int32_t* d_vert_up, int32_t* d_vert_down, int32_t* d_vert_one,
                          int32_t* d_vert_ext0, uint8_t* d_status, void* d_work, int64_t work_bytes, void* stream);
int tlc_pd_filtration_grad(int64_t n_graphs, const int64_t* d_node_offs, const int64_t* d_edge_offs, const int32_t* d_counts,
                           const int32_t* d_vert_up, const int32_t* d_vert_down, const int32_t* d_vert_one,
                           const int32_t* d_vert_ext0, const double* d_g_up, const double* d_g_down, const double* d_g_one,
                           const double* d_g_ext0, const uint8_t* d_status, double* d_grad_f, void* d_work, int64_t work_bytes,
                           void* stream);

/* ---- P9: PersistenceImager(resolution=res).transform (sg2dgm/PersistenceImager.pyx:352-388) -------
 * isotropic sigma=1 Gaussian, ranges [0,1]^2, linear-ramp weight (:9-30), birth-death input (skew=True).
 *   d_offs int64[n_dgms+1];  d_pts float64[sum k, 2];  d_out float64[n_dgms, res*res] */
int tlc_pi_raster(int32_t n_dgms, const int64_t* d_offs, const double* d_pts, int res, double* d_out,
                  void* stream);
/* Backward of the DIFFERENTIABLE imager, Knowledge_Distillation/pimg.py:354-400 (Teacher_Model.forward(grad_PI=True),
 * Teacher_model.py:80-81).  The reference computes a point's two normal-CDF factors from detached coordinates (:392,395), so a
 * point reaches the image through its weight alone, linear_ramp(death - birth) (:11-30, :371): d_grad_pts[i] = (-g, +g) with
 * g = sum_pixels d_grad_img[diagram of i] * (dPhi_b * dPhi_p of point i) for 0 <= death - birth <= 1, else 0.
 *   d_grad_img float64[n_dgms, res*res];  d_grad_pts float64[n_pts, 2] (every row written) */
int tlc_pi_raster_wgrad(int32_t n_dgms, int64_t n_pts, const int64_t* d_offs, const double* d_pts, int res,
                        const double* d_grad_img, double* d_grad_pts, void* stream);

/* ---- M1-M3: TLCGNN forward (baselines/TLCGNN.py:19-62) ------------------------------------------- */

/* gcn_norm of GCNConv(cached=True) (in-tree spec: Knowledge_Distillation/PD_conv.py:35-70): add the
 * remaining self loops (w=1), deg = scatter_add(w, target), norm = d^-1/2[src] * w * d^-1/2[dst];
 * result as CSR by target row, sources ascending inside a row.
 *   d_edge_index int64[2,n_edges] (row 0 = source, row 1 = target), existing self loops keep w=1 once
 *   d_rowptr int32[n_nodes+1]; d_col int32[n_edges+n_nodes]; d_val float32[n_edges+n_nodes]
 *   d_nnz int32[1]: entries actually written (<= n_edges+n_nodes) */
int tlc_gcn_norm_csr(int32_t n_nodes, int64_t n_edges, const int64_t* d_edge_index,
                     int32_t* d_rowptr, int32_t* d_col, float* d_val, int32_t* d_nnz, void* stream);

/* C[M,N] = A[M,K] @ B[K,N] (+bias[N]) (optional ReLU), fp32 in / fp32 accumulate on the f32 MFMA.
 * The dense projection x @ W of GCNConv (PD_conv.py:179-181). Row-major, leading dims = N/K. */
int tlc_gemm_f32(int32_t M, int32_t N, int32_t K, const float* d_A, const float* d_B, const float* d_bias,
                 int relu, float* d_C, void* stream);

/* The same product for a SPARSE A given as CSR (rowptr int32[M+1], col int32[nnz] < K, val f32[nnz]): the feature projection
 * x @ W of GCNConv (PD_conv.py:179-181) on bag-of-words / TF-IDF features (PubMed: 10 % non-zeros): the zeros contribute
 * nothing, a tenth of the flops.  B is staged in LDS in column slices of at most 64 (N = 100: 52 + 48): K * slice * 4 B + 1 KiB
 * <= 160 KiB, i.e. K <= 636 for a 64-column slice (TLC_ERR_UNSUPPORTED beyond).  Sums in a fixed order of its own (within 1e-5
 * relative of the dense product).  nnz < 2^29 (byte offsets of the entries are 32-bit). */
int tlc_spgemm_csr_dense_f32(int32_t M, int32_t K, int32_t N, const int32_t* d_rowptr, const int32_t* d_col, const float* d_val,
                             const float* d_B, const float* d_bias, int relu, float* d_C, void* stream);

/* Y[n,k] = act( CSR(rowptr,col,val) @ X[n,k] + bias[k] ): the propagate/scatter-add of GCNConv
 * (PD_conv.py:183-188; message_passing.py:275-293 aggr='add').  relu: bit 0 = ReLU; bit 1 = afterwards renormalise
 * every row like tlc_renorm_rows_f32 (the emb.renorm_ of TLCGNN.py:48 fused into the last layer's aggregation). */
int tlc_spmm_csr_f32(int32_t n_rows, const int32_t* d_rowptr, const int32_t* d_col, const float* d_val,
                     const float* d_X, int32_t k, const float* d_bias, int relu, float* d_Y, void* stream);

/* emb.renorm_(2, 0, 1) (TLCGNN.py:48): rows with L2 norm > 1 are scaled by 1/(norm + 1e-7), in place. */
int tlc_renorm_rows_f32(int32_t n_rows, int32_t k, float* d_emb, void* stream);

/* Net.encode in eval mode (baselines/TLCGNN.py:19-26: conv1 -> ReLU -> conv2 on the normalised adjacency of tlc_gcn_norm_csr)
 * as ONE call: tlc_gemm_f32, tlc_spmm_csr_f32 (+ b1, ReLU), tlc_gemm_f32, tlc_spmm_csr_f32 (+ b2; `flags` bit 0 = ReLU, bit 1 =
 * the emb.renorm_(2, 0, 1) of TLCGNN.py:48) submitted back to back.  d_ws: float32[tlc_gcn2_encode_work_floats(n_nodes, hidden,
 * out_dim)] scratch; d_emb: [n_nodes, out_dim].  hidden, out_dim <= 128.
 * The tlc_*_work_floats / tlc_*_work_ints functions of this header are host arithmetic (no device needed): the element count of the
 * scratch their entry takes as a bare pointer, -1 for a negative size.  The entry writes nowhere behind that count. */
int64_t tlc_gcn2_encode_work_floats(int32_t n_nodes, int32_t hidden, int32_t out_dim);
int tlc_gcn2_encode_f32(int32_t n_nodes, const int32_t* d_rowptr, const int32_t* d_col, const float* d_val,
                        const float* d_x, int32_t f_in, const float* d_w1, const float* d_b1, int32_t hidden,
                        const float* d_w2, const float* d_b2, int32_t out_dim, int flags, float* d_ws, float* d_emb, void* stream);

/* The same with the node features given as CSR (d_xs_rowptr int32[n_nodes+1], d_xs_col int32[nnz] < f_in, d_xs_val f32[nnz]): the
 * first projection is tlc_spgemm_csr_dense_f32 (its limit on f_in applies).  What Net.encode runs on PubMed's TF-IDF features. */
int tlc_gcn2_encode_csr_f32(int32_t n_nodes, const int32_t* d_rowptr, const int32_t* d_col, const float* d_val,
                            const int32_t* d_xs_rowptr, const int32_t* d_xs_col, const float* d_xs_val, int32_t f_in,
                            const float* d_w1, const float* d_b1, int32_t hidden, const float* d_w2, const float* d_b2,
                            int32_t out_dim, int flags, float* d_ws, float* d_emb, void* stream);

/* Net.decode after the renorm (TLCGNN.py:52-61), one fused pass per pair:
 *   h = LeakyReLU_0.2( W1 @ [ (emb[u]-emb[v])^2 || PI ] + b1 );  d = clamp(|W2 @ h + b2|, 0, 40);
 *   prob = 1 / (exp(d - 2) + 1)
 *   d_pairs int32[n_pairs,2]; d_emb float32[n_nodes,emb_dim]; d_pi float64[n_pairs,pi_dim] (cast to
 *   float32 on load, as torch.Tensor(PI) does); d_W1 float32[pi_dim, emb_dim+pi_dim] (torch Linear
 *   layout [out,in]); d_b1[pi_dim]; d_W2 float32[pi_dim]; d_b2 float32[1]; d_prob float32[n_pairs] */
int tlc_lp_decode_fused(int64_t n_pairs, const int32_t* d_pairs, const float* d_emb, int32_t emb_dim,
                        const double* d_pi, int32_t pi_dim, const float* d_W1, const float* d_b1,
                        const float* d_W2, const float* d_b2, float* d_prob, void* stream);
/* The same pass over a float32 image table [n_pairs, pi_dim]: the reference casts the images to float32 before the layer on
 * every decode (`PI = torch.Tensor(self.PI[...])`, TLCGNN.py:35-36,52-53); a caller that casts its table ONCE at set-up hands
 * it in here -- same values (the cast is the same rounding), 100 instead of 200 bytes per pair.  Both forms run the hidden
 * layer on the f32 MFMA when emb_dim == 16 and pi_dim == 25 (one lane per pair, K = 1 MFMAs in the reference's summation order,
 * weights in registers, no LDS). */
int tlc_lp_decode_fused_f32(int64_t n_pairs, const int32_t* d_pairs, const float* d_emb, int32_t emb_dim,
                            const float* d_pi, int32_t pi_dim, const float* d_W1, const float* d_b1,
                            const float* d_W2, const float* d_b2, float* d_prob, void* stream);

/* ---- The backward of the LP training step (pipelines.py:10-18, loss.backward()) -------------------------------------------
 * Deterministic like the forward: no atomics, every sum in an order fixed by the shapes, the same inputs give bit-identical
 * gradients. */

/* A^T of the normalised adjacency of tlc_gcn_norm_csr, as a CSR whose rows are the forward's sources (d(XW) = A^T G runs on
 * tlc_spmm_csr_f32): the structure of the flipped edge list under the same self-loop rule, targets ascending inside a row, the
 * forward's values (degrees = the forward rows' in-degrees; edge_index need not be symmetric).  d_rowptr: the forward operator's
 * row pointers.  d_rowptr_t int32[n_nodes+1]; d_col_t int32[n_edges+n_nodes]; d_val_t f32[n_edges+n_nodes]; d_nnz int32[1].
 * One-off (allocates, waits for the stream). */
int tlc_gcn_norm_csr_t(int32_t n_nodes, int64_t n_edges, const int64_t* d_edge_index, const int32_t* d_rowptr,
                       int32_t* d_rowptr_t, int32_t* d_col_t, float* d_val_t, int32_t* d_nnz, void* stream);

/* C[M,N] = A[K,M]^T @ B[K,N], row-major, fp32 on the f32 MFMA: dW = X^T d(XW) of GCNConv.  Split-K (at most 32 splits) with
 * the partials added in split order.  d_A NULL with M = 1: C = the column sums of B (bias gradients).  M, N >= 1, K >= 0 (K = 0:
 * zeros).  d_work float32[tlc_gemm_tn_work_floats(M, N)] scratch. */
int64_t tlc_gemm_tn_work_floats(int32_t M, int32_t N);
int tlc_gemm_tn_f32(int32_t M, int32_t N, int64_t K, const float* d_A, const float* d_B, float* d_C, float* d_work, void* stream);

/* Backward of tlc_lp_decode_fused_f32 and of the emb.renorm_(2, 0, 1) in front of it (TLCGNN.py:48-61), emb_dim 16 / pi_dim 25
 * (else TLC_ERR_UNSUPPORTED).  d_emb_pre f32[n_nodes,16]: the rows before the renorm; d_emb: after it (what the forward read);
 * d_pi f32[n_pairs,25]; d_gprob f32[n_pairs] = d loss / d prob.  The pair endpoints grouped by node, in the order their
 * contributions are added: d_node_ptr int32[n_nodes+1], d_node_slots int32[2 n_pairs] (slot 2 i = pair i's first endpoint,
 * 2 i + 1 its second).  Out: d_gemb f32[n_nodes,16] = d loss / d emb_pre; d_gw f32[1076] = dW1 [25][41] | db1 [25] | dW2 [25] |
 * db2 [1].  d_work float32[tlc_lp_decode_bwd_work_floats(n_pairs)] scratch (16-byte aligned, like d_emb). */
int64_t tlc_lp_decode_bwd_work_floats(int64_t n_pairs);
int tlc_lp_decode_bwd_f32(int64_t n_pairs, const int32_t* d_pairs, const float* d_emb_pre, const float* d_emb, int32_t n_nodes,
                          int32_t emb_dim, const float* d_pi, int32_t pi_dim, const float* d_W1, const float* d_b1,
                          const float* d_W2, const float* d_b2, const float* d_gprob, const int32_t* d_node_ptr,
                          const int32_t* d_node_slots, float* d_gemb, float* d_gw, float* d_work, void* stream);

/* ---- Node classification: curvGN of Knowledge_Distillation/ConvCurv_GIN.py:149-185 (nc_curv.hip) ---------------------------------
 * out[t] = sum over the edges e with edge_index[1][e] = t of alpha[e] * xl[edge_index[0][e]] (per channel), xl = x W^T + b, and
 * alpha = softmax of wt = W2 PReLU(W1 w_mul[e]) + b2 over the edges of one SOURCE, per channel (PyG's softmax: max, exp, / (sum + 1e-16)).
 * f32 throughout; C (channels) 1..256, D (w_mul width) 1..64, any F; E < 2^31.  Every call is asynchronous on `stream`, never waits
 * for the host and uses no floating-point atomics: the same inputs give bit-identical results on every call.  Bad sizes / NULL
 * pointers: TLC_ERR_INVALID_ARG; C, D or E beyond the built range: TLC_ERR_UNSUPPORTED. */

/* Scratch (int32 words) of the grouping: 2 n_nodes + 4 n_edges; -1 for bad sizes. */
int64_t tlc_nc_group_work_ints(int32_t n_nodes, int64_t n_edges);

/* Group the edge ids of d_edge_index int64[2,E] (row 0 source, row 1 target) by source and by target, a stable counting sort (edge ids
 * ascending inside a row); edges are kept as given (duplicates and self loops stay).  Out: d_groups int32[2 (n_nodes + 1) + 4 E] =
 * src_ptr[n+1] | tgt_ptr[n+1] | src_eid[E] | tgt_eid[E] | src[E] | dst[E].  d_bad int32[1] = the number of edges with an id outside
 * [0, n_nodes) (read it before using the grouping: such edges are left out).  d_work int32 scratch (tlc_nc_group_work_ints). */
int tlc_nc_group(int32_t n_nodes, int64_t n_edges, const int64_t* d_edge_index, int32_t* d_groups, int32_t* d_work, int32_t* d_bad,
                 void* stream);

/* y[M,N] = x[M,K] W^T + b on the f32 MFMA: a Linear with weight d_w f32[N,K] and bias d_b f32[N] (NULL: none).  Any N and K. */
int tlc_nc_linear_f32(int32_t M, int32_t N, int32_t K, const float* d_x, const float* d_w, const float* d_b, float* d_y, void* stream);

/* Backward of tlc_nc_linear_f32 for d_gy f32[M,N]: d_gw f32[N,K] = gy^T x, d_gb f32[N] = column sums of gy (NULL: skipped), d_gx f32[M,K]
 * = gy W (NULL: skipped).  Sums over M as fixed-order split-K products.  d_work float32[tlc_nc_linear_bwd_work_floats(N, K)] scratch. */
int64_t tlc_nc_linear_bwd_work_floats(int32_t N, int32_t K);
int tlc_nc_linear_bwd_f32(int32_t M, int32_t N, int32_t K, const float* d_x, const float* d_w, const float* d_gy, float* d_gx,
                          float* d_gw, float* d_gb, float* d_work, void* stream);

/* Workspace bytes of tlc_nc_curv_bwd_f32: 4 (3 E C + ceil(E / 64) C + 32 C max(C, D)); -1 for sizes outside the built range. */
int64_t tlc_nc_curv_work_bytes(int32_t n_nodes, int64_t n_edges, int32_t C, int32_t D);

/* Forward of curvGN after the projection: d_groups from tlc_nc_group; d_xl f32[n_nodes,C]; d_wmul f32[E,D]; the edge MLP
 * create_wmlp([D, C], C, 1): d_w1 f32[C,D] (Linear, no bias), d_prelu f32[C] (PReLU slopes), d_w2 f32[C,C], d_b2 f32[C].
 * Out: d_alpha f32[E,C] (kept for the backward), d_out f32[n_nodes,C]; a node without in-edges gets a zero row. */
int tlc_nc_curv_fwd_f32(int32_t n_nodes, int64_t n_edges, int32_t C, int32_t D, const int32_t* d_groups, const float* d_xl,
                        const float* d_wmul, const float* d_w1, const float* d_prelu, const float* d_w2, const float* d_b2, float* d_alpha,
                        float* d_out, void* stream);

/* Backward of tlc_nc_curv_fwd_f32 for d_gout f32[n_nodes,C] (d_alpha: the forward's): d_gxl f32[n_nodes,C], d_gw1 f32[C,D],
 * d_gprelu f32[C], d_gw2 f32[C,C], d_gb2 f32[C].  The edge MLP is recomputed from d_wmul.  d_work: tlc_nc_curv_work_bytes bytes. */
int tlc_nc_curv_bwd_f32(int32_t n_nodes, int64_t n_edges, int32_t C, int32_t D, const int32_t* d_groups, const float* d_xl,
                        const float* d_wmul, const float* d_w1, const float* d_prelu, const float* d_w2, const float* d_alpha,
                        const float* d_gout, float* d_gxl, float* d_gw1, float* d_gprelu, float* d_gw2, float* d_gb2, void* d_work,
                        int64_t work_bytes, void* stream);

/* ---- Link-prediction scoring (pipelines.py:20-40: roc_auc_score / average_precision_score) ----------------------------------
 * Binary ranking metrics per segment, with sklearn's binary semantics (pos_label 1): scores in descending order, equal scores one
 * threshold, -0.0 == +0.0.  AUC = U2 / (2 P N) with one rounding, U2 = sum over tie groups g of p_g (2 N_below,g + n_g) exact in
 * int64; AP = sum_g (p_g / P) tp_g / (tp_g + fp_g) in f64 (tp / fp cumulative through g).  Deterministic: no floating-point
 * atomics; a segment gives the same bits alone or among others.
 *   d_scores: TLC_SCORE_F32 / TLC_SCORE_F64; d_labels: TLC_LABEL_U8 (also bool) / TLC_LABEL_I64 / TLC_LABEL_F32, each 0 or 1.
 *   h_seg_ptr int64[n_segs + 1] (HOST): segment s = [h_seg_ptr[s], h_seg_ptr[s+1]) of both arrays; n_segs >= 1, h_seg_ptr[0] >= 0,
 *   non-decreasing (else TLC_ERR_INVALID_ARG); a segment of 2^31 scores or more: TLC_ERR_UNSUPPORTED.
 *   Out, per segment (device): d_auc / d_ap f64, d_n_pos / d_n_neg int64, d_status int32 (TLC_RANK_* bits, 0 = valid).  One class
 *   only: AUC NaN, AP 0.0 without positives / 1.0 without negatives (sklearn 1.7).  An empty segment: NaN / NaN, TLC_RANK_EMPTY.
 *   Segments of at most TLC_RANK_LDS_CAP scores are sorted in LDS, one workgroup each, all in one launch (per 64); longer ones by
 *   a multi-workgroup radix sort, one after the other in d_work: tlc_binary_rank_metrics_work_bytes() bytes (0 if no segment
 *   takes the radix tier, -1 for invalid arguments), 16-byte aligned.  TLC_RANK_FORCE_RADIX (tests): every non-empty segment
 *   through the radix tier.  Asynchronous on `stream`, no host synchronisation. */
#define TLC_SCORE_F32          0
#define TLC_SCORE_F64          1
#define TLC_LABEL_U8           0
#define TLC_LABEL_I64          1
#define TLC_LABEL_F32          2
#define TLC_RANK_FORCE_RADIX   0x1u
#define TLC_RANK_NONFINITE     0x1   /* a NaN or +-inf score      */
#define TLC_RANK_BAD_LABEL     0x2   /* a label other than 0 / 1  */
#define TLC_RANK_EMPTY         0x4   /* the segment has no scores */
#define TLC_RANK_LDS_CAP       16384 /* 9 B per score (u64 key + label) in the 160 KiB of LDS of one gfx950 workgroup, a power of 2 */
int64_t tlc_binary_rank_metrics_work_bytes(const int64_t* h_seg_ptr, int32_t n_segs, int score_dtype, uint32_t flags);
int tlc_binary_rank_metrics(const void* d_scores, int score_dtype, const void* d_labels, int label_dtype, const int64_t* h_seg_ptr,
                            int32_t n_segs, uint32_t flags, double* d_auc, double* d_ap, int64_t* d_n_pos, int64_t* d_n_neg,
                            int32_t* d_status, void* d_work, int64_t work_bytes, void* stream);

/* ---- Heat-kernel-signature filtration (Knowledge_Distillation/data_utils_LP.py:96-100,128-130; data_utils_NC.py:88-92,120-122;
 * data_utils_GC.py:90-94,114-116: `hks_signature`, then / (max + 1e-10)) ------------------------------------------------------------
 * For a packed batch of simple undirected graphs -- d_node_ptr / d_edge_ptr int64[n_graphs + 1] (the last entries are total_nodes /
 * total_edges), d_edges int32[total_edges, 2] local ids, each undirected edge ONCE (a pair listed twice, (a, b) (a, b) or (a, b) (b, a),
 * is TLC_ST_BAD_INPUT: scipy would sum it into a multigraph weight, this kernel does not compute weighted graphs) -- per graph
 *   L = I - D^-1/2 A D^-1/2 as scipy.sparse.csgraph.laplacian(normed=True) (a node of degree 0: diagonal 0),
 *   hks_t(x) = sum_k exp(-t lambda_k) phi_k(x)^2 over the eigenpairs of L, fp64,
 * for the n_times (1 .. TLC_HKS_TMAX) values of h_times (HOST; read during the call) from ONE decomposition: d_out f64[n_times,
 * total_nodes], row k bit-equal to a call with h_times[k] alone.  TLC_HKS_NORMALISE: each graph's values divided by (their max + 1e-10).
 * Eigenpairs: cyclic Jacobi, round-robin order, fixed arithmetic per element, no floating-point atomics: a graph's values are the same
 * bits run to run, alone or anywhere in any batch.  Agreement with LAPACK's eigh route: rounding level (<= 1e-11 absolute is tested on
 * normalised values up to n = TLC_HKS_NMAX, t = 10).
 * d_status uint8[n_graphs]: TLC_ST_OK; TLC_ST_TOO_LARGE (more than TLC_HKS_NMAX nodes), TLC_ST_NOT_CONVERGED, TLC_ST_BAD_INPUT -- the
 * graph's slice of d_out is then left untouched and no other graph is affected.  A graph without nodes: TLC_ST_OK, nothing written.
 * The graphs are binned into size tiers on the device (<= 32 nodes: a wavefront each, matrices in LDS; <= 64 and <= TLC_HKS_LDS_NMAX:
 * a workgroup each, matrices in LDS; <= TLC_HKS_NMAX: a workgroup each, matrices in d_work); nothing is read back, no host wait.
 * d_work: tlc_hks_batch_work_bytes() bytes, 16-byte aligned -- the tier lists (16 B per graph) and one 1.0 MiB slot of matrices per
 * resident workgroup of the last tier: min(CUs of the current device, total_nodes / (TLC_HKS_LDS_NMAX + 1)) slots, reused graph after
 * graph.  Runs on the caller's current device, asynchronous on `stream`. */
#define TLC_HKS_NMAX           256   /* most nodes of a graph; above it TLC_ST_TOO_LARGE */
#define TLC_HKS_LDS_NMAX       96    /* most nodes of a graph whose two n x n fp64 arrays stay in the 160 KiB of LDS */
#define TLC_HKS_TMAX           8     /* most times per call */
#define TLC_HKS_NORMALISE      0x1u
int tlc_hks_batch_work_bytes(int64_t n_graphs, int64_t total_nodes, int64_t total_edges, int32_t n_times, int64_t* bytes);
int tlc_hks_batch(const int64_t* d_node_ptr, const int64_t* d_edge_ptr, const int32_t* d_edges, int64_t n_graphs, int64_t total_nodes,
                  int64_t total_edges, const double* h_times, int32_t n_times, uint32_t flags, double* d_out, uint8_t* d_status,
                  void* d_work, int64_t work_bytes, void* stream);
/* tlc_hks_batch with the derivative in the diffusion time.  d_dout f64[n_times, total_nodes] is d/dt of exactly what d_out holds:
 *   d/dt hks_t(x) = - sum_k lambda_k exp(-t lambda_k) phi_k(x)^2   (k ascending, from the eigenpairs of the value),
 * and under TLC_HKS_NORMALISE, with f = hks / (mx + 1e-10) and mx = hks(a) taken at the LOWEST index a that attains the maximum,
 *   d/dt f(x) = (hks'(x) - f(x) hks'(a)) / (mx + 1e-10).
 * A node of degree 0 has derivative 0; at t = 0 every node of degree > 0 has -1 (raw).  d_out and d_status are bit for bit what
 * tlc_hks_batch writes for the same arguments; row k of d_dout is bit-equal to a call with h_times[k] alone; a graph whose status is
 * not TLC_ST_OK keeps both slices untouched.  Same workspace (tlc_hks_batch_work_bytes) and refusals, plus a null d_dout, all decided
 * before anything is launched. */
int tlc_hks_batch_dt(const int64_t* d_node_ptr, const int64_t* d_edge_ptr, const int32_t* d_edges, int64_t n_graphs, int64_t total_nodes,
                     int64_t total_edges, const double* h_times, int32_t n_times, uint32_t flags, double* d_out, double* d_dout,
                     uint8_t* d_status, void* d_work, int64_t work_bytes, void* stream);

/* ---- Heat-kernel signatures of graphs above TLC_HKS_NMAX nodes ---------------------------------------------------------------------------
 * The same values for SELECTED graphs of the packed batch of tlc_hks_batch, without eigenpairs: hks_t(v) = [exp(-t L)]_vv, and with
 * M = D^-1/2 A D^-1/2, [exp(-t L)]_vv = exp(-t) [exp(t M)]_vv for a node of degree > 0 and 1 for a node of degree 0.  Per time:
 * s = the least integer >= 0 with t / 2^s <= 1/2, X = (t / 2^s) M, the Taylor series of exp(X) to degree 14 by Horner (13 products),
 * times exp(-t / 2^s), s - 1 squarings, and the row sums of squares of the last matrix (s = 0: its diagonal) -- dense symmetric fp64
 * products on the matrix cores (v_mfma_f64_16x16x4_f64), 64 x 64 output tiles on and above the diagonal, mirrored on store.  No entry is
 * negative, so nothing cancels; every K-sum runs in one fixed order, no split-K, no floating-point atomics: a graph's values are the same
 * bits run to run, alone or in any selection, with any workspace.  Agreement with LAPACK's eigh route: <= 1e-11 absolute is tested up to
 * n = TLC_HKS_LARGE_NMAX, t = TLC_HKS_LARGE_TIME_MAX.
 * h_sel (HOST) int64[n_sel]: the indices of the graphs to compute, strictly ascending inside 0 .. n_graphs-1; h_sel_nodes (HOST)
 * int64[n_sel]: their node counts as the caller knows them (slots and groups are sized from them; nothing is read back, no host wait).
 * Only the slices of d_out f64[n_times, total_nodes] and the bytes of d_status u8[n_graphs] of selected graphs are written: TLC_ST_OK;
 * TLC_ST_TOO_LARGE (a declared count above TLC_HKS_LARGE_NMAX); TLC_ST_BAD_INPUT (the contract of tlc_hks_batch on offsets and edges,
 * or a declared count that is not node_ptr[g + 1] - node_ptr[g]: checked on the device before anything is indexed with it) -- the
 * slice is then left untouched.  A selected graph may have any size from 0 on (small ones are merely wasteful); no nodes: TLC_ST_OK,
 * nothing written.  n_times, flags (TLC_HKS_NORMALISE), row k of d_out bit-equal to a call with h_times[k] alone: as tlc_hks_batch.
 * d_work: 16-byte aligned, any work_bytes >= *min_bytes (the largest selected graph alone: three np x np fp64 matrices, np = n rounded
 * up to 64, and its lists); *all_bytes lets every selected graph run at once; in between the selection runs in groups that fit, in
 * h_sel order.  tlc_hks_large_work_bytes is host arithmetic (no device needed); both are 0 for an empty selection.
 * TLC_ERR_INVALID_ARG (nothing launched): null pointers, h_sel not ascending or out of range, a negative count, n_times outside
 * 1 .. TLC_HKS_TMAX, an unknown flag, a time outside [0, TLC_HKS_LARGE_TIME_MAX] or not finite, work_bytes < *min_bytes, d_work misaligned.
 * Runs on the caller's current device, asynchronous on `stream`. */
#define TLC_HKS_LARGE_NMAX      4096   /* most nodes of a graph; above it TLC_ST_TOO_LARGE, slice untouched */
#define TLC_HKS_LARGE_TIME_MAX  64.0   /* times outside [0, 64] or not finite: TLC_ERR_INVALID_ARG, nothing launched */
int tlc_hks_large_work_bytes(const int64_t* h_sel_nodes, int64_t n_sel, int32_t n_times, int64_t* min_bytes, int64_t* all_bytes);
int tlc_hks_large_batch(const int64_t* d_node_ptr, const int64_t* d_edge_ptr, const int32_t* d_edges, int64_t n_graphs,
                        int64_t total_nodes, int64_t total_edges, const int64_t* h_sel, const int64_t* h_sel_nodes, int64_t n_sel,
                        const double* h_times, int32_t n_times, uint32_t flags, double* d_out, uint8_t* d_status,
                        void* d_work, int64_t work_bytes, void* stream);
/* tlc_hks_large_batch with the derivative in the diffusion time, d_dout f64[n_times, total_nodes] as in tlc_hks_batch_dt, from
 *   d/dt hks_t(v) = -[L K_t]_vv = -[K_t]_vv + sum over the neighbours u of v of [K_t]_uv / sqrt(d_u d_v),   K_t = exp(-t L):
 * no product beyond those of the value.  The last matrix P is K_t (s = 0: [K_t]_uv = P_uv) or K_t/2 ([K_t]_uv = sum_j P_uj P_vj, a row
 * dot per edge end); the neighbours are walked u ascending in partial sums of 64 columns; t = 0 is answered directly (-1 for degree
 * > 0).  No floating-point atomics: the bits depend on the graph and the time alone, with any workspace.  d_out and d_status are bit
 * for bit tlc_hks_large_batch's; same workspace (tlc_hks_large_work_bytes) and refusals, plus a null d_dout. */
int tlc_hks_large_batch_dt(const int64_t* d_node_ptr, const int64_t* d_edge_ptr, const int32_t* d_edges, int64_t n_graphs,
                           int64_t total_nodes, int64_t total_edges, const int64_t* h_sel, const int64_t* h_sel_nodes, int64_t n_sel,
                           const double* h_times, int32_t n_times, uint32_t flags, double* d_out, double* d_dout, uint8_t* d_status,
                           void* d_work, int64_t work_bytes, void* stream);

/* ---- Heat-kernel signatures of sparse graphs of any size ---------------------------------------------------------------------------------
 * The same values for SELECTED graphs of the packed batch of tlc_hks_batch, without eigenpairs and without a dense matrix: with
 * M = D^-1/2 A D^-1/2, L = I - M and tau = t / 2, a node v of degree > 0 has
 *   y_v = exp(-tau L) e_v = exp(-tau) sum_{k = 0 .. K} z_k,   z_0 = e_v,   z_k = (tau / k) M z_{k-1},
 *   hks_t(v) = sum_u y_v[u]^2,        d/dt hks_t(v) = -(sum_u y_v[u]^2 - y_v^T M y_v);
 * a node of degree 0 has value 1 and derivative 0.  M has no negative entry, so no term cancels.  The work is n K 2m multiply-adds per
 * graph and time.  The contract of tlc_hks_large_batch holds (selection, 1 .. TLC_HKS_TMAX times, TLC_HKS_NORMALISE with the maximum at
 * its lowest index, the quotient rule of tlc_hks_batch_dt, a status byte per selected graph, slices of graphs that are not TLC_ST_OK
 * untouched, row k of d_out / d_dout bit-equal to a call with h_times[k] alone), with h_sel_edges (HOST) int64[n_sel], the selected
 * graphs' edge counts, beside h_sel_nodes: the workspace is laid out from both, nothing is read back, no host wait.  A declared count
 * (nodes or edges) that is not the device's, offsets out of order, an id out of range, a self loop, an unordered pair listed twice in
 * either orientation, or more than n (n - 1) / 2 edges: TLC_ST_BAD_INPUT.  There is no node cap and no TLC_ST_TOO_LARGE; ids are 32-bit:
 * the selected graphs together have fewer than 2^31 - 1 nodes and fewer than 2^30 edges.
 * K = tlc_hks_sparse_terms(t): the least k >= 0 with k + 2 > tau and
 *   (tau^(k+1) / (k+1)!) / (1 - tau / (k + 2)) / E * (1 + 2^-40) <= 2^-64,     E = sum_{j = 0 .. 400} tau^j / j!  (j ascending),
 * a bound on the Poisson(tau) tail beyond k, in IEEE double +, *, / only (term_j = term_{j-1} * tau / j; no libm call): the same K on
 * every host.  K = 0 at t = 0; 9, 16, 36, 96 at t = 0.1, 1, 10, 64; -1 for a time outside [0, TLC_HKS_SPARSE_TIME_MAX] or not finite.
 * The operation sequence (fp64, no fused multiply-add, no floating-point atomics; it fixes the bits):
 *   CSR.  Every edge (a, b) gives the entries (a, b) and (b, a); the entries of the selection are sorted by (row, column) with the
 *     shared radix driver, so a row's neighbours ascend and a repeat shows as two adjacent equal entries.  deg(u) is the integer length
 *     of row u, r_u = 1.0 / sqrt((double)deg(u)) (0.0 for degree 0).
 *   Row sum R_u(x) of a vector x: the neighbours of u in chunks of TLC_HKS_SPARSE_PANEL (64) consecutive ones; a chunk's partial sum
 *     starts at +0.0 and adds x[w], w ascending; R_u is +0.0 plus the partial sums, chunks ascending.  Rows above
 *     TLC_HKS_SPARSE_LONG_ROW neighbours are split over wavefronts along these same cuts (the partial sums go through d_work), so a
 *     hub neither serialises a launch nor changes a bit.
 *   Column v (one lane; TLC_HKS_SPARSE_PANEL consecutive columns make a panel):  S = e_v, s = r_v e_v; for k = 1 .. K, with
 *     c_k = tau / k (host):  z[u] = (c_k * r_u) * R_u(s);  S[u] = S[u] + z[u];  s[u] = r_u * z[u]  (all u, then the next k).
 *     y[u] = exp(-tau) * S[u] (the host's exp), q[u] = r_u * y[u], and for the derivative g[u] = q[u] * R_u(q).
 *   Sums over u (value: y[u] * y[u]; quadratic form: g[u]): blocks of 64 consecutive rows, a block's partial sum from +0.0 with u
 *     ascending, then +0.0 plus the partial sums, blocks ascending.  hks = that sum, d hks / dt = quadratic form - value.
 * One launch per Taylor step (and one for the split rows' partial sums, where a graph of the group can have such a row: min(n - 1, m)
 * above TLC_HKS_SPARSE_LONG_ROW) serves every panel of a group, and with them every graph of the
 * group.  d_work: 16-byte aligned; *min_bytes holds the CSR of the selection and the vectors of one panel of the largest graph,
 * *all_bytes those of every panel of every graph; any work_bytes in between runs the panels in groups that fit -- the same bits.
 * tlc_hks_sparse_work_bytes is host arithmetic (no device needed); both are 0 for an empty selection.
 * TLC_ERR_INVALID_ARG (nothing launched): what tlc_hks_large_batch refuses (with TLC_HKS_SPARSE_TIME_MAX), a negative edge count, or a
 * selection beyond the 32-bit limits above.  Runs on the caller's current device, asynchronous on `stream`. */
#define TLC_HKS_SPARSE_TIME_MAX  64.0   /* times outside [0, 64] or not finite: TLC_ERR_INVALID_ARG, nothing launched */
#define TLC_HKS_SPARSE_PANEL     64     /* columns of a panel (lane = column); neighbours of a chunk; rows of a block of the sums over u */
#define TLC_HKS_SPARSE_LONG_ROW  256    /* rows with more neighbours are split over wavefronts, chunk by chunk */
int32_t tlc_hks_sparse_terms(double t);
int tlc_hks_sparse_work_bytes(const int64_t* h_sel_nodes, const int64_t* h_sel_edges, int64_t n_sel, int32_t n_times, int64_t* min_bytes,
                              int64_t* all_bytes);
int tlc_hks_sparse_batch(const int64_t* d_node_ptr, const int64_t* d_edge_ptr, const int32_t* d_edges, int64_t n_graphs,
                         int64_t total_nodes, int64_t total_edges, const int64_t* h_sel, const int64_t* h_sel_nodes,
                         const int64_t* h_sel_edges, int64_t n_sel, const double* h_times, int32_t n_times, uint32_t flags, double* d_out,
                         uint8_t* d_status, void* d_work, int64_t work_bytes, void* stream);
int tlc_hks_sparse_batch_dt(const int64_t* d_node_ptr, const int64_t* d_edge_ptr, const int32_t* d_edges, int64_t n_graphs,
                            int64_t total_nodes, int64_t total_edges, const int64_t* h_sel, const int64_t* h_sel_nodes,
                            const int64_t* h_sel_edges, int64_t n_sel, const double* h_times, int32_t n_times, uint32_t flags,
                            double* d_out, double* d_dout, uint8_t* d_status, void* d_work, int64_t work_bytes, void* stream);

/* ---- Degree / centrality / clustering filtrations (Knowledge_Distillation/data_utils_LP.py:131-133; data_utils_NC.py:124-135: networkx's
 * degree(), degree_centrality and clustering of the vicinity, then / (max + 1e-10)) ------------------------------------------------------
 * For the packed batch of tlc_hks_batch (simple undirected graphs, each edge ONCE, local ids), per node v of a graph of n nodes with
 * d = its degree and t = the sum over its incident edges (v, w) of |N(v) & N(w)| (each triangle at v twice):
 *   TLC_STRUCT_DEGREE      d
 *   TLC_STRUCT_CENTRALITY  d * (1.0 / (n - 1.0)) -- the reciprocal first, then one multiply; n == 1: 1.0
 *   TLC_STRUCT_CLUSTERING  t / (d * (d - 1)); 0.0 where t == 0
 * d_out f64[popcount(kinds), total_nodes], rows in the order degree, centrality, clustering of the bits set in `kinds`; each row bit-equal
 * to a call with that kind alone.  TLC_STRUCT_NORMALISE: each graph's values divided by (their max + 1e-10).
 * d and t are integers, counted with integer atomics or fixed-order sums, followed by one or two correctly rounded fp64 operations; no
 * floating-point atomics: the values are bit for bit those of the host route (`structural_filtration`), run to run, alone or in any batch.
 * d_status uint8[n_graphs]: TLC_ST_OK, or TLC_ST_BAD_INPUT -- offsets out of order or beyond the totals, an id outside 0 .. n-1, a self
 * loop, an unordered pair listed twice in either orientation (more than n (n - 1) / 2 edges is refused as such without looking at them),
 * more than 2^31 - 1 nodes (int32 ids cannot name them); nothing out of range is dereferenced, the graph's slice of d_out is left untouched
 * and no other graph is affected.  There is no size cap: a graph of any size the int32 ids can express is computed on the device.  A graph
 * without nodes: TLC_ST_OK, nothing written.
 * Tiers, binned on the device (nothing is read back, no host wait): <= TLC_STRUCT_WAVE_NMAX nodes a wavefront each (a u64 adjacency row per
 * lane in LDS); <= TLC_STRUCT_LDS_SMALL_NMAX and <= TLC_STRUCT_LDS_NMAX a workgroup each (adjacency bitmap in LDS, work per edge); larger: a
 * workgroup each over a CSR built in d_work, neighbour bitmaps of TLC_STRUCT_BITMAP_BITS bits per wavefront in LDS, 64-bit counts.
 * d_work: tlc_struct_batch_work_bytes() bytes, 16-byte aligned: the tier lists (16 B per graph) and, when total_nodes > TLC_STRUCT_LDS_NMAX,
 * 16 B per node + 16 B per graph + 8 B per edge for the CSR tier.  Runs on the caller's current device, asynchronous on `stream`. */
#define TLC_STRUCT_DEGREE           0x1u
#define TLC_STRUCT_CENTRALITY       0x2u
#define TLC_STRUCT_CLUSTERING       0x4u
#define TLC_STRUCT_NORMALISE        0x100u
#define TLC_STRUCT_WAVE_NMAX        64      /* most nodes of a graph that one wavefront computes */
#define TLC_STRUCT_LDS_SMALL_NMAX   256     /* ... whose adjacency bitmap takes the narrow LDS tier (12 KiB) */
#define TLC_STRUCT_LDS_NMAX         1024    /* ... whose adjacency bitmap fits LDS: 1024 rows of 16 + 1 u64 words, 136 KiB of the 160 KiB */
#define TLC_STRUCT_BITMAP_BITS      65536   /* CSR tier: bits of one wavefront's neighbour bitmap (8 KiB) */
int tlc_struct_batch_work_bytes(int64_t n_graphs, int64_t total_nodes, int64_t total_edges, uint32_t kinds, int64_t* bytes);
int tlc_struct_batch(const int64_t* d_node_ptr, const int64_t* d_edge_ptr, const int32_t* d_edges, int64_t n_graphs,
                     int64_t total_nodes, int64_t total_edges, uint32_t kinds, uint32_t flags, double* d_out,
                     uint8_t* d_status, void* d_work, int64_t work_bytes, void* stream);

/* ---- Connected components of a packed batch of RAW edge lists, the largest one extracted (Knowledge_Distillation/data_utils_GC.py:
 * 240-248: self loops removed, nx.Graph, the largest connected component, convert_node_labels_to_integers) ------------------------------
 * Input: the packed batch of tlc_hks_batch (d_node_ptr / d_edge_ptr int64[n_graphs + 1], d_edges int32[total_edges, 2] local ids), but
 * the edges as a dataset gives them: both orientations, repeated pairs and self loops are allowed and dropped.  For graph g of n nodes
 * (the specification is `data_utils_GC.largest_component`, integer for integer):
 *   the simple graph = the distinct unordered pairs {a, b}, a != b;
 *   the chosen component = the one with the most nodes, among equals the one that holds the lowest node id (n >= 1 without an edge:
 *   node 0 alone);
 *   its nodes are renumbered 0 .. k-1 in ascending order of the old ids, its edges written as rows (lo, hi), lo < hi, in ascending
 *   lexicographic order.
 * Outputs in SLOT layout (graph g's slices start at its input offsets, like the diagrams of tlc_pd_from_filtration):
 *   d_info int32[n_graphs, 4]: k = nodes of the chosen component, m = its distinct edges, c = components of the simple graph (an
 *   isolated node is one), s = distinct non-loop pairs of the whole graph; a graph without nodes: 0 0 0 0;
 *   d_new_id int32[total_nodes]: the new id of a kept node, -1 for a dropped one (every entry of a computed graph is written);
 *   d_out_edges int32[total_edges, 2]: the first m rows of slot g; the rest of the slot is left untouched;
 *   d_status uint8[n_graphs]: TLC_ST_OK, or TLC_ST_BAD_INPUT -- offsets that are negative, decrease or pass the totals, more nodes than
 *   max_nodes, or an id outside 0 .. n-1, which is found before anything is indexed by it.  A refused graph has nothing written (its
 *   d_info row included) and no other graph is affected.
 * Everything is an integer and the only atomics are integer: a component's label is its lowest node id, the unique fixed point of
 * min-label hooking, counts are integer sums, and the edge order is the order of the sorted keys -- the outputs are the same bits run to
 * run, alone or anywhere in any batch, with any workspace of at least the reported size, whatever number of labelling rounds ran.
 * Size classes, binned on the device from d_node_ptr:
 *   WAVE  n <= TLC_CC_WAVE_NMAX: a wavefront per graph (four per workgroup, persistent, graphs drawn by a ticket).  Lane v owns row v of
 *         the adjacency matrix as one u64 in LDS (atomicOr: repeats and orientation fold into the bit, loops are masked); the rows are
 *         closed in registers by one Warshall sweep over the n pivot rows (readlane), label = lowest bit, size = popcount, the winner a
 *         wavefront maximum of (size, -label), new ids = popcount of the winner's mask below the lane, edges read off the rows.
 *         No host read-back.
 *   WIDE  every larger graph, all of them together in device-wide passes (a batch of thousands costs the launches of one; no node cap
 *         below the totals): keys (global lo id, global hi id), global id = node_ptr[g] + local id, sorted by the shared radix passes
 *         (16 or 32 bits per half, by total_nodes), repeats dropped against the predecessor; labels by hooking with a 32-bit atomicMin
 *         onto the grandparents plus pointer jumping (FastSV: the rounds grow with log n, not with the diameter); sizes by atomicAdd per
 *         label, the winner by a u64 atomicMax of (size << 32 | ~label); new ids and edge rows from two exclusive scans.
 *         Host reads of this class: 8 bytes once (its graphs and keys) and one "changed" word per four rounds; surplus rounds of a
 *         group return at once.
 * max_nodes: an upper bound on the nodes of one graph where the caller has it (a graph above it is TLC_ST_BAD_INPUT), negative where
 * not.  With max_nodes <= TLC_CC_WAVE_NMAX, or total_nodes <= TLC_CC_WAVE_NMAX, no graph can be WIDE and the call reads nothing back.
 * d_work: tlc_graph_components_work_bytes() bytes (host arithmetic: 4 B per graph; with total_nodes > TLC_CC_WAVE_NMAX another 17 B per
 * graph, 16 B per node, 24 B per edge and the sort's histograms), 16-byte aligned.  TLC_ERR_INVALID_ARG with nothing launched: a null
 * pointer, a negative size, total_nodes or total_edges of 2^31 or more, a workspace below the reported size or not 16-byte aligned.
 * n_graphs == 0: TLC_OK, nothing read.  Runs on the caller's current device, asynchronous on `stream` apart from the WIDE class's reads. */
#define TLC_CC_WAVE_NMAX            64      /* most nodes of a graph that one wavefront computes (a u64 adjacency row per lane) */
int tlc_graph_components_work_bytes(int64_t n_graphs, int64_t total_nodes, int64_t total_edges, int64_t* bytes);
int tlc_graph_components(const int64_t* d_node_ptr, const int64_t* d_edge_ptr, const int32_t* d_edges, int64_t n_graphs,
                         int64_t total_nodes, int64_t total_edges, int64_t max_nodes, int32_t* d_info, int32_t* d_new_id,
                         int32_t* d_out_edges, uint8_t* d_status, void* d_work, int64_t work_bytes, void* stream);

/* ---- M4-M6: PDGNN layer forward (Knowledge_Distillation/gat_conv.py:113-216) ----------------------
 * One GATConv(heads=1, new_node_feat, use_edge_attn) layer on a block-diagonal batch of graphs whose
 * edges are given as CSR BY TARGET (self loops already added, gat_conv.py:146-160):
 *   x_l = X @ Wl^T (no bias);  alpha = x_l . att;  per edge j->i: a = softmax_i(leaky_relu(alpha_j+alpha_i)),
 *   m = leaky_relu(Wij @ [x_i || x_j]) * a;  out_i = [ sum m || (min m + max m) ] + bias  (:166-172,202-216)
 *   d_X float32[n, c_in]; d_Wl float32[c_out, c_in]; d_att float32[c_out]; d_Wij float32[c_out, 2*c_out];
 *   d_bias float32[2*c_out]; d_out float32[n, 2*c_out]; prelu_slope < 0 disables the fused PReLU.
 *   d_work float32[tlc_gat_layer_fwd_work_floats(n, c_in, c_out)]: caller-provided scratch (per node: x_l, the two
 *   lin_ij half-projections, alpha; then the layer's weights packed for the MFMA GEMM).
 *   c_out in {8,16,32,64}. */
int64_t tlc_gat_layer_fwd_work_floats(int32_t n_nodes, int32_t c_in, int32_t c_out);
int tlc_gat_layer_fwd(int32_t n_nodes, const int32_t* d_rowptr, const int32_t* d_src,
                      const float* d_X, int32_t c_in, int32_t c_out,
                      const float* d_Wl, const float* d_att, const float* d_Wij, const float* d_bias,
                      float prelu_slope, float* d_work, float* d_out, void* stream);
/* The same layer on a BLOCK-DIAGONAL batch cut into self-contained tiles (round 5; gat_forward.hip, gat_tile_kernel): d_tile_ptr
 * int32[n_tiles + 1] = node offsets of tiles of at most 192 consecutive nodes such that every in-edge of a node has its source in the
 * node's own tile (a batch of small graphs cut at positions no edge crosses: Knowledge_Distillation/gat_conv.py, GraphBatch).  The node
 * rows [P | Q | alpha] are computed on the f32 MFMA into LDS and aggregated from there: they never reach HBM.  c_in = 1 or 64 with
 * c_out = 32 or 16 (the PDGNN layers of Teacher_model.py:182-189); other shapes: TLC_ERR_UNSUPPORTED (take tlc_gat_layer_fwd).
 * d_work: float32[tlc_gat_layer_tiled_fwd_work_floats(c_in, c_out)].  Results equal tlc_gat_layer_fwd's up to the rounding of fp32
 * sums. */
int64_t tlc_gat_layer_tiled_fwd_work_floats(int32_t c_in, int32_t c_out);
int tlc_gat_layer_tiled_fwd(int32_t n_nodes, const int32_t* d_rowptr, const int32_t* d_src, int32_t n_tiles,
                            const int32_t* d_tile_ptr, const float* d_X, int32_t c_in, int32_t c_out,
                            const float* d_Wl, const float* d_att, const float* d_Wij, const float* d_bias,
                            float prelu_slope, float* d_work, float* d_out, void* stream);

/* The tile cut tlc_gat_layer_tiled_fwd takes (Knowledge_Distillation/gat_conv.py GraphBatch -> ops.gat_tiles), made on the device:
 * d_tile_ptr int32[*n_tiles + 1] = node offsets of tiles of at most tile_nodes consecutive nodes, cut only at positions no edge of
 * the CSR (rows = targets, d_col = sources) crosses; with `gap` the largest distance between two such positions next to each other,
 * the first of them at or behind every multiple of tile_nodes - gap starts a tile.  *n_tiles (HOST int; the call waits for the
 * stream) = 0 when 2 gap > tile_nodes -- one big graph: the two-kernel layer (tlc_gat_layer_fwd) serves it.
 * d_work: int32[tlc_gat_tile_cut_work_ints(n_nodes)]; d_tile_ptr: room for tlc_gat_tile_cut_max_tiles(n_nodes, tile_nodes) entries
 * (-1 for n_nodes < 0 or tile_nodes < 1). */
int64_t tlc_gat_tile_cut_work_ints(int32_t n_nodes);
int64_t tlc_gat_tile_cut_max_tiles(int32_t n_nodes, int32_t tile_nodes);
int tlc_gat_tile_cut(int32_t n_nodes, const int32_t* d_rowptr, const int32_t* d_col, int32_t tile_nodes, int32_t* d_work,
                     int32_t* d_tile_ptr, int32_t* n_tiles, void* stream);


/* remove_self_loops + add_self_loops + grouping by target (gat_conv.py:146-152), the structure alone and per BATCH: what
 * tlc_gcn_norm_csr builds without its values, with the caller's temporaries -- nothing is allocated, nothing waits for the stream.
 *   d_rowptr int32[n_nodes+1]; d_col int32[n_edges+n_nodes] (sources ascending inside a row); d_nnz int32[1];
 *   d_work int32[tlc_csr_by_target_work_ints(n_nodes, n_edges)]. */
int64_t tlc_csr_by_target_work_ints(int32_t n_nodes, int64_t n_edges);
int tlc_csr_by_target(int32_t n_nodes, int64_t n_edges, const int64_t* d_edge_index, int32_t* d_rowptr, int32_t* d_col,
                      int32_t* d_nnz, int32_t* d_work, void* stream);

/* Teacher_Model.forward(compute_loss=False) without gradients (Knowledge_Distillation/Teacher_model.py:49-88) as ONE call: CSR by
 * target + tile cut of the batch (skipped when the caller hands in d_rowptr / d_col / d_tile_ptr of a batch it holds; d_tile_ptr NULL
 * with n_tiles 0: the two-kernel layers), conv1 -> conv2 -> conv4 -> conv3 with PReLU(0.1) behind the first three
 * (Base_Model.forward :218-227), the edge head (:54-59) and one res x res image per graph (:84).  Same kernels, same results as the
 * entry points above called one by one; the steps are submitted from native code out of one workspace.
 *   d_edge_index int64[2][n_edges], the n_nodes self loops LAST (train_Teacher_Model.py:43-44); d_x float32[n_nodes] (in_dim 1);
 *   hidden = 32; params: HOST array of 20 device pointers (float32) = for conv1, conv2, conv4, conv3 in this order
 *   {lin_l.weight, att_l, lin_ij.weight, bias}, then lin5.weight, lin5.bias, lin6.weight, lin6.bias;
 *   d_edge_ptr int64[n_graphs+1]: offsets into the n_edges - n_nodes edges; d_points float32[n_edges - n_nodes][2] (the predicted
 *   diagram points); d_img float64[n_graphs][res*res]; d_work: tlc_pdgnn_forward_work_bytes(n_nodes, n_edges, hidden) bytes.
 * The call waits for the stream once (the tile count) unless the structure is handed in.
 * Both entry points take n_nodes >= 1, n_edges >= n_nodes, hidden > 0 (work_bytes returns -1 otherwise, the forward TLC_ERR_INVALID_ARG). */
int64_t tlc_pdgnn_forward_work_bytes(int32_t n_nodes, int64_t n_edges, int32_t hidden);
int tlc_pdgnn_forward(int32_t n_nodes, int64_t n_edges, const int64_t* d_edge_index, const float* d_x, int32_t hidden,
                      const float* const* params, int64_t n_graphs, const int64_t* d_edge_ptr, int32_t res,
                      const int32_t* d_rowptr, const int32_t* d_col, const int32_t* d_tile_ptr, int32_t n_tiles,
                      void* d_work, int64_t work_bytes, float* d_points, double* d_img, void* stream);


/* ---- the diagram loss of PDGNN training ------------------------------------------------------------
 * `wasserstein_distance(X, Y, order=p, internal_p=inf, enable_autodiff=True, num_models=1)` of
 * Knowledge_Distillation/wasserstein.py:198-379, as called by Teacher_model.py:131 (compute_PD_loss, kernel='wasserstein'),
 * for a batch of diagram pairs: problem b has predicted points X[xoff[b] .. xoff[b+1]) and target points Y[yoff[b] .. yoff[b+1]),
 * (birth, death) float64 pairs.  Every predicted point goes to a target point (each target takes exactly one) or to the diagonal;
 * cost = ||X_i - Y_j||_inf ^ p, resp. ((death - birth) / 2) ^ p (:45-67); the optimum is found by the Hungarian method on the
 * device, one wavefront per problem (the reference calls POT's ot.emd: third-party, parity unpinned -- the optimal cost is
 * unique, the choice among tied optima is not reproduced).
 *   d_loss[b] = (sum over the matched distances d_k of |d_k|^p)^(1/p)   (:303-372; order p = 1 or 2)
 *   d_wxy / d_wxd[b] = the same norm over the point-point pairs / the points sent to the diagonal (what the reference logs)
 *   d_assign[i] = problem-local target index of predicted point i, -1 = diagonal
 *   d_gradX[i] (may be null) = d loss[b] / d X_i: what `loss.backward()` leaves on the predicted diagram
 *   d_status[b]: 0 ok; 1 = fewer predicted than target points (the reference's transport has negative diagonal mass: no
 *   result, loss 0); 2 = more than 4 096 predicted points (not supported: loss 0); 3 = a NaN / Inf coordinate (loss NaN, zero
 *   gradient: the augmenting search cannot run on it).  Problems of up to 512 predicted points take one
 *   wavefront each, larger ones a 512-thread workgroup each (a second launch when max_points > 512).  max_points: an upper bound of the predicted
 *   points of one problem (selects the kernel variant). */
int tlc_w2_partial_matching(int32_t n_problems, const int64_t* d_xoff, const double* d_X, const int64_t* d_yoff,
                            const double* d_Y, int order, int32_t max_points, double* d_loss, double* d_wxy, double* d_wxd,
                            int32_t* d_assign, double* d_gradX, uint8_t* d_status, void* stream);

/* The evaluation form: `wasserstein_distance_inference(X, Y, order=p, internal_p=inf, enable_autodiff=True)` of
 * Knowledge_Distillation/wasserstein.py:93-195, reached with `pair_diagonal=True` (train_Teacher_Model.py:99 ->
 * Teacher_model.py:66 -> compute_PD_loss(type='inference') :134-136).  The classic transport in which BOTH diagrams may use the
 * diagonal (masses [1]*n + [m] against [1]*m + [n], (n+1) x (m+1) costs, C[n, j] = ((Y_j.death - Y_j.birth) / 2) ^ p,
 * C[n, m] = 0 :127-131) = the assignment of n + m rows onto n + m columns; same kernels as tlc_w2_partial_matching.
 *   d_loss[b] = (sum |d_k|^p)^(1/p) over point-point pairs, predicted points sent to the diagonal and target points sent to the
 *   diagonal (:140-181); d_wxy / d_wxd / d_wyd[b]: the same norm over each of the three groups (the reference's five return
 *   values are (loss, None, wxy, wxd, wyd)).  An empty diagram on either side: loss = total persistence of the other one and
 *   the three parts 0 (:98-113).
 *   d_assign_x[i] = target index of predicted point i or -1 = diagonal; d_assign_y[j] = predicted index of target j or -1.
 *   d_gradX (may be null): d loss[b] / d X_i.  d_status[b]: 0 ok; 2 = n + m > 4 096; 3 = non-finite coordinates (loss NaN).
 *   max_points: an upper bound of n + m of one problem.  Parity unpinned like tlc_w2_partial_matching (POT absent). */
int tlc_w2_inference_matching(int32_t n_problems, const int64_t* d_xoff, const double* d_X, const int64_t* d_yoff,
                              const double* d_Y, int order, int32_t max_points, double* d_loss, double* d_wxy, double* d_wxd,
                              double* d_wyd, int32_t* d_assign_x, int32_t* d_assign_y, double* d_gradX, uint8_t* d_status,
                              void* stream);

/* ---- The same two losses above 4 096 rows: the workspace tier (csrc/w2_large.hip) --------------------------------
 * infer = 0: the training form of tlc_w2_partial_matching (n predicted rows onto m targets and n - m copies of the diagonal, N = n);
 * infer = 1: the evaluation form of tlc_w2_inference_matching (N = n + m).  Cost, loss, the three partial sums, d_assign_x,
 * d_assign_y and d_gradX are what the two entries above specify; d_wyd and d_assign_y may be null when infer = 0.  The same
 * shortest-augmenting-path method, one workgroup of 1 024 threads per problem in flight, with the O(N) state (34 bytes per row) in
 * the caller's workspace instead of LDS, a dual-feasible start (u_i = min_j c_ij, v_j = min_i (c_ij - u_i), then the rows ascending
 * take their lowest free tight column) and one dual update per augmentation.
 *   min_rows: a problem with N <= min_rows is LEFT ALONE, none of its outputs is written.  A mixed batch is two calls: the entries
 *   above give the problems beyond their 4 096 rows status 2 and defined outputs, and this call with min_rows = 4096 overwrites
 *   exactly those.  min_rows = 0 takes every problem that has a row, -1 the problems without rows too.
 *   d_status[b]: 0 ok; 1 = n < m in the training form; 2 = N > TLC_W2_LARGE_NMAX; 3 = a NaN / Inf coordinate.  For 1 .. 3 the
 *   outputs are those of the entries above (loss 0, or NaN for status 3; no matching; zero gradient); the other problems of the batch
 *   are not affected.  Empty diagrams as above.
 *   d_work / work_bytes: 256-byte aligned, at least tlc_w2_large_work_bytes(N_max, 1) bytes, N_max = the rows of the largest problem
 *   this call solves (host arithmetic; -1 for a negative argument; linear in slots).  The workspace holds work_bytes / (the bytes of
 *   one slot) slots; the grid is min(slots, problems above min_rows) workgroups and a workgroup takes problems by that stride, so the
 *   least workspace runs them one after another.  A problem's bits depend on the problem alone: not on the batch, the slot, the
 *   workspace or the run.  Ties take the lowest column, but under tied costs the start may choose another optimal assignment than the
 *   entries above, and sums are ordered differently (loss equal to rounding, not to the bit).
 *   The entry reads the offsets back (one copy that waits for `stream`).  TLC_ERR_INVALID_ARG before any launch: order not 1 or 2,
 *   infer not 0 or 1, min_rows < -1, a null pointer, a misaligned or too small d_work, decreasing offsets.  The first
 *   TLC_W2_LARGE_COUNTERS int64 of every slot hold what its workgroup did in the call: steps, augmentations, rows the start assigned,
 *   problems (read by tools/time_w2_large.py).  No floating-point atomics; every loop is bounded by N. */
#define TLC_W2_LDS_NMAX        4096    /* the rows the two entries above take */
#define TLC_W2_LARGE_NMAX      65536
#define TLC_W2_LARGE_COUNTERS  4
int64_t tlc_w2_large_work_bytes(int64_t max_rows, int32_t slots);
int tlc_w2_large_matching(int32_t n_problems, const int64_t* d_xoff, const double* d_X, const int64_t* d_yoff, const double* d_Y,
                          int order, int infer, int32_t min_rows, double* d_loss, double* d_wxy, double* d_wxd, double* d_wyd,
                          int32_t* d_assign_x, int32_t* d_assign_y, double* d_gradX, uint8_t* d_status, void* d_work,
                          int64_t work_bytes, void* stream);

/* ---- The sliced Wasserstein diagram loss and its gradient (csrc/sliced_w.hip) ----------------------------------
 * `compute_PD_loss(kernel='sliced')` of Knowledge_Distillation/Teacher_model.py:110-124 (the distance of Carriere et al.), at any
 * diagram size.  The directions and the scale are INPUTS: the reference's angles are made by the caller (ops.sliced_directions).
 *
 * THE FUNCTION.  Problem b: diagrams X (n points) and Y (m points), fp64 (birth, death) rows in the packed layout of
 * tlc_w2_partial_matching; N = n + m.  c(p) = |b + d| * 0.5 is the coordinate of the diagonal projection of point p (= the
 * reference's sqrt(x**2 / 2) of x = (b + d) / sqrt 2, :111-115).  For direction l = (l0, l1):
 *     V1 = [ l0 * b + l1 * d  of X's points in order ]  then  [ (l0 + l1) * c(y)  of Y's points in order ]        (N elements)
 *     V2 = [ l0 * b + l1 * d  of Y's points in order ]  then  [ (l0 + l1) * c(x)  of X's points in order ]
 * in plain fp64 multiplies and adds (no FMA).  Both lists are sorted ascending by IEEE < (-0.0 equals +0.0); equal keys keep their
 * listing order (a stable sort).  loss[b] = sum over the directions i ascending, from +0.0, of  scale * r_i,  r_i = sum over the
 * ranks k of |sort(V1)_k - sort(V2)_k|.  The order inside a rank sum is fixed per size class and depends on the ranks alone:
 *     N <= TLC_SW_WAVE_NMAX:  the butterfly k ^ 1, k ^ 2, ... k ^ 32 over 64 ranks (absent ranks add +0.0);
 *     N <= TLC_SW_LDS_NMAX:   thread t of 256 adds its ranks t, t + 256, ... ascending; the butterfly inside each wavefront of 64
 *                             threads; the four wavefronts ascending;
 *     above:                  tiles of 1 024 ranks, each summed like the class before; the tiles ascending.
 * So loss(X, Y) and loss(Y, X) have the same bits.
 *
 * THE GRADIENT.  s_k = sign(sort(V1)_k - sort(V2)_k) in {-1, 0, 1}; sA[a] = the s at the rank that listing element a of V1
 * received, sB[c] the same for V2.  Per direction i:  t_ic = scale * l_ic,  u_i = scale * ((l_i0 + l_i1) * 0.5);  sigma_j =
 * sign(b_j + d_j) of X's point j (0 at 0), tau_j the same of Y's point j.  For point j of X and component c, from +0.0, over i
 * ascending:   g += sA_i[j] * t_ic;      g -= sB_i[m + j] * sigma_j * u_i.
 * For point j of Y:   g -= sB_i[j] * t_ic;      g += sA_i[n + j] * tau_j * u_i.
 * One owner sums a point in that order; there is no floating-point atomic: the bits of a problem depend on its own inputs alone --
 * not on the run, the batch around it or the workspace.  Under ties the loss is not differentiable and the stable order with
 * sign(0) = 0 is the convention.
 *
 * Size classes by N, cut on the device: up to TLC_SW_WAVE_NMAX one wavefront per problem (the sort across lanes); up to
 * TLC_SW_LDS_NMAX one workgroup per problem (both lists in LDS); above, the whole device, one problem after the other: the items of
 * as many directions as d_work holds (and directions x N <= 2^27) are radix-sorted together with the segment number
 * 2 * direction + list as the leading digit, sign bytes per (direction, listing position) go to d_work and one kernel sums each
 * point's directions ascending.
 *
 * d_dirs float64[n_dirs, 2], 1 <= n_dirs <= TLC_SW_MAX_DIRS.  d_loss float64[B].  d_gradX float64[sum n, 2] / d_gradY
 * float64[sum m, 2] (each may be NULL): every row of every problem is written.  d_status uint8[B]: 0 ok (n = 0 and / or m = 0 are
 * ordinary problems; both empty: loss +0.0); 3 = a NaN / Inf coordinate, decided before any sort: loss NaN, gradients zero (the
 * device-wide class does not skip its sorts for such a problem: their result is discarded).
 * max_points: an upper bound of one problem's N.  The entry reads the offsets back once and synchronises the stream before it
 * launches anything.
 * tlc_sliced_w_work_bytes (host arithmetic; total_points = sum of N): the d_work that runs all directions of the largest problem at
 * once; 0 (d_work may be NULL) when max_points <= TLC_SW_LDS_NMAX; -1 for a negative size or n_dirs out of range.  Any d_work of at
 * least the size reported for ONE direction gives the same bits (the directions then go in groups).
 * TLC_ERR_INVALID_ARG, nothing launched: negative sizes, null required pointers, n_dirs outside 1 .. TLC_SW_MAX_DIRS, a d_work below
 * the size for one direction of max_points, offsets that decrease or a problem above max_points.  TLC_ERR_UNSUPPORTED: a problem above
 * 2^27 points.  n_problems == 0: TLC_OK, nothing read. */
#define TLC_SW_WAVE_NMAX  64
#define TLC_SW_LDS_NMAX   2048
#define TLC_SW_MAX_DIRS   128
int64_t tlc_sliced_w_work_bytes(int32_t n_problems, int64_t total_points, int64_t max_points, int32_t n_dirs);
int tlc_sliced_wasserstein(int32_t n_problems, const int64_t* d_xoff, const double* d_X, const int64_t* d_yoff, const double* d_Y,
                           int32_t n_dirs, const double* d_dirs, double scale, int64_t max_points, double* d_loss, double* d_gradX,
                           double* d_gradY, uint8_t* d_status, void* d_work, int64_t work_bytes, void* stream);

/* ---- The bottleneck distance between diagrams, a witness matching and its gradient (csrc/bottleneck.hip) ----------
 * THE FUNCTION.  Problem b: diagrams X (n points) and Y (m points), fp64 (birth, death) rows in the packed layout of
 * tlc_w2_inference_matching; both may use the diagonal, N = n + m.  Rows 0 .. n-1 are X's points and rows n .. N-1 copies of the
 * diagonal; columns 0 .. m-1 are Y's points and columns m .. N-1 copies of the diagonal.  In plain fp64 subtract, abs, max and multiply
 * (no FMA, no power, no root):
 *     c(i, j) = max(|X_i.birth - Y_j.birth|, |X_i.death - Y_j.death|)     i < n,  j < m      (max(a, b) = a > b ? a : b)
 *     c(i, j) = |X_i.death - X_i.birth| * 0.5                             i < n,  j >= m
 *     c(i, j) = |Y_j.death - Y_j.birth| * 0.5                             i >= n, j < m
 *     c(i, j) = +0.0                                                      i >= n, j >= m
 *   d_dist[b] = the least t for which a perfect matching of the N x N problem uses only costs <= t: one entry of the matrix, exact.  An
 *   empty diagram on one side gives the largest diagonal cost of the other; both empty (N = 0) give +0.0.
 *
 * THE WITNESS.  d_assign_x[i] = the target of predicted point i or -1 = diagonal, d_assign_y[j] = the predicted point of target j or
 * -1, as tlc_w2_inference_matching writes them: inverse to each other, and the matching they describe (every point left out of a pair
 * goes to the diagonal) attains d_dist.  Under tied costs it is one of several; it depends on the problem alone.
 *   d_arg[b] = (i, j): the pair of that matching whose cost equals d_dist; -1 stands for the diagonal side.  Among several pairs of that
 *   cost the lowest predicted index i wins (a point of X sent to the diagonal counts under its own index; a matching has one pair per
 *   i), and a pair (-1, j) is taken only if no pair with a predicted point attains the value, then the one of the lowest j.  Pairs of
 *   two diagonal copies are never named.  N = 0: (-1, -1).
 *
 * THE GRADIENT.  d_gradX float64[sum n, 2] / d_gradY float64[sum m, 2] (each may be NULL): every row of every problem is written, and
 * only the rows d_arg names are non-zero.  With sign(0) = 0:
 *     (i, j):   e = X_i - Y_j.  |e.birth| >= |e.death| (birth wins an exact tie): gradX[i] = (sign(e.birth), 0), else (0, sign(e.death));
 *               gradY[j] = the negative of gradX[i].
 *     (i, -1):  gradX[i] = (-0.5, +0.5) * sign(X_i.death - X_i.birth).          (-1, j):  gradY[j] = (-0.5, +0.5) * sign(Y_j.death - Y_j.birth).
 * Where the maximum is attained by several pairs, or by both coordinates, d_B is not differentiable and this is a convention (one
 * subgradient), as elsewhere in `topo`.
 *
 * d_status uint8[B]: 0 ok; 2 = N > TLC_BN_NMAX: distance 0, no matching (-1 everywhere), d_arg (-1, -1), zero gradient; 3 = a NaN / Inf
 * coordinate: distance NaN, otherwise the same.  A bad problem never affects its neighbours.  Finite coordinates whose difference
 * overflows give +Inf costs, which compare like any other.
 * max_points: an upper bound of one problem's N.  The entry reads the offsets back once and synchronises the stream before it
 * launches anything.  TLC_ERR_INVALID_ARG, nothing launched: n_problems < 0, max_points < 0, a null required pointer (the offsets,
 * d_dist, d_arg, the two maps, d_status; d_X / d_Y where there are points), offsets that decrease or a problem above max_points.
 * n_problems == 0: TLC_OK, nothing read.
 *
 * Size classes by N alone: up to TLC_BN_WAVE_NMAX a wavefront per problem, up to TLC_BN_NMAX a workgroup per problem with the O(N)
 * state in LDS.  Costs are recomputed from the points, no matrix is stored; every loop is bounded by N; there are no floating-point
 * atomics; a problem's bits depend on the problem alone: not on the batch, the grid or the run. */
#define TLC_BN_WAVE_NMAX  512
#define TLC_BN_NMAX       4096
int tlc_bottleneck_matching(int32_t n_problems, const int64_t* d_xoff, const double* d_X, const int64_t* d_yoff, const double* d_Y,
                            int32_t max_points, double* d_dist, int32_t* d_arg /* [n_problems,2] */, int32_t* d_assign_x, int32_t* d_assign_y,
                            double* d_gradX, double* d_gradY, uint8_t* d_status, void* stream);

/* ---- The general persistence imager and its gradient (csrc/pi_general.hip) --------------------------------------
 * PersistenceImager.transform of Knowledge_Distillation/pimg.py:354-414 (= sg2dgm/PersistenceImager.pyx:352-403) for any grid, ramp
 * and Gaussian kernel; tlc_pi_raster stays the kernel of the one configuration the TLC-GNN pipeline uses.
 *
 * THE SPECIFICATION (host memory, one per call):
 *   res_b, res_p   1 .. TLC_PI_MAX_RES pixels along birth and persistence
 *   h_bpnts float64[res_b + 1], h_ppnts float64[res_p + 1]: the grid lines, strictly increasing -- the imager object's own arrays
 *                  (its linspace bits); no uniform step is assumed
 *   h_ramp  float64[4] = (low, high, start, end), end > start: weight low below start, high above end, the line between
 *   h_sigma float64[3] = (var_b, var_p, cov): positive definite, and |r| < 0.925 for r = cov / sqrt(var_b var_p)
 *   skew           nonzero: rows of d_pts are (birth, death) and x = death - birth; zero: rows are (birth, x)
 * THE FUNCTION.  Phi = the standard normal CDF, 0.5 erfc(-z / sqrt 2).  For point i with weight w_i (d_weights[i] where d_weights is
 * given -- it overrides the ramp --, else the ramp at x_i):
 *   cov == 0:  image[rb, rp] = sum_i w_i dPhi_b(i, rb) dPhi_p(i, rp),   dPhi_b(i, rb) = Phi((bpnts[rb + 1] - b_i) / sd_b) -
 *              Phi((bpnts[rb] - b_i) / sd_b), dPhi_p alike in x_i and sd_p (sd = sqrt var): equal or unequal variances;
 *   cov != 0:  image[rb, rp] = sum_i w_i (F_i(rb + 1, rp + 1) - F_i(rb, rp + 1) - F_i(rb + 1, rp) + F_i(rb, rp)), F_i the bivariate
 *              normal CDF about point i at a grid corner by the Drezner-Wesolowsky form (Gauss-Legendre over the correlation: 6, 12
 *              or 20 nodes for |r| < 0.3, < 0.75, beyond); the four corners are combined per point before the sum over the points.
 * d_out float64[B, res_b * res_p], row-major [birth_bin, pers_bin] in every case (the reference returns the transpose for a
 * non-isotropic sigma: DESIGN.md 6.8).  Empty diagrams give zero rows; a NaN coordinate makes its own diagram's image NaN.
 * SUMMATION ORDER of a pixel: a diagram's points in slices of 1 024; inside a slice the points ascending (cov == 0: on the f64 MFMA,
 * four at a time); the slices ascending.  No floating-point atomics: the bits of an image depend on its diagram and the
 * specification alone, not on the batch around it, the launch geometry, the workspace or the run.
 *
 * d_offs int64[B + 1] and h_offs, the same offsets in host memory (the entry reads nothing back); d_pts float64[n_pts, 2].
 * d_work: only diagrams above 1 024 points need it (their slices' partial images).  tlc_pi_image_work_bytes (host arithmetic)
 * returns the size that runs 32 diagrams of max_points per launch and stores in *least (may be NULL) the size for one; any d_work
 * of at least *least gives the same bits.  0: d_work may be NULL.  -1: a negative size or a resolution out of range.
 *
 * tlc_pi_image_vjp: grad_pts float64[n_pts, 2] = d (sum grad_img * image) / d pts, every row written, one wavefront per point, a
 * fixed order, no atomics.  The ramp's slope is (high - low) / (end - start) for start <= x <= end and 0 outside.
 *   TLC_PI_GRAD_WEIGHT  the reference's gradient (pimg.py:392,395 detach the CDF factors): through the weight only,
 *                       g = slope * sum_pixels grad_img * (the point's unweighted contribution); skew: d/d death = g,
 *                       d/d birth = -g; no skew: only the persistence column receives g.
 *   TLC_PI_GRAD_FULL    the true derivative, cov == 0 only: it adds the two terms through Phi (the normal densities at the grid
 *                       lines in place of one of the CDF differences), chained through x = death - birth under the skew.
 * Explicit weights have no gradient entry (they are constants of the caller).
 * TLC_ERR_INVALID_ARG, nothing launched: a resolution outside 1 .. TLC_PI_MAX_RES, grid lines not finite or not strictly increasing,
 * end <= start, a non-finite ramp or sigma, a singular or non-positive-definite sigma, |r| >= 0.925 (the reference's branch for it is
 * wrong: DESIGN.md 6.8), TLC_PI_GRAD_FULL with cov != 0, an unknown mode, null required pointers, negative sizes, offsets that
 * decrease or leave 0 .. n_pts, a d_work below *least.  The message of tlc_last_error says which. */
#define TLC_PI_MAX_RES      128
#define TLC_PI_GRAD_WEIGHT  0
#define TLC_PI_GRAD_FULL    1
int64_t tlc_pi_image_work_bytes(int32_t n_dgms, int64_t max_points, int32_t res_b, int32_t res_p, int64_t* least);
int tlc_pi_image(int32_t n_dgms, int64_t n_pts, const int64_t* d_offs, const int64_t* h_offs, const double* d_pts,
                 const double* d_weights, int32_t res_b, int32_t res_p, const double* h_bpnts, const double* h_ppnts,
                 const double* h_ramp, const double* h_sigma, int32_t skew, double* d_out, void* d_work, int64_t work_bytes,
                 void* stream);
int tlc_pi_image_vjp(int32_t n_dgms, int64_t n_pts, const int64_t* d_offs, const double* d_pts, int32_t res_b, int32_t res_p,
                     const double* h_bpnts, const double* h_ppnts, const double* h_ramp, const double* h_sigma, int32_t skew,
                     int32_t mode, const double* d_grad_img, double* d_grad_pts, void* stream);

/* ---- Persistence landscapes of packed diagrams and their gradient (csrc/landscape.hip) ---------------------------
 * The landscape of Bubenik: the top K of the points' tent functions on a grid of sample values (PersLay's triangle layer under a
 * top-k pooling).  No smoothing parameter; the samples are INPUTS (a linspace is the caller's business).
 *
 * THE FUNCTION.  Diagram b: n points (birth_i, death_i), fp64 rows in the packed layout of tlc_sliced_wasserstein (d_offs
 * int64[B + 1]).  d_ts float64[T], any finite values, 1 <= T <= TLC_LS_TMAX; 1 <= K <= TLC_LS_KMAX.  In plain fp64:
 *     v_i(t) = min(t - birth_i, death_i - t)                                          (min(a, b) = a < b ? a : b)
 *   Point i is present at t iff v_i(t) > 0: a point with death <= birth is never present.  The present points are ordered by
 *   (v descending, i ascending), a strict total order.  d_out[b, k, j] is the v of the k-th point of that order at t_j (k = 0 .. K-1)
 *   and d_winner[b, k, j] its index, local to the diagram; with fewer than k + 1 points present the value is +0.0 and the winner -1.
 *   d_out float64[B, K, T], d_winner int32[B, K, T] (may be NULL): every cell of every diagram is written.
 *   Every value is one subtraction and one min of the inputs, and the K best under a strict total order do not depend on how the
 *   points are divided: the bits of a diagram depend on its own points, the samples and K alone -- not on the run, the batch around
 *   it or the workspace.
 * d_status uint8[B]: 0 ok (n = 0 is an ordinary diagram of zero rows); 3 = a NaN / Inf coordinate in the diagram: its values NaN, its
 *   winners -1, and so its gradient zero; its neighbours are untouched.
 *
 * THE GRADIENT (tlc_landscape_vjp).  d_grad_pts float64[sum n, 2], every row written.  A cell (k, j) with winner i and upstream g =
 *   d_grad_out[b, k, j] contributes (-g, 0) to point i when  t_j - birth_i <= death_i - t_j  (the birth side wins the exact tie at the
 *   peak), else (0, +g).  A point's contributions are added from +0.0 over the cells in ascending (k, j); one owner sums a point and
 *   there is no floating-point atomic.  The side is recomputed from the points; d_winner is the forward's output (an index outside
 *   0 .. n-1 names nobody).  Points that win nothing get zero rows.  Under ties (duplicate points, a sample on a peak) the landscape is
 *   not differentiable and this convention is the subgradient.
 *
 * Size classes by n, cut on the device: up to TLC_LS_WAVE_NMAX one wavefront per diagram (the points broadcast from its lanes); up
 * to TLC_LS_LDS_NMAX one workgroup per diagram and block of 256 samples (the points in LDS); above, the whole device, one diagram
 * after the other: slices of TLC_LS_LDS_NMAX points write their K-lists to d_work and a second kernel merges a cell's lists, the
 * slices ascending.  No cap below 2^27 points.
 * max_points: an upper bound of one diagram's n.  Both entries read the offsets and the samples back once and synchronise the
 * stream before they launch anything.
 * tlc_landscape_work_bytes (host arithmetic): the d_work that runs the slices of the largest diagram in the fewest launches; 0 (d_work
 * may be NULL) when max_points <= TLC_LS_LDS_NMAX; -1 for a negative size or K / T out of range.  *least (may be NULL): the size that
 * runs one slice at a time; any d_work of at least *least gives the same bits.
 * TLC_ERR_INVALID_ARG, nothing launched: negative sizes, K or T out of range, null required pointers, a NaN / Inf sample, offsets
 * that decrease or a diagram above max_points, a d_work below *least.  TLC_ERR_UNSUPPORTED: a diagram above 2^27 points.
 * n_dgms == 0: TLC_OK, nothing read. */
#define TLC_LS_WAVE_NMAX  64
#define TLC_LS_LDS_NMAX   4096
#define TLC_LS_KMAX       16
#define TLC_LS_TMAX       4096
int64_t tlc_landscape_work_bytes(int32_t n_dgms, int64_t max_points, int32_t K, int32_t T, int64_t* least);
int tlc_landscape(int32_t n_dgms, const int64_t* d_offs, const double* d_pts, int32_t T, const double* d_ts, int32_t K,
                  int64_t max_points, double* d_out, int32_t* d_winner, uint8_t* d_status, void* d_work, int64_t work_bytes,
                  void* stream);
int tlc_landscape_vjp(int32_t n_dgms, const int64_t* d_offs, const double* d_pts, int32_t T, const double* d_ts, int32_t K,
                      int64_t max_points, const int32_t* d_winner, const double* d_grad_out, double* d_grad_pts, void* stream);

/* ---- Gram matrices of persistence diagram kernels and their gradient (csrc/dgm_gram.hip) --------------------------
 * The persistence scale-space kernel (Reininghaus et al. 2015) and the persistence weighted Gaussian kernel (Kusano et al. 2016)
 * between packed diagrams: every diagram of X against every diagram of Y (TLC_DG_ALL) or diagram i against diagram i (TLC_DG_PAIRED).
 *
 * THE FUNCTION.  X: nx diagrams, x_offs int64[nx + 1], x_pts float64[sum n, 2] rows (birth, death), x_w float64[sum n] or NULL (every
 * weight 1); Y likewise.  gamma > 0, scale finite; mirror = 1 with TLC_DG_MIRROR, else 0.  For p in X_i and q in Y_j:
 *     e1(p, q) = exp(-gamma * ((p.b - q.b)^2 + (p.d - q.d)^2))        e2(p, q) = exp(-gamma * ((p.b - q.d)^2 + (p.d - q.b)^2))
 *     k(X_i, Y_j) = scale * sum_p sum_q w_p w_q (e1 - mirror * e2)
 *   PSS with bandwidth sigma: gamma = 1 / (8 sigma), scale = 1 / (8 pi sigma), TLC_DG_MIRROR, no weights.  PWG: gamma = 1 / (2 s^2),
 *   scale = 1, no mirror, w = arctan(C * pers^p) made by the caller.
 * d_out float64[nx, ny] (ALL) or float64[nx] (PAIRED, nx == ny).  TLC_DG_SYMMETRIC (ALL only, Y the same buffers as X): only j >= i
 *   is computed and stored to [i, j] and [j, i]; the upper triangle and the diagonal equal the general call on a copy of X bit for bit.
 * A pair with an empty diagram gives +0.0.
 * d_status_x uint8[nx], d_status_y uint8[ny] (written by tlc_dgm_gram): 0 ok, 3 = a NaN / Inf coordinate or weight in that diagram:
 *   its row (column) of d_out is NaN, its gradient rows are zero, and no other entry changes.
 *
 * THE ORDER, operation by operation (fp64, round to nearest, no fused multiply-add, exp = the device library's).  ng = -gamma.
 *   One summand t(p, q):  db = p.b - q.b;  dd = p.d - q.d;  e = exp(ng * (db * db + dd * dd));  with the mirror:  xb = p.b - q.d;
 *     xd = p.d - q.b;  e = e - exp(ng * (xb * xb + xd * xd));  with weights:  t = (w_p * w_q) * e;  without:  t = e.
 *   X_i (n points) is cut into max(1, ceil(n / TLC_DG_SLICE)) slices of TLC_DG_SLICE points and Y_j (m points) into
 *     max(1, ceil(m / TLC_DG_GROUP)) groups of TLC_DG_GROUP points, a group into chunks of 64 points, all from the diagram's own start.
 *   Unit (slice s, group g):  P = +0.0;  for the group's chunks ascending:  for l = 0 .. 63:  a[l] = +0.0, and if point q = chunk
 *     start + l exists, for p of the slice ascending:  a[l] = a[l] + t(p, q);  FOLD:  for d = 32, 16, 8, 4, 2, 1:  for every l < d at
 *     once:  a[l] = a[l] + a[l + d];  P = P + a[0].
 *   R = +0.0;  for s ascending:  for g ascending:  R = R + P(s, g).  d_out = scale * R  (an empty diagram: +0.0; status 3: NaN).
 *   The order is a function of (n, m) alone: d_out[i, j] is the same bits alone, in any batch, in ALL or PAIRED mode, with any
 *   workspace from *least up, and from run to run.  No floating-point atomics.
 *
 * THE GRADIENT IN THE FIRST ARGUMENT (tlc_dgm_gram_vjp).  d_grad_out float64[nx, ny] or [nx]; d_grad_pts_x float64[sum n, 2] and,
 * exactly when x_w is given, d_grad_w_x float64[sum n]: every row written.  d_status_x / d_status_y are INPUTS here, the forward's.
 *   For point p of X_i, one owner (a lane):  gb = gd = gw = +0.0;  for j ascending (PAIRED: j = i only), skipping status 3:
 *     ib = id = iw = +0.0;  for q of Y_j ascending:  db, dd as above;  t1 = w_q * exp(ng * (db * db + dd * dd))  (no weights: the exp);
 *       without the mirror:  ib = ib - db * t1;  id = id - dd * t1;  iw = iw + t1;
 *       with it:  xb, xd as above;  t2 = w_q * exp(ng * (xb * xb + xd * xd));  ib = ib + (xb * t2 - db * t1);
 *                 id = id + (xd * t2 - dd * t1);  iw = iw + (t1 - t2).
 *     G = d_grad_out[i, j];  gb = gb + G * ib;  gd = gd + G * id;  gw = gw + G * iw.
 *   c = scale * w_p (no weights: scale);  grad_pts = ((c * (2 * gamma)) * gb, (c * (2 * gamma)) * gd);  grad_w = scale * gw.
 *   A diagram of X with status 3 gets zero rows.  The order for a row is a function of the sizes of Y's diagrams alone.  The gradient
 *   in the second argument is this entry with the roles swapped and d_grad_out transposed (|p - q~| = |q - p~|); for Y = X the caller
 *   passes G + G^T (PAIRED: 2 G).  TLC_DG_SYMMETRIC is accepted and changes nothing here.
 *
 * max_nx_points / max_ny_points: upper bounds of one diagram's points.  Both entries read the offsets back once and synchronise the
 * stream before they launch anything; an entry that uses its prefix arrays (below) uploads them in one copy and synchronises once more.
 * tlc_dgm_gram_work_bytes (host arithmetic, one size for both entries): the d_work that runs every diagram pair in one launch, at most
 * 1 GiB of partials; 0 when max_nx_points <= 64 and max_ny_points <= TLC_DG_GROUP; -1 for a negative size, any flag word the entries
 * refuse, or a size beyond int64.  *least (may be NULL): the size that runs the pairs of one X diagram at a time.  An entry asks for
 * d_work only where it uses it: tlc_dgm_gram when a pair can have more than one unit (max_nx_points > TLC_DG_SLICE or max_ny_points >
 * TLC_DG_GROUP), tlc_dgm_gram_vjp for its chunk prefix (PAIRED with max_nx_points > 64); otherwise d_work may be NULL.
 * TLC_ERR_INVALID_ARG, nothing launched and nothing written: null required pointers, negative sizes, gamma not finite or not > 0,
 * scale not finite, unknown flag bits, not exactly one of ALL / PAIRED, PAIRED with nx != ny, SYMMETRIC without ALL, with different
 * X and Y buffers or with nx != ny or max_nx_points != max_ny_points, offsets that are negative or decrease, a diagram above its
 * max_*_points, a d_work the entry uses below *least, tlc_dgm_gram_vjp with exactly one of x_w and d_grad_w_x.
 * nx == 0 or ny == 0: TLC_OK (the VJP with ny == 0 writes zero rows). */
#define TLC_DG_ALL        0x1u
#define TLC_DG_PAIRED     0x2u
#define TLC_DG_SYMMETRIC  0x4u
#define TLC_DG_MIRROR     0x8u
#define TLC_DG_SLICE      1024   /* points of a slice of the first argument */
#define TLC_DG_GROUP      1024   /* points of a group of the second argument: 16 chunks of 64 */
int64_t tlc_dgm_gram_work_bytes(int32_t nx, int32_t ny, int64_t max_nx_points, int64_t max_ny_points, uint32_t flags, int64_t* least);
int tlc_dgm_gram(int32_t nx, const int64_t* x_offs, const double* x_pts, const double* x_w, int32_t ny, const int64_t* y_offs,
                 const double* y_pts, const double* y_w, double gamma, double scale, uint32_t flags, int64_t max_nx_points,
                 int64_t max_ny_points, double* d_out, uint8_t* d_status_x, uint8_t* d_status_y, void* d_work, int64_t work_bytes,
                 void* stream);
int tlc_dgm_gram_vjp(int32_t nx, const int64_t* x_offs, const double* x_pts, const double* x_w, int32_t ny, const int64_t* y_offs,
                     const double* y_pts, const double* y_w, double gamma, double scale, uint32_t flags, int64_t max_nx_points,
                     int64_t max_ny_points, const uint8_t* d_status_x, const uint8_t* d_status_y, const double* d_grad_out,
                     double* d_grad_pts_x, double* d_grad_w_x, void* d_work, int64_t work_bytes, void* stream);

/* ---- what `loss.backward()` runs through the PDGNN layer and the edge head ---------------------------
 * (Knowledge_Distillation/train_Teacher_Model.py:55-62 through gat_conv.py:113-216 and Teacher_model.py:53-59.)
 * tlc_gat_layer_bwd: gradients of one layer, same operands as tlc_gat_layer_fwd.  Nothing of the forward is kept: the node rows,
 * the row softmax and the channel-wise minima / maxima are recomputed (one wavefront per target row).  A tied minimum / maximum
 * sends its gradient to the first edge of the row that attains it.
 *   d_out  float32[n, 2*c_out]: the forward's output, read only when prelu_slope >= 0 (sign of the pre-activation); else may be NULL
 *   d_gout float32[n, 2*c_out]: d loss / d out
 *   d_gX   float32[n, c_in] or NULL (first layer);  d_gWl [c_out, c_in], d_gatt [c_out], d_gWij [c_out, 2*c_out], d_gbias [2*c_out]:
 *   OVERWRITTEN.   d_work float32[tlc_gat_layer_bwd_work_floats(n, c_in, c_out)] scratch.   c_out in {8,16,32,64}, c_in <= 64.
 * Float atomics towards the sources of the edges and in the weight reductions: the summation order is not fixed. */
int64_t tlc_gat_layer_bwd_work_floats(int32_t n_nodes, int32_t c_in, int32_t c_out);
int tlc_gat_layer_bwd(int32_t n_nodes, const int32_t* d_rowptr, const int32_t* d_src, const float* d_X, int32_t c_in,
                      int32_t c_out, const float* d_Wl, const float* d_att, const float* d_Wij, float prelu_slope,
                      const float* d_out, const float* d_gout, float* d_gX, float* d_gWl, float* d_gatt, float* d_gWij,
                      float* d_gbias, float* d_work, void* stream);

/* tlc_edge_head_bwd: gradients of tlc_edge_head_fwd.  d_gpd float32[n_edges, 2] = d loss / d pd.
 *   d_gX float32[n_nodes, c] is ADDED to (the caller zeroes it); d_gW5 [hidden, 2c], d_gb5 [hidden], d_gW6 [2, hidden], d_gb6 [2]:
 *   OVERWRITTEN.   d_work float32[tlc_edge_head_bwd_work_floats(n_edges, c, hidden)] scratch.   hidden in {16,32,64}. */
int64_t tlc_edge_head_bwd_work_floats(int64_t n_edges, int32_t c, int32_t hidden);
int tlc_edge_head_bwd(int64_t n_edges, const int32_t* d_src, const int32_t* d_dst, const float* d_X, int32_t c,
                      const float* d_W5, const float* d_b5, int32_t hidden, float prelu_slope, const float* d_W6,
                      const float* d_gpd, float* d_gX, float* d_gW5, float* d_gb5, float* d_gW6, float* d_gb6,
                      float* d_work, void* stream);

/* MessagePassing.aggregate (Knowledge_Distillation/message_passing.py:275-293): torch_scatter.scatter(inputs, index, dim=0,
 * dim_size=n_out, reduce) with reduce 0 = sum, 1 = mean, 2 = min, 3 = max; empty segments give 0, as torch_scatter does.
 *   d_index int64[n_src]; d_src float32[n_src,k]; d_out float32[n_out,k]; d_count_work int32[n_out] (not needed for sum).
 * Float atomics: the summation order is not fixed (same as the reference's scatter kernels). */
int tlc_scatter_f32(int64_t n_src, const int64_t* d_index, const float* d_src, int32_t k, int reduce, int32_t n_out,
                    float* d_out, int32_t* d_count_work, void* stream);

/* Edge head of Teacher_Model.forward (Teacher_model.py:54-59): for every non-self-loop edge e=(s,t):
 *   pd[e] = W6 @ prelu(W5 @ [x[s] || x[t]] + b5) + b6   -> float32[n_edges,2]
 * d_work (optional, float32[tlc_edge_head_fwd_work_floats(n_nodes, c, hidden)]): with it the first layer is computed per node on the
 * MFMA GEMM (W5[:, :c] x_s + W5[:, c:] x_t) and only gathered per edge; NULL: one 2c x hidden product per edge. */
int64_t tlc_edge_head_fwd_work_floats(int32_t n_nodes, int32_t c, int32_t hidden);
int tlc_edge_head_fwd(int64_t n_edges, const int32_t* d_src, const int32_t* d_dst, const float* d_X,
                      int32_t c, const float* d_W5, const float* d_b5, int32_t hidden, float prelu_slope,
                      const float* d_W6, const float* d_b6, float* d_pd, int32_t n_nodes, float* d_work, void* stream);

/* ---- the callers' side of the path: negative enumeration and the image cache ----------
 *
 * loaddatas.py:44-45 lists the non-edges as `sp.triu(sp.csr_matrix(1. - adj.toarray())).nonzero()` (a dense N x N float64
 * matrix), shuffles the [n_neg, 2] array and slices it (:46,:51-53).  Pair number r of that list -- row-major over x <= y with
 * adj[x,y] == 0, the diagonal included -- is a function of the CSR alone:
 *
 * tlc_complement_rows: d_row_start int64[n_nodes+1] = exclusive prefix of the per-row non-edge counts (d_row_start[n_nodes] =
 *   n_neg).  The CSR must be the symmetric adjacency with columns ascending and unique inside a row (a stored entry is an
 *   edge, whatever its weight -- the reference's matrices are 0/1).
 * tlc_complement_pairs: d_pairs int32[count,2] = the pairs with list numbers d_ranks[0..count) (int64; e.g. a slice of the
 *   shuffled index list), or first, first+1, ... when d_ranks is NULL.  A number outside [0, n_neg) yields (-1, -1). */
int tlc_complement_rows(int32_t n_nodes, const int32_t* d_rowptr, const int32_t* d_col, int64_t* d_row_start, void* stream);
int tlc_complement_pairs(int32_t n_nodes, const int32_t* d_rowptr, const int32_t* d_col, const int64_t* d_row_start,
                         const int64_t* d_ranks, int64_t first, int64_t count, int32_t* d_pairs, void* stream);

/* The distance <= hop pre-filter of the sweep (PI-C): an image row can be non-zero only when d(u,v) <= hop
 * (SURVEY.md A.6, Z0), so only those non-edges need tlc_pd_pi_batch.  Appends every non-adjacent pair u <= v with d(u,v) <= hop
 * (the diagonal included unless u has a self loop): d_out_pairs int32[k,2] and d_out_rank int64[k] = the pair's number in the
 * list of tlc_complement_pairs.  *d_count (uint64, device, zeroed by the caller) is advanced even beyond `cap` (pairs past the
 * capacity are not written).  Append order is not fixed.  Graphs up to ~400 000 nodes (three LDS bitmaps per wavefront);
 * beyond that TLC_ERR_UNSUPPORTED (the full sweep does not have the limit). */
int tlc_near_pairs(int32_t n_nodes, const int32_t* d_rowptr, const int32_t* d_col, const int64_t* d_row_start, int hop, int64_t cap,
                   uint64_t* d_count, int64_t* d_out_rank, int32_t* d_out_pairs, void* stream);

/* The reference caches the dense float64[n_pairs, res^2] image array (loaddatas.py:62-64,102: 39 GB for PubMed's sweep) although
 * every pair with d(u,v) > hop has a zero row, and keeps of the exceptions it swallows only their number (`cnt_compute`,
 * riccidist2dgm.py:355).  tlc_select_rows appends the rows of one image block that have a non-zero entry -- with
 * TLC_SELECT_KEEP_FAILED also the zero rows whose status is not TLC_ST_OK -- to a sparse store: d_out_idx[k] = index_base + row
 * number, d_out_status[k] (may be NULL), d_out_rows[k, width]; and adds the block's status bytes to the histogram
 * d_status_hist uint64[8] (may be NULL; the caller zeroes it once per store).  *d_count (uint64, device; the caller zeroes it
 * per call) is advanced by the number of kept rows even beyond `cap` (rows past the capacity are not written: re-run the block
 * with a larger store, and a fresh histogram).  Append order is not fixed. */
/* |S| and the number of induced edges of every pair's vicinity, nothing else (the extraction of tlc_vicinity_filtration without the
 * filtration): d_n / d_m int32[n_pairs], n = 0 for a pair without a vicinity; same hop / flags as the tlc_vicinity_filtration call
 * that follows.  With tlc_pack_offsets a caller gets exact offsets from them: no per-pair capacity to guess (replaces the sizing
 * the reference does implicitly by building Python lists, data_utils_LP.py:107-125). */
int tlc_vicinity_sizes(tlc_graph* g, const int32_t* d_pairs, int64_t n_pairs, int hop, uint32_t flags, int32_t* d_n, int32_t* d_m,
                       void* stream);
/* The offsets of that packed batch from the per-pair counts of tlc_vicinity_filtration, one launch: d_node_ptr / d_edge_ptr int64[n_pairs+1]
 * = exclusive prefix sums of (m > 0 ? n : 0) and max(m, 0) -- a vicinity without an edge is left out, the reference returns (None, None)
 * for it (data_utils_LP.py:117-118) -- and d_totals int64[4] = {min n, min m, sum n, sum m} (a negative minimum: some vicinity did not
 * fit the capacity it was given). */
int tlc_pack_offsets(int64_t n_pairs, const int32_t* d_n, const int32_t* d_m, int64_t* d_node_ptr, int64_t* d_edge_ptr,
                     int64_t* d_totals, void* stream);
/* The caller side of the PDGNN fork's vicinity extraction (Knowledge_Distillation/data_utils_LP.py:105-200 returns one
 * (filtration values, edge_index) per candidate edge; gcn_LP_GIN.Net.compute_PI :43-64 feeds them to the model one by one): the
 * per-pair capacity slots tlc_vicinity_filtration wrote -> ONE packed block-diagonal batch.  d_node_ptr / d_edge_ptr int64[n+1]:
 * the packed offsets (exclusive prefix sums of the node and edge counts the caller wants kept -- a pair's slice may be empty);
 * d_out_ids int64 = d_label[id] (NULL: the id itself), d_out_f, d_out_edges int32[.,2] (local ids, as written), and the owner
 * pair of every packed node / edge (either may be NULL).  One wavefront per pair, coalesced both ways. */
int tlc_pack_vicinities(int64_t n_pairs, const int64_t* d_node_offs, const int32_t* d_ids, const double* d_f,
                        const int64_t* d_edge_offs, const int32_t* d_edges, const int64_t* d_node_ptr, const int64_t* d_edge_ptr,
                        const int64_t* d_label, int64_t* d_out_ids, double* d_out_f, int32_t* d_out_edges,
                        int64_t* d_pair_of_node, int64_t* d_pair_of_edge, void* stream);

/* The packed batch -> the operands Teacher_Model.forward takes, one launch: what gcn_LP_GIN.py:43-64 builds per vicinity (its
 * edge_index plus self loops, the filtration as a float32 column), for the block-diagonal batch as a whole.  d_edge_index
 * int64[2][tot_m + tot_n]: global ids = local id + d_node_ptr[owner], the tot_n self loops LAST (train_Teacher_Model.py:43-44);
 * d_x float32[tot_n] = (float)d_f (both may be NULL).  d_node_ptr / d_edge_ptr int64[n_graphs + 1] with totals tot_n / tot_m. */
int tlc_stack_batch(int64_t n_graphs, const int64_t* d_node_ptr, const int64_t* d_edge_ptr, const int32_t* d_edges, const double* d_f,
                    int64_t tot_n, int64_t tot_m, int64_t* d_edge_index, float* d_x, void* stream);

#define TLC_SELECT_KEEP_FAILED 0x1u
int tlc_select_rows(int64_t n_rows, int32_t width, const double* d_pi, const uint8_t* d_status, int64_t index_base, int64_t cap,
                    uint32_t flags, uint64_t* d_count, uint64_t* d_status_hist, int64_t* d_out_idx, uint8_t* d_out_status,
                    double* d_out_rows, void* stream);

/* ---- the producer of the path's edge weights -------------------------------------------------------
 * compute_ricci_curvature (loaddatas.py:105-123) = third-party GraphRicciCurvature `OllivierRicci(G, alpha=0.5,
 * method="Sinkhorn")` (not in the reference tree, version not pinned; restated from the published algorithm -- parity unpinned):
 * per edge (s,t), m_s = alpha at s + (1-alpha)/deg on the neighbours, cost = hop distance, W = <P, d> of POT's
 * `sinkhorn2(x, y, d, reg)` (sinkhorn_knopp: stop when the marginal violation <= stop_thr, tested every 10th iteration, or after
 * max_iter iterations), kappa = 1 - W.  The library's call is (alpha 0.5, reg 0.1, max_iter 1000, stop_thr 1e-9).
 *   CSR: symmetric, no self loops, columns ascending and unique inside a row, unit weights.  d_edges int32[n_edges,2]: adjacent
 *   pairs (a self pair gets curvature 0).  d_kappa double[n_edges]; d_iters int32[n_edges] (may be NULL): iterations used.
 *   d_work/work_bytes: >= 16 + 4*n_edges (rounded up to 16) + k * max_product/4 bytes (rounded up to 16), k >= 1 slots for the
 *   hub edges (2-bit hop codes of supports beyond the LDS); max_support >= max over edges of deg(s)+deg(t)+2 and max_product >= max of (deg(s)+1)*(deg(t)+1) over the edges
 *   with more than 8 192 entries or deg(s)+deg(t)+2 > 256 (those the one-wavefront kernel leaves to the workgroup kernel).  An edge that exceeds them gets NaN (and iters -1), never a silent value. */
int tlc_ollivier_ricci_sinkhorn(int32_t n_nodes, const int32_t* d_rowptr, const int32_t* d_col, int64_t n_edges,
                                const int32_t* d_edges, double alpha, double reg, int32_t max_iter, double stop_thr,
                                double* d_kappa, int32_t* d_iters, void* d_work, int64_t work_bytes, int32_t max_support,
                                int64_t max_product, void* stream);

/* The same curvature with the EXACT transport distance: `OllivierRicci(G, alpha, method="OTD")` (POT's emd2), which the reference's
 * node-classification pipeline uses for its curvature files (pipelines_GIN.py:79).  Integer throughout: with alpha = alpha_num /
 * alpha_den and D = alpha_den * deg(s) * deg(t) the scaled masses are alpha_num * deg(s) * deg(t) at s and (alpha_den - alpha_num) *
 * deg(t) on each neighbour of s (t likewise), the costs are the hop distances 0..3, W = the integer minimum cost of that
 * transportation problem (primal-dual, level-synchronous searches; every loop bounded by the sizes), and kappa = 1.0 - (double)W /
 * (double)D -- the only floating-point operations.  Bit-identical from run to run, independent of the batch, symmetric in (s, t).
 * Not reproduced: the library's nbr_topk cut of neighbourhoods above 3 000, weighted graphs, directed graphs.
 *   CSR and d_edges: as for tlc_ollivier_ricci_sinkhorn (symmetric, loop-free, columns ascending and unique, adjacent pairs only; a
 *   self pair gets kappa 0, W 0, D 0).  d_kappa double[n_edges]; d_cost / d_denom int64[n_edges] (either may be NULL): W and D.
 *   One wavefront solves an edge with (deg(s)+1)*(deg(t)+1) <= TLC_OTD_WAVE_PRODUCT, deg(s)+deg(t)+2 <= TLC_OTD_WAVE_SUPPORT and
 *   D <= TLC_OTD_WAVE_DENOM in LDS; the others take one workgroup each and a slot of the workspace (2-bit codes when they do not
 *   fit the LDS, and the flow cells: 4 bytes each, 8 when max_support >= 4 094).  max_support >= max over all edges of
 *   deg(s)+deg(t)+2, at most TLC_OTD_MAX_SUPPORT; max_product >= max of (deg(s)+1)*(deg(t)+1) over the edges of the second kind (>= 1).
 *   An edge beyond them, or one whose solve ran out of its bound, gets NaN and W = -1, never a silent value.
 *   d_work: 16-byte aligned, >= 16 + 4*n_edges (rounded up to 16) + one slot; tlc_ollivier_ricci_otd_work_bytes() gives the size with
 *   min(n_edges, 32) slots (more bytes = more hub edges in flight, up to 1 024).  Stream-ordered, no host synchronisation. */
#define TLC_OTD_WAVE_PRODUCT   8192
#define TLC_OTD_WAVE_SUPPORT   256
#define TLC_OTD_WAVE_DENOM     65535
#define TLC_OTD_MAX_SUPPORT    12794   /* 12 bytes of LDS per support entry + 64 within 150 KiB */
#define TLC_OTD_LDS_BYTES      153600  /* of which the hub kernel's codes get what 12 * max_support (rounded up to 16) + 32 leave */
int tlc_ollivier_ricci_otd_work_bytes(int64_t n_edges, int32_t max_support, int64_t max_product, int64_t* bytes);
int tlc_ollivier_ricci_otd(int32_t n_nodes, const int32_t* d_rowptr, const int32_t* d_col, int64_t n_edges, const int32_t* d_edges,
                           int32_t alpha_num, int32_t alpha_den, double* d_kappa, int64_t* d_cost, int64_t* d_denom, void* d_work,
                           int64_t work_bytes, int32_t max_support, int64_t max_product, void* stream);

/* ---- The distance filtration of a packed batch, and its vector-Jacobian product in the edge weights (csrc/dist_filt.hip, DESIGN.md
 * 6.10): filtration.build_fv (sg2dgm/riccidist2dgm.py:20-56) and ricci_filtration.build_fv (Knowledge_Distillation/data_utils_NC.py:34-55,
 * data_utils_LP.py:35-65) on graphs the caller packs, without a graph handle, a pair list or a size cap.
 * Input: the packed batch of tlc_struct_batch (d_node_ptr / d_edge_ptr int64[n_graphs + 1], d_edges int32[total_edges, 2] local ids, every
 * undirected edge ONCE), d_w float64[total_edges] (kappa + 1 of the edge), d_roots int32[n_graphs, 2] local ids; roots[g, 1] == -1: one
 * root (and TLC_DESC_ROOT1: the first root alone for every graph); equal roots are allowed.
 * Value, bit for bit the reference's: D_r[x] = the minimum over the paths x -> r of the left-to-right fp64 sum of the weights that
 * starts at x, 100 where r cannot be reached (TLC_UNREACHABLE_100; without the flag a graph with a node that root 0 does not reach is
 * TLC_ST_DISCONNECTED, as in tlc_vicinity_filtration); q[x] = 0 at a root, else D_0 + D_1 / min / max by TLC_DESC_*, D_0 for one root;
 * f = q / max q ('min': / max_x max(D_0, D_1), the roots counting as 0), TLC_NORM_EPS: / (that maximum + 1e-10), TLC_NO_NORM: f = q.
 * TLC_INCLUDE_ROOTS is accepted and changes nothing: it adds the roots to an EXTRACTED vicinity, and a packed graph holds its roots.
 * d_f float64[total_nodes].  d_status uint8[n_graphs]: TLC_ST_OK; TLC_ST_BAD_INPUT (the contract of tlc_struct_batch on offsets, ids,
 * loops and repeated pairs; a weight that is not finite and > 0; a root outside 0 .. n-1); TLC_ST_DISCONNECTED; TLC_ST_ZERO_RANGE (the
 * maximum is 0 and neither TLC_NORM_EPS nor TLC_NO_NORM is set).  The d_f slice of a graph that is not TLC_ST_OK is left untouched and no
 * other graph is affected.  A graph without nodes: TLC_ST_OK, nothing written.
 * d_parent int32[2, total_nodes] (may be NULL), written for every graph that is not TLC_ST_BAD_INPUT: THE TREE of root r.  With R_r the
 * root-sourced fixpoint (R_r[r] = 0, R_r[x] = min over the neighbours y of fl(R_r[y] + w(x, y))), P_r[x] = the lowest local id y among the
 * neighbours of x with R_r[y] < R_r[x] and fl(R_r[y] + w(x, y)) == R_r[x] (IEEE ==); -1 for the root, for a node r does not reach, for a
 * node without such a neighbour (only where rounding absorbs a weight), and in row 1 of a graph with one root.  With pairwise distinct path
 * lengths (what learned weights have) this is the shortest-path tree and the path behind D_r[x] is x's tree path.  Under ties the
 * filtration is not differentiable and this tree is the fixed convention (the stance of tlc_pd_point_vertices).
 * Size classes, cut on the device: up to TLC_DIST_WAVE_NMAX nodes a wavefront per graph; up to TLC_DIST_WG_NMAX nodes and TLC_DIST_WG_MMAX
 * edges a workgroup per graph, distances in LDS; larger: the whole device, distances in d_work, a launch per Bellman-Ford round, the
 * "changed" word read back every 8 rounds (the entry then synchronises the stream; a batch of at most TLC_DIST_WG_NMAX nodes and
 * TLC_DIST_WG_MMAX edges in total never does).  No floating-point atomics: a graph's bits depend neither on the batch, nor on d_work, nor
 * on the run.  d_work: 256-byte aligned, at least tlc_dist_filtration_work_bytes() bytes (host arithmetic; 16 B per edge + 12 B per graph,
 * and 56 B per node when the batch can hold a graph of the third class); more bytes = more per-source fallback searches of that class in
 * flight (8 B per node each, up to 256).  The u64 at byte TLC_DIST_WORK_FALLBACKS_OFF of d_work counts the sources that took the fallback.
 * TLC_ERR_INVALID_ARG, nothing launched: null required pointers, negative sizes, an unknown flag, a d_work below the minimum or
 * misaligned.  TLC_ERR_UNSUPPORTED: 2^30 nodes or edges in the batch.  n_graphs == 0: TLC_OK, nothing read.
 *
 * tlc_dist_filtration_vjp: the forward's inputs and flags, d_parent of that forward, d_grad_f float64[total_nodes] -> d_grad_w
 * float64[total_edges], every entry of every TLC_ST_OK graph, zeros included (other graphs: untouched).  d_f is not read (may be NULL):
 * the values are rebuilt from the tree.  d_status: TLC_ST_OK, TLC_ST_BAD_INPUT, TLC_ST_ZERO_RANGE as above.  The specification, in this
 * order of operations (fp64, no fused multiply-add); r runs over root 0 and, with two roots, root 1:
 *   e_r[x]  = the edge (x, P_r[x]) if P_r[x] >= 0 and that edge exists, else none.
 *   T_r[x]  = t after: t = +0.0; c = x; while c has e_r[c] (at most n steps): t = t + w[e_r[c]], c = P_r[c].  If the walk does not end at
 *             root r, x "does not arrive" at r and T_r[x] = 100.  depth_r[x] = the steps of that walk.
 *   q[x]    = 0 at a root; else T_0 + T_1 / min / max / T_0, as the forward.  dm[x] = q[x], but max(T_0, T_1) for 'min' (0 at a root).
 *   den0    = max_x dm[x];  den = den0, den0 + 1e-10 (TLC_NORM_EPS) or 1 (TLC_NO_NORM);  x* = the lowest x with dm[x] == den0.
 *   a[x]    = g[x] / den;  corr = (sum over x ascending, from +0.0, of g[x] * q[x]) / (den * den), only with a normalisation.
 *   sel_r(x): root r contributes to q[x] -- 'sum' and one root: yes; 'min': r == (T_1 < T_0 ? 1 : 0); 'max': r == (T_1 > T_0 ? 1 : 0).
 *   dsel_r(x): root r contributes to dm[x] -- as sel_r, but for 'min': r == (T_1 > T_0 ? 1 : 0)  (the divisor of 'min' is a 'max').
 *   c_r[x]  = a[x] if sel_r(x), else +0.0;  with a normalisation and x == x* and dsel_r(x): c_r[x] = c_r[x] - corr;
 *             c_r[x] = +0.0 where the value is forced: x is a root, or x does not arrive at r (the sentinel).
 *   S_r[x]  = c_r[x], then + S_r[z] for the tree children z of x (e_r[z] exists and P_r[z] == x) in ascending id; computed level by
 *             level from the deepest depth_r, every node PULLING over its child list, never a child pushing.
 *   grad_w[e] = +0.0, then + S_0[z] if e == e_0[z] for one of its ends z, then + S_1[z] likewise.
 * A group of 64 threads (up to TLC_DIST_WAVE_NMAX nodes) or 256 threads per graph, all state in d_work (tlc_dist_filtration_vjp_work_bytes():
 * 72 B per node + 16 B per edge + 12 B per graph), no host synchronisation. */
#define TLC_DIST_WAVE_NMAX          64      /* most nodes of a graph that one wavefront computes */
#define TLC_DIST_WG_NMAX            2048    /* most nodes ... */
#define TLC_DIST_WG_MMAX            4096    /* ... and most undirected edges of a graph that one workgroup computes in LDS */
#define TLC_DIST_WORK_FALLBACKS_OFF 64      /* byte offset in d_work of the u64 count of sources that took the fallback search */
int tlc_dist_filtration_work_bytes(int64_t n_graphs, int64_t total_nodes, int64_t total_edges, int64_t* bytes);
int tlc_dist_filtration_vjp_work_bytes(int64_t n_graphs, int64_t total_nodes, int64_t total_edges, int64_t* bytes);
int tlc_dist_filtration(int64_t n_graphs, const int64_t* d_node_ptr, const int64_t* d_edge_ptr, const int32_t* d_edges,
                        const double* d_w, const int32_t* d_roots, int64_t total_nodes, int64_t total_edges, uint32_t flags,
                        double* d_f, uint8_t* d_status, int32_t* d_parent, void* d_work, int64_t work_bytes, void* stream);
int tlc_dist_filtration_vjp(int64_t n_graphs, const int64_t* d_node_ptr, const int64_t* d_edge_ptr, const int32_t* d_edges,
                            const double* d_w, const int32_t* d_roots, int64_t total_nodes, int64_t total_edges, uint32_t flags,
                            const double* d_f, const int32_t* d_parent, const double* d_grad_f, double* d_grad_w,
                            uint8_t* d_status, void* d_work, int64_t work_bytes, void* stream);

/* ---- Vicinity images differentiable in the GRAPH's edge weights (csrc/vic_grad.hip): what lies between the kappa of the
 * graph's edges and the packed weights of tlc_dist_filtration, and between the decoder's loss and the image table.  Every call is
 * asynchronous on `stream`, reads nothing back and uses no floating-point atomics.
 *
 * tlc_packed_edge_lookup: d_graph_edges int32[n_graph_edges, 2], every undirected edge once with lo < hi, ascending by (lo, hi) (what
 * np.unique or tlc_graph_components produces).  The packed vicinity batch of Vicinities.batch / tlc_pack_vicinities / tlc_vicinity_filtration
 * with exact offsets: d_node_ptr / d_edge_ptr int64[n_vicinities + 1], d_ids the global ids, ascending inside a vicinity, int64[total_nodes]
 * (ids_int64 = 1) or int32 (0), d_edges int32[total_edges, 2] local ids.  d_pairs int32[n_vicinities, 2] global ids, or NULL (d_roots NULL too).
 * Out: d_eid int32[total_edges] = the index in d_graph_edges of the packed edge (either order of its ends), by binary search;
 * d_roots int32[n_vicinities, 2] = the local ids of the pair's ends in the vicinity's slice of d_ids, by binary search; one_root = 1:
 * only the first end is looked up and d_roots[:, 1] = -1, as tlc_dist_filtration reads one root.  d_status uint8[n_vicinities]: TLC_ST_OK, or
 * TLC_ST_BAD_INPUT -- a packed edge that is not in the list or has a local id outside its vicinity, or a looked-up end that is not in
 * the vicinity: every d_eid of that vicinity is -1 and its d_roots row is (-1, -1) -- or offsets that are negative, decrease or pass the
 * totals (d_roots (-1, -1), no d_eid written).  No other vicinity is affected.  n_vicinities == 0: TLC_OK, nothing read.
 * TLC_ERR_INVALID_ARG, nothing launched: a negative size, 2^31 edges, a flag other than 0 / 1, a null required pointer, d_pairs without
 * d_roots or the reverse. */
int tlc_packed_edge_lookup(int64_t n_graph_edges, const int32_t* d_graph_edges, int64_t n_vicinities, const int64_t* d_node_ptr,
                           const int64_t* d_edge_ptr, const void* d_ids, int32_t ids_int64, const int32_t* d_edges, int64_t total_nodes,
                           int64_t total_edges, const int32_t* d_pairs, int32_t one_root, int32_t* d_eid, int32_t* d_roots,
                           uint8_t* d_status, void* stream);

/* tlc_segment_index (one-off per pair list): d_key int32[n_items], the key of every item; a key outside 0 .. n_keys-1 (negative: the -1
 * of a refused vicinity) is skipped.  Out: d_seg_ptr int64[n_keys + 1], d_seg_pos int32[n_items]: the items of key k are
 * d_seg_pos[d_seg_ptr[k] .. d_seg_ptr[k + 1]), ascending; behind d_seg_ptr[n_keys] lie the skipped items, ascending.  A stable radix
 * sort of (key, position) (two 8-bit digits while n_keys < 2^16, else four) and one binary search per key: integers only, the same
 * output on every run.  d_work: 256-byte aligned, tlc_segment_index_work_bytes() bytes (12 B per item and the sort's histograms).
 * TLC_ERR_INVALID_ARG, nothing launched: a size outside 0 .. 2^31 - 1, a null required pointer, a d_work too small or misaligned.
 *
 * tlc_segment_sum_f64 (per step): d_out[k] = the sum of v_j = d_val[d_seg_pos[d_seg_ptr[k] + j]], j = 0 .. L-1, L the segment's length;
 * d_val float64[n_items].  THE ORDER, operation by operation (fp64, round to nearest, no fused multiply-add); it depends on L alone:
 *   L <= TLC_SEG_LANE_MAX (one lane):        s = +0.0; for j = 0 .. L-1: s = s + v_j.  d_out[k] = s  (L = 0: +0.0).
 *   L <= TLC_SEG_WAVE_MAX (one wavefront):   for l = 0 .. 63: p[l] = +0.0; for j = l, l + 64, l + 128, ... < L: p[l] = p[l] + v_j.
 *                                            FOLD: for d = 32, 16, 8, 4, 2, 1: for every l < d at once: p[l] = p[l] + p[l + d].
 *                                            d_out[k] = p[0].
 *   longer (one workgroup of 256 threads):   for t = 0 .. 255: p[t] = +0.0; for j = t, t + 256, ... < L: p[t] = p[t] + v_j.
 *                                            For w = 0 .. 3: q[w] = FOLD of p[64 w .. 64 w + 63].  d_out[k] = ((q[0] + q[1]) + q[2]) + q[3].
 * Every sum starts from +0.0, so no output is -0.0.  The classes are cut on the device: a first kernel (a thread per segment) sums
 * the first class and lists the segments of the other two in d_work -- in the order of arrival, which decides who sums a segment and
 * never how.  Neither the batch, nor the grid, nor d_work, nor the run changes a bit.  A d_seg_pos entry outside 0 .. n_items-1 counts as
 * +0.0 and a segment whose offsets decrease or leave 0 .. n_items as empty: a damaged index reads nothing out of bounds.
 * d_work: 256-byte aligned, tlc_segment_sum_work_bytes() bytes (8 B per key + 256).  n_keys == 0: TLC_OK.  Refusals as above. */
#define TLC_SEG_LANE_MAX  16     /* longest segment that one lane sums */
#define TLC_SEG_WAVE_MAX  2048   /* longest segment that one wavefront sums; longer ones take a workgroup */
int tlc_segment_index_work_bytes(int64_t n_items, int64_t n_keys, int64_t* bytes);
int tlc_segment_index(int64_t n_items, const int32_t* d_key, int64_t n_keys, int64_t* d_seg_ptr, int32_t* d_seg_pos, void* d_work,
                      int64_t work_bytes, void* stream);
int tlc_segment_sum_work_bytes(int64_t n_keys, int64_t* bytes);
int tlc_segment_sum_f64(int64_t n_keys, const int64_t* d_seg_ptr, const int32_t* d_seg_pos, int64_t n_items, const double* d_val,
                        double* d_out, void* d_work, int64_t work_bytes, void* stream);

/* d loss / d PI of tlc_lp_decode_fused_f32: the inputs of tlc_lp_decode_bwd_f32 up to d_gprob (d_emb_pre is not read: the renorm lies in
 * front of the embedding) -> d_gpi float32[n_pairs, 25].  With gz[k], k = 0 .. 24, the gradient at the hidden layer's pre-activation
 * that tlc_lp_decode_bwd_f32 forms (the Fermi-Dirac derivative -gprob p^2 exp(z), the clamp: 0 beyond 40, the sign of the abs, times
 * W2[k], times 1 or 0.2 by the sign of h[k]), in f32: d_gpi[i][j] = acc after acc = +0.0; for k = 0 .. 24: acc = acc + W1[k][16 + j] * gz[k]
 * (the product rounded, then the sum: no fused multiply-add).  A pair with an end outside 0 .. n_nodes-1 gets zeros.  emb_dim 16 / pi_dim
 * 25, else TLC_ERR_UNSUPPORTED; null pointers and negative sizes: TLC_ERR_INVALID_ARG; n_pairs == 0: TLC_OK.  One thread per pair, no
 * scratch, bit-identical from run to run. */
int tlc_lp_decode_bwd_pi_f32(int64_t n_pairs, const int32_t* d_pairs, const float* d_emb_pre, const float* d_emb, int32_t n_nodes,
                             int32_t emb_dim, const float* d_pi, int32_t pi_dim, const float* d_W1, const float* d_b1, const float* d_W2,
                             const float* d_b2, const float* d_gprob, float* d_gpi, void* stream);

/* ---- The sum-aggregating baselines of the PDGNN teacher (Knowledge_Distillation/Teacher_model.py:148-175,202-208: GINConv, GCNConv,
 * SAGEConv), one layer form (csrc/gnn_layers.hip) on any CSR BY TARGET, block-diagonal or one big graph:
 *   agg_i = sum over the in-edges e of i of coef[e] * x_src[e], + self_scale * x_i     z_i = Wa agg_i + Ws x_i + b     y_i = act(z_i)
 *   GIN: the edge list as given, coef NULL, self_scale 1 (eps = 0), Wa = nn.0.weight, b = nn.0.bias, ReLU or none;
 *   GCN: tlc_gcn_norm_csr's operator and values, self_scale 0, Wa = weight^T, b = bias;
 *   SAGE (PyG 1.6.1): coef = 1 / max(in-degree of the target, 1), self_scale 0, Wa = lin_l.weight, Ws = lin_r.weight, b = lin_l.bias.
 * d_rowptr int32[n + 1], d_src int32[rowptr[n]] (not read, and may be NULL, when every row is empty), d_coef f32[rowptr[n]] or NULL (all 1), d_X f32[n, c_in], d_Wa f32[c_out, c_in], d_Ws
 * the same or NULL, d_bias f32[c_out] or NULL, act: TLC_GNN_ACT_NONE / _RELU / _PRELU (slope > 0 then, else ignored), d_out f32[n, c_out],
 * d_agg f32[n, c_in] or NULL: the aggregate, kept for the backward.
 * Order of operations, all in f32.  Per element k of a row: acc = +0; for the row's entries e ascending: acc = acc + (coef[e] * x_src[e][k])
 * (the product rounded first; coef NULL: acc + x_src[e][k]); then, with self_scale != 0, acc = acc + (self_scale * x_i[k]).  The projection
 * is the f32 MFMA's (v_mfma_f32_16x16x4f32) from a zero accumulator: the four-wide steps {16 q + e, 16 q + 4 + e, 16 q + 8 + e, 16 q + 12 + e}
 * of k for q ascending and e = 0 .. 3 inside, k padded with zeros to a multiple of 16, first all of Wa agg, then all of Ws x; then + b,
 * then the activation.  No atomics; a row of d_out / d_agg depends on that row's entries alone: the same bits from run to run and for a
 * graph alone or anywhere in any batch.  A source id outside 0 .. n - 1 makes its row NaN and reads nothing.
 * c_in in 1 .. 64 and c_out in {8, 16, 32, 64}, else TLC_ERR_UNSUPPORTED; null required pointers, n_nodes < 0, an unknown act or PReLU with
 * a slope <= 0: TLC_ERR_INVALID_ARG; nothing is written in either case.  n_nodes == 0: TLC_OK. */
#define TLC_GNN_ACT_NONE   0
#define TLC_GNN_ACT_RELU   1
#define TLC_GNN_ACT_PRELU  2
int tlc_gnn_layer_fwd(int32_t n_nodes, const int32_t* d_rowptr, const int32_t* d_src, const float* d_coef, float self_scale,
                      const float* d_X, int32_t c_in, int32_t c_out, const float* d_Wa, const float* d_Ws, const float* d_bias,
                      int32_t act, float slope, float* d_out, float* d_agg, void* stream);

/* Gradients of tlc_gnn_layer_fwd.  dZ = d_gout * act'(d_out) (read off the sign of the output: 1 above 0; at and below it 0 for ReLU and
 * `slope` for PReLU, as torch does);  G = dZ Wa;  gX = S^T G + self_scale G + dZ Ws;  gWa = dZ^T agg;  gWs = dZ^T X;  gb = colsum dZ.
 * S^T comes in as a second CSR, BY SOURCE (d_rowptr_t int32[n + 1], d_col_t = the targets, d_coef_t = the forward's coefficient of the
 * same edge or NULL; for GCN tlc_gcn_norm_csr_t), so the scatter towards the sources is a gather: gX[i][k] = acc after acc = +0; for row
 * i's entries e ascending: acc = acc + (coef_t[e] * G[col_t[e]][k]); with self_scale != 0: acc = acc + (self_scale * G[i][k]); with Ws:
 * acc = acc + (dZ Ws)[i][k].  G and dZ Ws are f32 MFMA products as in the forward.  The weight gradients are tlc_gemm_tn_f32 products over
 * the materialised dZ: split-K partials over a partition that n_nodes and the widths alone fix, added in split order.  No floating-point
 * atomics anywhere: every output is the same bits from run to run, and a graph's rows of gX the same alone or in any batch.
 * d_agg: the forward's; d_out: read only with an activation; d_X: read only for d_gWs.  d_gX f32[n, c_in] or NULL (first layer: neither
 * G nor the CSR by source is touched); d_gWa f32[c_out, c_in]; d_gWs the same or NULL; d_gb f32[c_out] or NULL.
 * d_work: tlc_gnn_layer_bwd_work_bytes(n_nodes, c_in, c_out) bytes (-1 for a negative size), 16-byte aligned.  Refusals as the forward's,
 * and TLC_ERR_INVALID_ARG for a d_work too small or misaligned.  n_nodes == 0: the weight gradients are zeros. */
int64_t tlc_gnn_layer_bwd_work_bytes(int32_t n_nodes, int32_t c_in, int32_t c_out);
int tlc_gnn_layer_bwd(int32_t n_nodes, const int32_t* d_rowptr_t, const int32_t* d_col_t, const float* d_coef_t, float self_scale,
                      const float* d_X, const float* d_agg, const float* d_out, const float* d_gout, int32_t c_in, int32_t c_out,
                      const float* d_Wa, const float* d_Ws, int32_t act, float slope, float* d_gX, float* d_gWa, float* d_gWs,
                      float* d_gb, void* d_work, int64_t work_bytes, void* stream);

/* The inference forward of Base_Model's four layers (Teacher_model.py:213-241: conv1 -> conv2 -> conv4 -> conv3, in_dim 1, hidden 32) in
 * ONE launch on a batch cut into self-contained tiles (d_tile_ptr int32[n_tiles + 1] of tlc_gat_tile_cut: at most 192 nodes, no edge
 * crosses a cut): a workgroup keeps a tile's node rows in LDS through the four layers, so the intermediate rows never reach HBM.
 * d_x f32[n_nodes]; params: HOST array of 12 device pointers, per layer in the order above {Wa f32[32, c_in], Ws or NULL, bias or NULL},
 * Ws on all four layers or on none; acts / slopes: HOST int32[4] / float[4]; d_out f32[n_nodes, 32].  The layers run the device code of
 * tlc_gnn_layer_fwd operation for operation: the rows equal, bit for bit, those of four tlc_gnn_layer_fwd calls.  A caller-made cut with
 * an empty tile, one above 192 rows or one outside the batch gets NaN rows.  hidden != 32: TLC_ERR_UNSUPPORTED; n_tiles == 0: TLC_OK,
 * nothing written (no cut, e.g. one big graph: run the layers one by one). */
int tlc_gnn_stack_fwd(int32_t n_nodes, const int32_t* d_rowptr, const int32_t* d_src, const float* d_coef, float self_scale,
                      int32_t n_tiles, const int32_t* d_tile_ptr, const float* d_x, int32_t hidden, const float* const* params,
                      const int32_t* acts, const float* slopes, float* d_out, void* stream);

/* ---- The PDGNN layer family (csrc/msg_layers.hip): Knowledge_Distillation/gat_conv.py:113-216 with its ablation switches (new_node_feat
 * :78-79,193-195; use_edge_attn :197-200) and PD_conv.py's PDConv (:179-219), on any CSR BY TARGET with the self loops added
 * (tlc_csr_by_target).  Per entry e = (j -> i) of row i:
 *   x_l = X Wl^T     alpha = x_l . att     P = x_l Wij[:, :C]^T     Q = x_l Wij[:, C:]^T                      (C = c_out)
 *   h_e = leaky_relu(P_i + Q_j, 0.2) with TLC_MSG_NODE_FEAT, else x_l[j]
 *   a_e = softmax over row i of leaky_relu(alpha_j + alpha_i, 0.2) with TLC_MSG_EDGE_ATTN, else 1           m_e = a_e * h_e
 *   out_i = [ sum_e m_e || min_e m_e + max_e m_e ] + bias  (TLC_MSG_AGG_SUM_MINMAX, gat_conv.py:216)
 *   out_i = [ sum_e m_e || min_e m_e             ] + bias  (TLC_MSG_AGG_SUM_MIN,    PD_conv.py:219), then PReLU when prelu_slope >= 0.
 * Operands as tlc_gat_layer_fwd's: d_Wl f32[C, c_in], d_att f32[C] (may be NULL without EDGE_ATTN), d_Wij f32[C, 2C] (may be NULL without
 * NODE_FEAT), d_bias f32[2C], d_out f32[n, 2C].  d_work: tlc_msg_layer_fwd_work_bytes(n_nodes, c_in, c_out, mode) bytes (-1 for a negative
 * size or unknown mode bits), 16-byte aligned: x_l, alpha, P and Q of the call.
 * Order of operations, all in f32, every product rounded before it is added.  x_l, P and Q are f32 MFMA products (v_mfma_f32_16x16x4f32)
 * from a zero accumulator: the four-wide steps {16 q + e, 16 q + 4 + e, 16 q + 8 + e, 16 q + 12 + e} of k for q ascending and e = 0 .. 3
 * inside, k padded with zeros to a multiple of 16.  alpha_i: four chains from +0 over k = 16 q + 4 g + e (q, then e ascending), g = 0 .. 3,
 * then (g + (g ^ 1)) + the other pair.  A row's softmax: logits leaky_relu(alpha_j + alpha_i); maximum exact; the exponentials
 * __expf(logit - maximum) are summed in C chains (chain c takes the row's entries c, c + C, ...; from +0, ascending) that meet in a
 * butterfly over c ^ C/2, ..., c ^ 1; denominator = that + 1e-16 (PyG's softmax); a_e = exponential / denominator.  Per channel: sum = +0,
 * then + m_e for the row's entries ascending; min / max exact.  An empty row (possible through this ABI only) has sum 0 and min = max = 0
 * (torch_scatter's value), so out_i = bias.  No atomics; a row's bits depend on that row's entries alone: the same from run to run and for a
 * graph alone or anywhere in any batch.  A source id outside 0 .. n - 1 makes its row NaN and reads nothing.
 * c_in in 1 .. 64 and c_out in {8, 16, 32, 64}, else TLC_ERR_UNSUPPORTED; null required pointers, n_nodes < 0, unknown mode / agg bits, a
 * d_work too small or misaligned: TLC_ERR_INVALID_ARG; nothing is written in either case.  n_nodes == 0: TLC_OK. */
#define TLC_MSG_NODE_FEAT      1
#define TLC_MSG_EDGE_ATTN      2
#define TLC_MSG_AGG_SUM_MINMAX 0
#define TLC_MSG_AGG_SUM_MIN    1
int64_t tlc_msg_layer_fwd_work_bytes(int32_t n_nodes, int32_t c_in, int32_t c_out, int32_t mode);
int tlc_msg_layer_fwd(int32_t n_nodes, const int32_t* d_rowptr, const int32_t* d_src, const float* d_X, int32_t c_in, int32_t c_out,
                      const float* d_Wl, const float* d_att, const float* d_Wij, const float* d_bias, int32_t mode, int32_t agg,
                      float prelu_slope, void* d_work, int64_t work_bytes, float* d_out, void* stream);

/* Gradients of tlc_msg_layer_fwd, WITHOUT floating-point atomics.  Nothing of the forward is kept: the node rows are recomputed.
 * d_rowptr_t / d_col_t / d_pos_t: the same structure as a CSR BY SOURCE -- row j lists the entries (j -> i) as d_col_t = i and d_pos_t =
 * the entry's position in d_src, positions ascending inside a row -- so that the adjoint of "gather from the sources" is a second gather.
 * Pass 1, per target row: Gz = d_gout * PReLU'(d_out) (`slope` at d_out <= 0, as torch); the row's softmax statistics; per channel the
 * FIRST entry of the row attaining the minimum / the maximum (strict comparisons in entry order -- tlc_gat_layer_bwd's convention; torch
 * splits the gradient of a tie evenly instead, which differs per entry but not per tensor when the tying entries share both ends, as
 * repeated edges do); with gm_e = Gz_sum + Gz_mm ([e is arg-min] + [e is arg-max]) per channel: S_i = sum_e (sum_c gm_e m_e), the logit
 * gradient gt_e = ((sum_c gm_e m_e) - a_e S_i) leaky'(alpha_j + alpha_i), gP_i = sum_e gm_e a_e leaky'(P_i + Q_j), and the target side of
 * galpha_i = sum_e gt_e.  It keeps per row: gP, that sum, the maximum, the denominator, S and the arg entries; nothing per entry.
 * Pass 2, per source row: every entry's a_e, m_e, gm_e and gt_e again from those; gQ_j = sum_e gm_e a_e leaky'(.), galpha_j = (sum_e gt_e) +
 * the target side.  Every sum over entries: +0, then the row's entries ascending; every sum over channels: a butterfly over c ^ C/2, ...,
 * c ^ 1.  Then gx_l = gP Wij[:, :C] + gQ Wij[:, C:] + galpha (x) att (MFMA products as above, the rank-one term added last; without
 * NODE_FEAT gx_l = gQ + galpha (x) att), gX = gx_l Wl, and the weight gradients gWl = gx_l^T X, gWij = [gP^T x_l | gQ^T x_l], gatt =
 * galpha^T x_l, gbias = column sums of Gz as tlc_gemm_tn_f32 products: split-K partials over a partition that n_nodes and the widths alone
 * fix, added in split order.  Every output is the same bits from run to run, and a graph's rows of d_gX the same alone or in any batch.
 * d_out: read only with prelu_slope >= 0.  d_gX f32[n, c_in] or NULL (first layer: the last product is left out; the source pass still
 * runs, because the weight gradients need gQ and galpha).  d_gWl f32[C, c_in], d_gbias f32[2C]; d_gatt f32[C] is written only with
 * EDGE_ATTN, d_gWij f32[C, 2C] only with NODE_FEAT (either may be NULL otherwise).
 * d_work: tlc_msg_layer_bwd_work_bytes(n_nodes, n_entries, c_in, c_out, mode) bytes, 16-byte aligned; it does not grow with n_entries.
 * Refusals as the forward's.  n_nodes == 0: TLC_OK, the weight gradients are zeros. */
int64_t tlc_msg_layer_bwd_work_bytes(int32_t n_nodes, int64_t n_entries, int32_t c_in, int32_t c_out, int32_t mode);
int tlc_msg_layer_bwd(int32_t n_nodes, const int32_t* d_rowptr, const int32_t* d_src, const int32_t* d_rowptr_t, const int32_t* d_col_t,
                      const int32_t* d_pos_t, const float* d_X, int32_t c_in, int32_t c_out, const float* d_Wl, const float* d_att,
                      const float* d_Wij, int32_t mode, int32_t agg, float prelu_slope, const float* d_out, const float* d_gout,
                      float* d_gX, float* d_gWl, float* d_gatt, float* d_gWij, float* d_gbias, void* d_work, int64_t work_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TLCGNN_H */

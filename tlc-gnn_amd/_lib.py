"""ctypes binding of libtlcgnn_hip.so (the C ABI of include/tlcgnn.h).

PyTorch is plumbing here: it owns device memory and streams; every compute call goes through the C ABI
with raw device pointers.  There is NO CPU fallback: if the HIP library is missing or no GPU is visible,
the product path raises.
"""
import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libtlcgnn_hip.so")
CSRC = os.path.join(HERE, "csrc")

OK = 0
ERRORS = {1: "TLC_ERR_INVALID_ARG", 2: "TLC_ERR_HIP", 3: "TLC_ERR_NO_DEVICE", 4: "TLC_ERR_UNSUPPORTED",
          5: "TLC_ERR_OUT_OF_MEMORY"}

ST_OK, ST_MISSING_NODE, ST_DISCONNECTED, ST_ZERO_RANGE, ST_NO_TREE_EDGE, ST_TOO_LARGE = range(6)
ST_NOT_CONVERGED, ST_BAD_INPUT = 6, 7                               # tlc_hks_batch (both), tlc_struct_batch (ST_BAD_INPUT)
HKS_NMAX, HKS_LDS_NMAX, HKS_TMAX, HKS_NORMALISE = 256, 96, 8, 0x1   # TLC_HKS_* of include/tlcgnn.h
HKS_LARGE_NMAX, HKS_LARGE_TIME_MAX = 4096, 64.0                     # TLC_HKS_LARGE_* of include/tlcgnn.h (tlc_hks_large_batch)
HKS_LARGE_TILE, HKS_LARGE_KSTEP = 64, 16                            # HKSL_T, HKSL_KS of csrc/hks_large.hip: output-tile side, K-step
HKS_SPARSE_TIME_MAX, HKS_SPARSE_PANEL, HKS_SPARSE_LONG_ROW = 64.0, 64, 256      # TLC_HKS_SPARSE_* of include/tlcgnn.h (tlc_hks_sparse_batch)
STRUCT_DEGREE, STRUCT_CENTRALITY, STRUCT_CLUSTERING, STRUCT_NORMALISE = 0x1, 0x2, 0x4, 0x100      # TLC_STRUCT_* of include/tlcgnn.h
STRUCT_WAVE_NMAX, STRUCT_LDS_SMALL_NMAX, STRUCT_LDS_NMAX, STRUCT_BITMAP_BITS = 64, 256, 1024, 65536
STRUCT_KINDS = {"degree": STRUCT_DEGREE, "centrality": STRUCT_CENTRALITY, "clustering": STRUCT_CLUSTERING}   # in output-row order
CC_WAVE_NMAX = 64                                                   # TLC_CC_WAVE_NMAX: tlc_graph_components, a wavefront per graph up to here
OTD_WAVE_PRODUCT, OTD_WAVE_SUPPORT, OTD_WAVE_DENOM, OTD_MAX_SUPPORT, OTD_LDS_BYTES = 8192, 256, 65535, 12794, 153600   # TLC_OTD_* of include/tlcgnn.h
KEEP_ZERO_PERS, INCLUDE_ROOTS, NORM_EPS, PI_ORD0_EXT1, NO_EXT1, UNREACHABLE_100 = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20
DESC_MIN, DESC_MAX, DESC_ROOT1, NO_NORM = 0x40, 0x80, 0xC0, 0x100
PD_L_NMAX, PD_L_MMAX = 2048, 4096                                   # TLC_L_NMAX / TLC_L_MMAX of csrc/tlc_kernels.h: above either, the HUGE class
PD_HUGE_NMAX, PD_HUGE_MMAX = 65535, (1 << 24) - 2                   # above either, tlc_pd_from_filtration does not compute the graph
PD_WIDE_MAX_ITEMS, PD_WIDE_FORCE_FALLBACK, PD_WIDE_BAD_INPUT_ROW, PD_WIDE_N_STATS = 1 << 27, 0x40000000, -2, 5   # TLC_PD_WIDE_* of include/tlcgnn.h
PD_WIDE_LDS_NODES = 40000                                           # TLC_PD_WIDE_LDS_NODES: comp[] of the elder-rule passes in LDS up to here
PD_WIDE_BLOCK, PD_WIDE_SORT_TILE, PD_WIDE_SCAN_CHUNK = 256, 4096, 2048   # workgroup width, edges per radix tile, flags per scan chunk (csrc/pd_wide.hip)
PD_VERT_WAVE_NMAX, PD_VERT_LDS_NMAX = 64, 2048                       # TLC_PD_VERT_*: the size classes of csrc/pd_grad.hip (wavefront / workgroup per graph)
SW_WAVE_NMAX, SW_LDS_NMAX, SW_MAX_DIRS = 64, 2048, 128              # TLC_SW_*: the size classes of csrc/sliced_w.hip by n + m, and the most directions
W2_LDS_NMAX, W2_LARGE_NMAX, W2_LARGE_COUNTERS = 4096, 65536, 4       # TLC_W2_*: the rows the LDS matching kernels take, the workspace tier's cap, its counters per slot
BN_WAVE_NMAX, BN_NMAX = 512, 4096                                   # TLC_BN_*: the size classes of csrc/bottleneck.hip by n + m (wavefront / workgroup per problem)
PI_MAX_RES, PI_GRAD_WEIGHT, PI_GRAD_FULL = 128, 0, 1                # TLC_PI_*: the general imager of csrc/pi_general.hip
PI_SLICE, PI_CHUNK, PI_GROUP = 1024, 32, 32                         # points per K-slice / per LDS chunk, K-split diagrams per launch
LS_WAVE_NMAX, LS_LDS_NMAX, LS_KMAX, LS_TMAX = 64, 4096, 16, 4096    # TLC_LS_*: the size classes of csrc/landscape.hip by n, the most levels and samples
DG_ALL, DG_PAIRED, DG_SYMMETRIC, DG_MIRROR, DG_SLICE, DG_GROUP = 0x1, 0x2, 0x4, 0x8, 1024, 1024   # TLC_DG_*: the layouts of csrc/dgm_gram.hip and its cuts
DIST_WAVE_NMAX, DIST_WG_NMAX, DIST_WG_MMAX, DIST_WORK_FALLBACKS_OFF = 64, 2048, 4096, 64   # TLC_DIST_*: the size classes of csrc/dist_filt.hip
SEG_LANE_MAX, SEG_WAVE_MAX, SEG_WG_THREADS = 16, 2048, 256           # TLC_SEG_*: the size classes of csrc/vic_grad.hip by segment length
GNN_ACT_NONE, GNN_ACT_RELU, GNN_ACT_PRELU, GNN_ROWS = 0, 1, 2, 64      # TLC_GNN_ACT_*; GN_ROWS of csrc/gnn_layers.hip: node rows per group
MSG_NODE_FEAT, MSG_EDGE_ATTN, MSG_AGG_SUM_MINMAX, MSG_AGG_SUM_MIN = 1, 2, 0, 1   # TLC_MSG_* of include/tlcgnn.h (csrc/msg_layers.hip)
DESCRIPTOR_FLAG ={"sum": 0, "min": DESC_MIN, "max": DESC_MAX}      # the three node values of filtration.build_fv

# every symbol include/tlcgnn.h declares (tests check that the library exports all of them)
SYMBOLS = [
    "tlc_version", "tlc_last_error", "tlc_device_count", "tlc_graph_create", "tlc_graph_destroy",
    "tlc_pd_pi_batch", "tlc_pd_pi_batch_async", "tlc_pd_pi_batch_join", "tlc_vicinity_filtration", "tlc_pd_pi_batch_stats", "tlc_pd_pi_batch_set_timing",
    "tlc_pd_pi_batch_timings", "tlc_pd_pi_batch_timing_history", "tlc_pd_pi_batch_sizes", "tlc_pd_pi_algorithmic_bytes", "tlc_pd_from_filtration",
    "tlc_pi_raster", "tlc_pi_raster_wgrad", "tlc_gcn_norm_csr", "tlc_gcn_norm_csr_t", "tlc_gemm_f32", "tlc_gemm_tn_f32", "tlc_lp_decode_bwd_f32", "tlc_binary_rank_metrics", "tlc_binary_rank_metrics_work_bytes",
    "tlc_nc_group_work_ints", "tlc_nc_group", "tlc_nc_linear_f32", "tlc_nc_linear_bwd_f32", "tlc_nc_curv_work_bytes", "tlc_nc_curv_fwd_f32",
    "tlc_nc_curv_bwd_f32", "tlc_spgemm_csr_dense_f32", "tlc_spmm_csr_f32", "tlc_renorm_rows_f32", "tlc_gcn2_encode_f32", "tlc_gcn2_encode_csr_f32",
    "tlc_lp_decode_fused", "tlc_lp_decode_fused_f32", "tlc_gat_layer_fwd", "tlc_gat_layer_tiled_fwd", "tlc_gat_tile_cut", "tlc_csr_by_target", "tlc_pdgnn_forward", "tlc_pdgnn_forward_work_bytes", "tlc_scatter_f32", "tlc_edge_head_fwd",
    "tlc_complement_rows", "tlc_complement_pairs", "tlc_select_rows", "tlc_pack_vicinities", "tlc_stack_batch", "tlc_ollivier_ricci_sinkhorn",
    "tlc_near_pairs", "tlc_w2_partial_matching", "tlc_w2_inference_matching", "tlc_gat_layer_bwd", "tlc_edge_head_bwd", "tlc_pack_offsets", "tlc_vicinity_sizes", "tlc_debug_dc_stats", "tlc_debug_tier_counts", "tlc_debug_chunk_counters", "tlc_debug_phase_profile", "tlc_debug_set_option", "tlc_debug_pair_times",
    "tlc_hks_batch", "tlc_hks_batch_work_bytes", "tlc_hks_large_batch", "tlc_hks_large_work_bytes", "tlc_hks_batch_dt", "tlc_hks_large_batch_dt",
    "tlc_hks_sparse_terms", "tlc_hks_sparse_work_bytes", "tlc_hks_sparse_batch", "tlc_hks_sparse_batch_dt", "tlc_struct_batch", "tlc_struct_batch_work_bytes",
    "tlc_ollivier_ricci_otd", "tlc_ollivier_ricci_otd_work_bytes", "tlc_pd_wide", "tlc_pd_wide_work_bytes",
    "tlc_pd_grad_work_bytes", "tlc_pd_point_vertices", "tlc_pd_filtration_grad",
    "tlc_sliced_w_work_bytes", "tlc_sliced_wasserstein",
    "tlc_w2_large_work_bytes", "tlc_w2_large_matching",
    "tlc_bottleneck_matching",
    "tlc_pi_image_work_bytes", "tlc_pi_image", "tlc_pi_image_vjp",
    "tlc_landscape_work_bytes", "tlc_landscape", "tlc_landscape_vjp",
    "tlc_dgm_gram_work_bytes", "tlc_dgm_gram", "tlc_dgm_gram_vjp",
    "tlc_graph_components_work_bytes", "tlc_graph_components",
    "tlc_dist_filtration_work_bytes", "tlc_dist_filtration_vjp_work_bytes", "tlc_dist_filtration", "tlc_dist_filtration_vjp",
    "tlc_packed_edge_lookup", "tlc_segment_index_work_bytes", "tlc_segment_index", "tlc_segment_sum_work_bytes", "tlc_segment_sum_f64",
    "tlc_lp_decode_bwd_pi_f32",
    "tlc_gcn2_encode_work_floats", "tlc_gemm_tn_work_floats", "tlc_lp_decode_bwd_work_floats", "tlc_nc_linear_bwd_work_floats",
    "tlc_gat_layer_fwd_work_floats", "tlc_gat_layer_tiled_fwd_work_floats", "tlc_gat_tile_cut_work_ints", "tlc_gat_tile_cut_max_tiles",
    "tlc_csr_by_target_work_ints", "tlc_gat_layer_bwd_work_floats", "tlc_edge_head_fwd_work_floats", "tlc_edge_head_bwd_work_floats",
    "tlc_gnn_layer_fwd", "tlc_gnn_layer_bwd_work_bytes", "tlc_gnn_layer_bwd", "tlc_gnn_stack_fwd",
    "tlc_msg_layer_fwd_work_bytes", "tlc_msg_layer_fwd", "tlc_msg_layer_bwd_work_bytes", "tlc_msg_layer_bwd",
]


class TlcError(RuntimeError):
    pass


def build(verbose=False, force=False):
    """Compile the HIP sources for gfx950 into tlc-gnn_amd/libtlcgnn_hip.so (hipcc cross-compiles without a GPU).
    force=True: `make clean` first, so every object is rebuilt from source (the "does it build" check must not be
    satisfied by a shipped .so)."""
    if force:
        subprocess.run(["make", "-C", CSRC, "clean"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    cmd = ["make", "-C", CSRC, "-j", str(min(8, os.cpu_count() or 1))]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if verbose or res.returncode != 0:
        print(res.stdout)
    if res.returncode != 0:
        raise TlcError("building libtlcgnn_hip.so failed")
    return LIB_PATH


_lib = None


def lib():
    """The loaded library; raises if it has not been built (no silent fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise TlcError("libtlcgnn_hip.so is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback for the product path)")
        # torch first: it ships its own libamdhip64, and a process must end up with ONE HIP runtime -- with this library (linked
        # against /opt/rocm's) loaded before torch, the two copies each initialise and the second sees no device
        # (`build()` followed by `smoke()` in one process: TLC_ERR_NO_DEVICE)
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        L.tlc_version.restype = C.c_char_p
        L.tlc_last_error.restype = C.c_char_p
        L.tlc_graph_create.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
        L.tlc_graph_destroy.argtypes = [C.c_void_p]
        L.tlc_pd_pi_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_uint32, C.c_int, C.c_void_p,
                                      C.c_void_p, C.c_void_p]
        L.tlc_pd_pi_batch_async.argtypes = L.tlc_pd_pi_batch.argtypes
        L.tlc_pd_pi_batch_join.argtypes = [C.c_void_p, C.c_void_p]
        L.tlc_vicinity_filtration.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_uint32, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p]
        L.tlc_pd_pi_batch_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.tlc_pd_pi_batch_set_timing.argtypes = [C.c_void_p, C.c_int]
        L.tlc_pd_pi_batch_timings.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.tlc_pd_pi_batch_timing_history.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        L.tlc_pd_pi_batch_sizes.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        L.tlc_pd_pi_algorithmic_bytes.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p]
        L.tlc_pd_from_filtration.argtypes = [C.c_int32] + [C.c_void_p] * 4 + [C.c_uint32] + [C.c_void_p] * 7
        L.tlc_pi_raster.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.tlc_pi_raster_wgrad.argtypes = [C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.tlc_gcn_norm_csr.argtypes = [C.c_int32, C.c_int64] + [C.c_void_p] * 6
        L.tlc_gemm_f32.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                   C.c_void_p, C.c_void_p]
        L.tlc_spgemm_csr_dense_f32.argtypes = [C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 5 + [C.c_int, C.c_void_p, C.c_void_p]
        L.tlc_spmm_csr_f32.argtypes = [C.c_int32] + [C.c_void_p] * 4 + [C.c_int32, C.c_void_p, C.c_int, C.c_void_p,
                                                                        C.c_void_p]
        L.tlc_renorm_rows_f32.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
        L.tlc_gcn2_encode_f32.argtypes = ([C.c_int32] + [C.c_void_p] * 4 + [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                          C.c_void_p, C.c_int32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p])
        L.tlc_gcn2_encode_csr_f32.argtypes = ([C.c_int32] + [C.c_void_p] * 6 + [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                              C.c_void_p, C.c_int32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p])
        L.tlc_lp_decode_fused.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.tlc_lp_decode_fused_f32.argtypes = L.tlc_lp_decode_fused.argtypes
        L.tlc_gcn_norm_csr_t.argtypes = [C.c_int32, C.c_int64] + [C.c_void_p] * 7
        L.tlc_gemm_tn_f32.argtypes = [C.c_int32, C.c_int32, C.c_int64] + [C.c_void_p] * 5
        L.tlc_lp_decode_bwd_f32.argtypes = ([C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32]
                                            + [C.c_void_p] * 10)
        L.tlc_binary_rank_metrics_work_bytes.argtypes = [C.c_void_p, C.c_int32, C.c_int, C.c_uint32]
        L.tlc_binary_rank_metrics_work_bytes.restype = C.c_int64
        L.tlc_binary_rank_metrics.argtypes = ([C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int32, C.c_uint32]
                                              + [C.c_void_p] * 6 + [C.c_int64, C.c_void_p])
        L.tlc_nc_group_work_ints.argtypes = [C.c_int32, C.c_int64]
        L.tlc_nc_group_work_ints.restype = C.c_int64
        L.tlc_nc_group.argtypes = [C.c_int32, C.c_int64] + [C.c_void_p] * 5
        L.tlc_nc_linear_f32.argtypes = [C.c_int32] * 3 + [C.c_void_p] * 5
        L.tlc_nc_linear_bwd_f32.argtypes = [C.c_int32] * 3 + [C.c_void_p] * 8
        L.tlc_nc_curv_work_bytes.argtypes = [C.c_int32, C.c_int64, C.c_int32, C.c_int32]
        L.tlc_nc_curv_work_bytes.restype = C.c_int64
        L.tlc_nc_curv_fwd_f32.argtypes = [C.c_int32, C.c_int64, C.c_int32, C.c_int32] + [C.c_void_p] * 10
        L.tlc_nc_curv_bwd_f32.argtypes = [C.c_int32, C.c_int64, C.c_int32, C.c_int32] + [C.c_void_p] * 14 + [C.c_int64, C.c_void_p]
        L.tlc_gat_layer_fwd.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p,
                                        C.c_void_p, C.c_void_p]
        L.tlc_csr_by_target.argtypes = [C.c_int32, C.c_int64] + [C.c_void_p] * 6
        L.tlc_pdgnn_forward_work_bytes.argtypes = [C.c_int32, C.c_int64, C.c_int32]
        L.tlc_pdgnn_forward_work_bytes.restype = C.c_int64
        L.tlc_pdgnn_forward.argtypes = [C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.tlc_gat_tile_cut.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_void_p]
        L.tlc_gat_layer_tiled_fwd.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p,
                                              C.c_void_p, C.c_void_p]
        L.tlc_scatter_f32.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int, C.c_int32, C.c_void_p,
                                      C.c_void_p, C.c_void_p]
        L.tlc_edge_head_fwd.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                        C.c_void_p, C.c_int32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_int32, C.c_void_p, C.c_void_p]
        L.tlc_complement_rows.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.tlc_complement_pairs.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                           C.c_void_p, C.c_void_p]
        L.tlc_select_rows.argtypes = [C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_uint32, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.tlc_pack_vicinities.argtypes = [C.c_int64] + [C.c_void_p] * 14
        L.tlc_pack_offsets.argtypes = [C.c_int64] + [C.c_void_p] * 6
        L.tlc_stack_batch.argtypes = [C.c_int64] + [C.c_void_p] * 4 + [C.c_int64, C.c_int64] + [C.c_void_p] * 3
        L.tlc_vicinity_sizes.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.tlc_ollivier_ricci_sinkhorn.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_double, C.c_double,
                                                  C.c_int32, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32,
                                                  C.c_int64, C.c_void_p]
        L.tlc_near_pairs.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p]
        L.tlc_w2_partial_matching.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int32] + [C.c_void_p] * 7
        L.tlc_w2_inference_matching.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int32] + [C.c_void_p] * 9
        L.tlc_gat_layer_bwd.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_float] + [C.c_void_p] * 9
        L.tlc_edge_head_bwd.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                        C.c_float] + [C.c_void_p] * 9
        L.tlc_hks_batch_work_bytes.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.POINTER(C.c_int64)]
        L.tlc_hks_batch.argtypes = ([C.c_void_p] * 3 + [C.c_int64] * 3 + [C.POINTER(C.c_double), C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_int64, C.c_void_p])
        L.tlc_hks_large_work_bytes.argtypes = [C.POINTER(C.c_int64), C.c_int64, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.tlc_hks_large_batch.argtypes = ([C.c_void_p] * 3 + [C.c_int64] * 3 + [C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int64,
                                          C.POINTER(C.c_double), C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p])
        L.tlc_hks_batch_dt.argtypes = ([C.c_void_p] * 3 + [C.c_int64] * 3 + [C.POINTER(C.c_double), C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p])
        L.tlc_hks_large_batch_dt.argtypes = ([C.c_void_p] * 3 + [C.c_int64] * 3 + [C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int64,
                                             C.POINTER(C.c_double), C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_int64, C.c_void_p])
        L.tlc_hks_sparse_terms.argtypes, L.tlc_hks_sparse_terms.restype = [C.c_double], C.c_int32
        L.tlc_hks_sparse_work_bytes.argtypes = [C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int64, C.c_int32, C.POINTER(C.c_int64),
                                                C.POINTER(C.c_int64)]
        L.tlc_hks_sparse_batch.argtypes = ([C.c_void_p] * 3 + [C.c_int64] * 3 + [C.POINTER(C.c_int64)] * 3 + [C.c_int64, C.POINTER(C.c_double),
                                           C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p])
        L.tlc_hks_sparse_batch_dt.argtypes = ([C.c_void_p] * 3 + [C.c_int64] * 3 + [C.POINTER(C.c_int64)] * 3 + [C.c_int64, C.POINTER(C.c_double),
                                              C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p])
        L.tlc_struct_batch_work_bytes.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.c_uint32, C.POINTER(C.c_int64)]
        L.tlc_struct_batch.argtypes = [C.c_void_p] * 3 + [C.c_int64] * 3 + [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        L.tlc_dist_filtration_work_bytes.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_int64)]
        L.tlc_dist_filtration_vjp_work_bytes.argtypes = L.tlc_dist_filtration_work_bytes.argtypes
        L.tlc_dist_filtration.argtypes = [C.c_int64] + [C.c_void_p] * 5 + [C.c_int64, C.c_int64, C.c_uint32] + [C.c_void_p] * 4 + [C.c_int64, C.c_void_p]
        L.tlc_dist_filtration_vjp.argtypes = [C.c_int64] + [C.c_void_p] * 5 + [C.c_int64, C.c_int64, C.c_uint32] + [C.c_void_p] * 6 + [C.c_int64, C.c_void_p]
        L.tlc_packed_edge_lookup.argtypes = ([C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64,
                                              C.c_int64, C.c_void_p, C.c_int32] + [C.c_void_p] * 4)
        L.tlc_segment_index_work_bytes.argtypes = [C.c_int64, C.c_int64, C.POINTER(C.c_int64)]
        L.tlc_segment_index.argtypes = [C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        L.tlc_segment_sum_work_bytes.argtypes = [C.c_int64, C.POINTER(C.c_int64)]
        L.tlc_segment_sum_f64.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        L.tlc_lp_decode_bwd_pi_f32.argtypes = ([C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32]
                                               + [C.c_void_p] * 7)
        L.tlc_ollivier_ricci_otd_work_bytes.argtypes = [C.c_int64, C.c_int32, C.c_int64, C.POINTER(C.c_int64)]
        L.tlc_ollivier_ricci_otd.argtypes = ([C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 4
                                             + [C.c_int64, C.c_int32, C.c_int64, C.c_void_p])
        L.tlc_pd_wide_work_bytes.argtypes = [C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int64, C.POINTER(C.c_int64)]
        L.tlc_pd_wide.argtypes = ([C.c_int64] + [C.c_void_p] * 4 + [C.c_uint32, C.POINTER(C.c_int64), C.c_int64] + [C.c_void_p] * 7
                                  + [C.c_int64, C.POINTER(C.c_int64), C.c_void_p])
        L.tlc_pd_grad_work_bytes.argtypes = [C.c_int64, C.c_int64, C.POINTER(C.c_int64)]
        L.tlc_pd_point_vertices.argtypes = [C.c_int64] + [C.c_void_p] * 14 + [C.c_int64, C.c_void_p]
        L.tlc_pd_filtration_grad.argtypes = [C.c_int64] + [C.c_void_p] * 14 + [C.c_int64, C.c_void_p]
        L.tlc_sliced_w_work_bytes.argtypes = [C.c_int32, C.c_int64, C.c_int64, C.c_int32]
        L.tlc_sliced_w_work_bytes.restype = C.c_int64
        L.tlc_sliced_wasserstein.argtypes = ([C.c_int32] + [C.c_void_p] * 4 + [C.c_int32, C.c_void_p, C.c_double, C.c_int64] + [C.c_void_p] * 5
                                             + [C.c_int64, C.c_void_p])
        L.tlc_w2_large_work_bytes.argtypes, L.tlc_w2_large_work_bytes.restype = [C.c_int64, C.c_int32], C.c_int64
        L.tlc_w2_large_matching.argtypes = ([C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int32]
                                            + [C.c_void_p] * 9 + [C.c_int64, C.c_void_p])
        L.tlc_bottleneck_matching.argtypes = [C.c_int32] + [C.c_void_p] * 4 + [C.c_int32] + [C.c_void_p] * 8
        L.tlc_pi_image_work_bytes.argtypes = [C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_int64)]
        L.tlc_pi_image_work_bytes.restype = C.c_int64
        L.tlc_pi_image.argtypes = ([C.c_int32, C.c_int64] + [C.c_void_p] * 4 + [C.c_int32, C.c_int32] + [C.c_void_p] * 4 + [C.c_int32, C.c_void_p,
                                   C.c_void_p, C.c_int64, C.c_void_p])
        L.tlc_pi_image_vjp.argtypes = ([C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 4
                                       + [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p])
        L.tlc_landscape_work_bytes.argtypes = [C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_int64)]
        L.tlc_landscape_work_bytes.restype = C.c_int64
        L.tlc_landscape.argtypes = ([C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int64] + [C.c_void_p] * 4
                                    + [C.c_int64, C.c_void_p])
        L.tlc_landscape_vjp.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int64] + [C.c_void_p] * 4
        L.tlc_dgm_gram_work_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_uint32, C.POINTER(C.c_int64)]
        L.tlc_dgm_gram_work_bytes.restype = C.c_int64
        L.tlc_dgm_gram.argtypes = ([C.c_int32] + [C.c_void_p] * 3 + [C.c_int32] + [C.c_void_p] * 3 + [C.c_double, C.c_double, C.c_uint32, C.c_int64,
                                   C.c_int64] + [C.c_void_p] * 4 + [C.c_int64, C.c_void_p])
        L.tlc_dgm_gram_vjp.argtypes = ([C.c_int32] + [C.c_void_p] * 3 + [C.c_int32] + [C.c_void_p] * 3 + [C.c_double, C.c_double, C.c_uint32, C.c_int64,
                                       C.c_int64] + [C.c_void_p] * 6 + [C.c_int64, C.c_void_p])
        L.tlc_graph_components_work_bytes.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_int64)]
        L.tlc_graph_components.argtypes = [C.c_void_p] * 3 + [C.c_int64] * 4 + [C.c_void_p] * 5 + [C.c_int64, C.c_void_p]
        # the scratch sizes of the entries that take a bare d_work (csrc/scratch_layouts.h)
        for name, args in (("tlc_gcn2_encode_work_floats", [C.c_int32] * 3), ("tlc_gemm_tn_work_floats", [C.c_int32] * 2),
                           ("tlc_lp_decode_bwd_work_floats", [C.c_int64]), ("tlc_nc_linear_bwd_work_floats", [C.c_int32] * 2),
                           ("tlc_gat_layer_fwd_work_floats", [C.c_int32] * 3), ("tlc_gat_layer_tiled_fwd_work_floats", [C.c_int32] * 2),
                           ("tlc_gat_tile_cut_work_ints", [C.c_int32]), ("tlc_gat_tile_cut_max_tiles", [C.c_int32] * 2),
                           ("tlc_csr_by_target_work_ints", [C.c_int32, C.c_int64]), ("tlc_gat_layer_bwd_work_floats", [C.c_int32] * 3),
                           ("tlc_edge_head_fwd_work_floats", [C.c_int32] * 3), ("tlc_edge_head_bwd_work_floats", [C.c_int64, C.c_int32, C.c_int32])):
            fn = getattr(L, name)
            fn.argtypes, fn.restype = args, C.c_int64
        L.tlc_gnn_layer_fwd.argtypes = ([C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 3
                                        + [C.c_int32, C.c_float] + [C.c_void_p] * 3)
        L.tlc_gnn_layer_bwd_work_bytes.argtypes, L.tlc_gnn_layer_bwd_work_bytes.restype = [C.c_int32] * 3, C.c_int64
        L.tlc_gnn_layer_bwd.argtypes = ([C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float] + [C.c_void_p] * 4 + [C.c_int32, C.c_int32]
                                        + [C.c_void_p] * 2 + [C.c_int32, C.c_float] + [C.c_void_p] * 5 + [C.c_int64, C.c_void_p])
        L.tlc_gnn_stack_fwd.argtypes = ([C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                         C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.POINTER(C.c_float), C.c_void_p, C.c_void_p])
        L.tlc_msg_layer_fwd_work_bytes.argtypes, L.tlc_msg_layer_fwd_work_bytes.restype = [C.c_int32] * 4, C.c_int64
        L.tlc_msg_layer_fwd.argtypes = ([C.c_int32] + [C.c_void_p] * 3 + [C.c_int32, C.c_int32] + [C.c_void_p] * 4 + [C.c_int32, C.c_int32, C.c_float,
                                        C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p])
        L.tlc_msg_layer_bwd_work_bytes.argtypes, L.tlc_msg_layer_bwd_work_bytes.restype = [C.c_int32, C.c_int64] + [C.c_int32] * 3, C.c_int64
        L.tlc_msg_layer_bwd.argtypes = ([C.c_int32] + [C.c_void_p] * 6 + [C.c_int32, C.c_int32] + [C.c_void_p] * 3 + [C.c_int32, C.c_int32, C.c_float]
                                        + [C.c_void_p] * 8 + [C.c_int64, C.c_void_p])
        L.tlc_debug_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
        L.tlc_debug_dc_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.tlc_debug_tier_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.tlc_debug_chunk_counters.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        L.tlc_debug_phase_profile.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]
        _lib = L
    return _lib


def hks_sparse_terms(t):
    """tlc_hks_sparse_terms in Python, operation for operation (IEEE double +, *, / only): the number of Taylor terms K of the sparse HKS
    tier at diffusion time t -- the least k with k + 2 > t / 2 whose bound on the Poisson(t / 2) tail beyond k is <= 2^-64; -1 for a
    time outside [0, HKS_SPARSE_TIME_MAX]."""
    t = float(t)
    if not 0.0 <= t <= HKS_SPARSE_TIME_MAX:
        return -1
    tau = t * 0.5
    if tau == 0.0:
        return 0
    E = term = 1.0
    for j in range(1, 401):
        term = term * tau / float(j)
        E = E + term
    bound, slack = 1.0 / 18446744073709551616.0, 1.0 + 1.0 / 1099511627776.0
    term = 1.0
    for k in range(1000):
        term = term * tau / float(k + 1)
        if float(k + 2) > tau and term / (1.0 - tau / float(k + 2)) / E * slack <= bound:
            return k
    return -1


def check(rc, what=""):
    if rc != OK:
        msg = lib().tlc_last_error().decode("utf-8", "replace")
        raise TlcError("%s: %s (%s)" % (what or "libtlcgnn_hip", ERRORS.get(rc, rc), msg))


def require_gpu():
    import torch
    if not torch.cuda.is_available():
        raise TlcError("no MI355X/HIP device visible: the TLC-GNN hot path has no CPU fallback")
    return torch


def stream_ptr(device=None):
    """torch's current stream ON `device` (default: torch's current device) -- a stream belongs to one device."""
    import torch
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def on_device_of(fn):
    """Decorator for the pointer-only entry points (no handle, so the library cannot know the device): run the call with the
    device of its first CUDA tensor argument current, so the stream handed over and the temporaries belong to the device
    that owns the pointers; the caller's current device is restored on exit."""
    import functools

    @functools.wraps(fn)
    def wrapped(*args, **kwargs):
        import torch
        for a in list(args) + list(kwargs.values()):
            if isinstance(a, torch.Tensor) and a.is_cuda:
                if a.device.index != torch.cuda.current_device():
                    with torch.cuda.device(a.device):
                        return fn(*args, **kwargs)
                break
        return fn(*args, **kwargs)
    return wrapped


def ptr(t):
    """Device pointer of a torch tensor (or None)."""
    if t is None:
        return None
    assert t.is_contiguous()
    return C.c_void_p(t.data_ptr())

"""Scratch sizes of the entries that take a bare d_work pointer, pinned (no GPU).  The tlc_*_work_floats / tlc_*_work_ints functions
return the `total` of the layouts in csrc/scratch_layouts.h, which the launches carve and ops.py allocates by.  The literals are the
element counts that include/tlcgnn.h documented as formulas, and ops.py restated, before the layouts existed (commit 46b31dd);
those of tlc_pdgnn_forward_work_bytes were printed from that commit's build.  Integers, so there is no tolerance: a change here
changes what callers must allocate, not a refactor."""
import pytest

from tlc_gnn_amd import _lib

NS = (0, 1, 135, 136, 200000)                                          # columns of the two layer tables: n_nodes
GAT_FWD = {                                                            # (c_in, c_out): n (3 c_out + 4) + c_in c_out + c_out (2 c_out + 4)
    (1, 8): (168, 196, 3948, 3976, 5600168),
    (1, 16): (592, 644, 7612, 7664, 10400592),
    (1, 32): (2208, 2308, 15708, 15808, 20002208),
    (1, 64): (8512, 8708, 34972, 35168, 39208512),
    (3, 8): (184, 212, 3964, 3992, 5600184),
    (3, 16): (624, 676, 7644, 7696, 10400624),
    (3, 32): (2272, 2372, 15772, 15872, 20002272),
    (3, 64): (8640, 8836, 35100, 35296, 39208640),
    (64, 8): (672, 700, 4452, 4480, 5600672),
    (64, 16): (1600, 1652, 8620, 8672, 10401600),
    (64, 32): (4224, 4324, 17724, 17824, 20004224),
    (64, 64): (12544, 12740, 39004, 39200, 39212544),
}
GAT_BWD = {                                       # n (8 c_out + 5) + 2 c_out^2 + c_in c_out + 4 + c_out (2 c_out + 4)
    (1, 8): (300, 369, 9615, 9684, 13800300),
    (1, 16): (1108, 1241, 19063, 19196, 26601108),
    (1, 32): (4260, 4521, 39495, 39756, 52204260),
    (1, 64): (16708, 17225, 86503, 87020, 103416708),
    (3, 8): (316, 385, 9631, 9700, 13800316),
    (3, 16): (1140, 1273, 19095, 19228, 26601140),
    (3, 32): (4324, 4585, 39559, 39820, 52204324),
    (3, 64): (16836, 17353, 86631, 87148, 103416836),
    (64, 8): (804, 873, 10119, 10188, 13800804),
    (64, 16): (2116, 2249, 20071, 20204, 26602116),
    (64, 32): (6276, 6537, 41511, 41772, 52206276),
    (64, 64): (20740, 21257, 90535, 91052, 103420740),
}
GAT_TILED = {(1, 8): 212, (1, 16): 668, (1, 32): 2348, (1, 64): 8780, (3, 8): 268, (3, 16): 772, (3, 32): 2548, (3, 64): 9172,
             (64, 8): 1976, (64, 16): 3944, (64, 32): 8648, (64, 64): 21128}
# every other function: {its arguments: count}, with 0, 1 and one six-digit size
OTHERS = {
    "tlc_gemm_tn_work_floats": {(1, 1): 32, (5, 5): 800, (25, 41): 32800, (256, 128): 1048576},
    "tlc_nc_linear_bwd_work_floats": {(0, 0): 0, (1, 0): 32, (1, 1): 32, (7, 3): 672, (3, 7): 672, (123457, 3): 11851872},
    "tlc_lp_decode_bwd_work_floats": {(0,): 550912, (1,): 550928, (123457,): 2526224},
    "tlc_gcn2_encode_work_floats": {(0, 32, 16): 12, (0, 6, 16): 12, (0, 32, 7): 12, (1, 32, 16): 92, (1, 6, 16): 40, (1, 32, 7): 83,
                                    (123457, 32, 16): 9876572, (123457, 6, 16): 3456808, (123457, 32, 7): 8765459},
    "tlc_gat_tile_cut_work_ints": {(0,): 6, (1,): 6, (123457,): 3864},
    "tlc_gat_tile_cut_max_tiles": {(0, 192): 3, (0, 2): 3, (1, 192): 3, (1, 2): 4, (123457, 192): 1289, (123457, 2): 123460},
    "tlc_csr_by_target_work_ints": {(0, 0): 0, (1, 0): 3, (1, 1): 4, (123457, 654321): 1024692},
    "tlc_edge_head_fwd_work_floats": {(0, 16, 32): 1024, (0, 32, 32): 2048, (1, 16, 32): 1088, (1, 32, 32): 2112,
                                      (123457, 16, 32): 7902272, (123457, 32, 32): 7903296},
    "tlc_edge_head_bwd_work_floats": {(0, 16, 32): 0, (0, 32, 64): 0, (1, 16, 32): 96, (1, 32, 64): 192,
                                      (123457, 16, 32): 11851872, (123457, 32, 64): 23703744},
}
PDGNN = {(1, 1): 115200, (44, 200): 152576, (45, 200): 153600, (192, 1000): 345088, (193, 1000): 346368,       # hidden = 32
         (200000, 1200000): 263328768}
NEGATIVE = {
    "tlc_gemm_tn_work_floats": ((-1, 1), (1, -1)),
    "tlc_nc_linear_bwd_work_floats": ((-1, 1), (1, -1)),
    "tlc_lp_decode_bwd_work_floats": ((-1,),),
    "tlc_gcn2_encode_work_floats": ((-1, 32, 16), (1, -32, 16), (1, 32, -16)),
    "tlc_gat_layer_fwd_work_floats": ((-1, 64, 32), (1, -64, 32), (1, 64, -32)),
    "tlc_gat_layer_bwd_work_floats": ((-1, 64, 32), (1, -64, 32), (1, 64, -32)),
    "tlc_gat_layer_tiled_fwd_work_floats": ((-64, 32), (64, -32)),
    "tlc_gat_tile_cut_work_ints": ((-1,),),
    "tlc_gat_tile_cut_max_tiles": ((-1, 192), (1, -192), (1, 0)),
    "tlc_csr_by_target_work_ints": ((-1, 1), (1, -1)),
    "tlc_edge_head_fwd_work_floats": ((-1, 16, 32), (1, -16, 32), (1, 16, -32)),
    "tlc_edge_head_bwd_work_floats": ((-1, 16, 32), (1, -16, 32), (1, 16, -32)),
}


@pytest.mark.parametrize("c_in,c_out", sorted(GAT_FWD))
def test_gat_layer(c_in, c_out):
    L = _lib.lib()
    assert tuple(L.tlc_gat_layer_fwd_work_floats(n, c_in, c_out) for n in NS) == GAT_FWD[c_in, c_out]
    assert tuple(L.tlc_gat_layer_bwd_work_floats(n, c_in, c_out) for n in NS) == GAT_BWD[c_in, c_out]
    assert L.tlc_gat_layer_tiled_fwd_work_floats(c_in, c_out) == GAT_TILED[c_in, c_out]


@pytest.mark.parametrize("name", sorted(OTHERS))
def test_others(name):
    fn = getattr(_lib.lib(), name)
    assert {args: fn(*args) for args in OTHERS[name]} == OTHERS[name]


@pytest.mark.parametrize("n,E", sorted(PDGNN))
def test_pdgnn_forward(n, E):
    assert _lib.lib().tlc_pdgnn_forward_work_bytes(n, E, 32) == PDGNN[n, E]


@pytest.mark.parametrize("name", sorted(NEGATIVE))
def test_negative_size(name):
    fn = getattr(_lib.lib(), name)
    assert [fn(*args) for args in NEGATIVE[name]] == [-1] * len(NEGATIVE[name])


def test_every_size_function_is_covered():
    named = {s for s in _lib.SYMBOLS if s.endswith(("_work_floats", "_work_ints", "_max_tiles"))} - {"tlc_nc_group_work_ints"}
    assert named == set(NEGATIVE) == set(OTHERS) | {"tlc_gat_layer_fwd_work_floats", "tlc_gat_layer_bwd_work_floats",
                                                     "tlc_gat_layer_tiled_fwd_work_floats"}

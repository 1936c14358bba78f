"""Host-side checks of tlc_binary_rank_metrics (csrc/lp_metrics.hip): workspace sizes and argument errors, which are decided before
anything touches a device."""
import ctypes as C

import numpy as np

CAP = 16384                      # include/tlcgnn.h TLC_RANK_LDS_CAP


def _work_bytes(L, seg_ptr, score_dtype=0, flags=0):
    sp = np.asarray(seg_ptr, dtype=np.int64)
    return L.tlc_binary_rank_metrics_work_bytes(sp.ctypes.data_as(C.c_void_p), len(sp) - 1, score_dtype, flags)


def test_work_bytes_follow_the_tiers():
    from tlc_gnn_amd import _lib
    L = _lib.lib()
    assert _work_bytes(L, [0, 4432, 8864]) == 0                   # LDS tier only: no workspace
    assert _work_bytes(L, [0, CAP]) == 0
    f32, f64 = _work_bytes(L, [0, CAP + 1]), _work_bytes(L, [0, CAP + 1], 1)
    assert 0 < f32 < f64                                          # u32 keys for f32 scores, u64 for f64
    assert _work_bytes(L, [0, 5, 5 + CAP + 1]) == f32             # the largest radix segment decides
    assert _work_bytes(L, [0, 5], 0, 1) > 0                       # TLC_RANK_FORCE_RADIX
    assert _work_bytes(L, [0, 0], 0, 1) == 0                      # an empty segment stays in the LDS tier
    assert _work_bytes(L, [0, 1 << 24]) >= (1 << 24) * 10


def test_malformed_arguments_are_refused():
    from tlc_gnn_amd import _lib
    L = _lib.lib()
    for bad in ([0, 6, 4], [-1, 5], [3, 2]):
        assert _work_bytes(L, bad) == -1
    assert _work_bytes(L, [0, 5], 0, 2) == -1                     # unknown flag
    assert _work_bytes(L, [0, 5], 2) == -1                        # unknown score dtype
    assert _work_bytes(L, [0, 1 << 31]) == -1                     # segment too long
    one = C.c_void_p(8)                                           # never dereferenced: the checks come first
    sp = np.asarray([0, 6, 4], dtype=np.int64)
    rc = L.tlc_binary_rank_metrics(one, 0, one, 0, sp.ctypes.data_as(C.c_void_p), 2, 0, one, one, one, one, one, None, 0, None)
    assert rc == 1                                                # TLC_ERR_INVALID_ARG
    assert b"seg_ptr" in L.tlc_last_error()
    sp = np.asarray([0, 10], dtype=np.int64)
    assert L.tlc_binary_rank_metrics(one, 3, one, 0, sp.ctypes.data_as(C.c_void_p), 1, 0, one, one, one, one, one, None, 0, None) == 4
    assert L.tlc_binary_rank_metrics(one, 0, one, 9, sp.ctypes.data_as(C.c_void_p), 1, 0, one, one, one, one, one, None, 0, None) == 4
    sp = np.asarray([0, 1 << 31], dtype=np.int64)
    assert L.tlc_binary_rank_metrics(one, 0, one, 0, sp.ctypes.data_as(C.c_void_p), 1, 0, one, one, one, one, one, None, 0, None) == 4
    sp = np.asarray([0, CAP + 1], dtype=np.int64)                 # radix tier without its workspace
    assert L.tlc_binary_rank_metrics(one, 0, one, 0, sp.ctypes.data_as(C.c_void_p), 1, 0, one, one, one, one, one, None, 0, None) == 1

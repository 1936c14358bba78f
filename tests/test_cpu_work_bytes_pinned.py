"""Workspace sizes of the whole-device classes, pinned (no GPU).  The four `*_work_bytes` entries are host arithmetic that callers
allocate by; the launches inside carve the same bytes.  The literals below are what the library returned before the carving and the
radix scratch sizes moved into csrc/tlc_common.h and csrc/radix_passes.h (commit 553b44b, printed from its build): integers, so
there is no tolerance, and a change here is a change of the ABI's behaviour, not a refactor."""
import ctypes as C

import pytest

from tlc_gnn_amd import _lib

SIZES = ((1, 0), (2049, 2048), (5000, 20000), (65536, 65535), (1 << 20, 1 << 22))      # (nodes, edges)
PD_WIDE = dict(zip(SIZES, (15616, 770304, 6657280, 24140032, 1393638656)))
PD_GRAD = dict(zip(SIZES, (0, 203776, 977920, 6392832, 204476416)))
SLICED_W = {                                                                            # (max_points, n_dirs)
    (2049, 1): 140800, (2049, 8): 1094144, (2049, 128): 17448704,
    (4096, 1): 275968, (4096, 8): 2182912, (4096, 128): 34873856,
    (4097, 1): 276992, (4097, 8): 2183936, (4097, 128): 34883328,
    (100000, 1): 6654464, (100000, 8): 53210112, (100000, 128): 851304448,
}
RANK = {                                                                                # (scores of the one segment, TLC_SCORE_*)
    (16385, 0): 173056, (16385, 1): 304128,
    (1 << 24, 0): 172213504, (1 << 24, 1): 306431232,
}


@pytest.mark.parametrize("n,m", SIZES)
def test_pd_wide(n, m):
    need = C.c_int64(-1)
    assert _lib.lib().tlc_pd_wide_work_bytes((C.c_int64 * 1)(n), (C.c_int64 * 1)(m), C.c_int64(1), C.byref(need)) == 0
    assert need.value == PD_WIDE[n, m]


@pytest.mark.parametrize("n,m", SIZES)
def test_pd_grad(n, m):
    need = C.c_int64(-1)
    assert _lib.lib().tlc_pd_grad_work_bytes(C.c_int64(n), C.c_int64(m), C.byref(need)) == 0
    assert need.value == PD_GRAD[n, m]


@pytest.mark.parametrize("max_points,n_dirs", sorted(SLICED_W))
def test_sliced_w(max_points, n_dirs):
    got = _lib.lib().tlc_sliced_w_work_bytes(C.c_int32(1), C.c_int64(max_points), C.c_int64(max_points), C.c_int32(n_dirs))
    assert got == SLICED_W[max_points, n_dirs]


@pytest.mark.parametrize("scores,dtype", sorted(RANK))
def test_binary_rank_metrics(scores, dtype):
    seg = (C.c_int64 * 2)(0, scores)
    assert _lib.lib().tlc_binary_rank_metrics_work_bytes(seg, C.c_int32(1), C.c_int(dtype), C.c_uint32(0)) == RANK[scores, dtype]

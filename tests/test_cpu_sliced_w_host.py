"""Host side of tlc_sliced_wasserstein (no GPU): the exported symbols, the mirrored constants, the reference's directions, the workspace
arithmetic, what the entry refuses before it reads a pointer and what the wrappers refuse before they call it."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import sliced_w_cases as cases
from tlc_gnn_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1                                           # TLC_ERR_INVALID_ARG
NAMES = ("tlc_sliced_w_work_bytes", "tlc_sliced_wasserstein")
LDS_NMAX, MAX_DIRS = _lib.SW_LDS_NMAX, _lib.SW_MAX_DIRS


def need(n_problems, total, max_points, n_dirs):
    return _lib.lib().tlc_sliced_w_work_bytes(C.c_int32(n_problems), C.c_int64(total), C.c_int64(max_points), C.c_int32(n_dirs))


def call(n_problems=1, n_dirs=4, max_points=10, work_bytes=0, ptr=0x1000, work=0x1000, null_at=None):
    """tlc_sliced_wasserstein with made-up device pointers: every case here must be refused (or be done) before one of them is read.
    null_at: which of (xoff, X, yoff, Y, dirs, loss, gradX, gradY, status) is NULL."""
    p = [C.c_void_p(ptr) for _ in range(9)]
    if null_at is not None:
        p[null_at] = None
    return _lib.lib().tlc_sliced_wasserstein(C.c_int32(n_problems), p[0], p[1], p[2], p[3], C.c_int32(n_dirs), p[4], C.c_double(0.25),
                                             C.c_int64(max_points), p[5], p[6], p[7], p[8], C.c_void_p(work), C.c_int64(work_bytes), None)


def test_symbols_and_constants():
    L = _lib.lib()
    for name in NAMES:
        assert hasattr(L, name) and name in _lib.SYMBOLS, name
    header = open(os.path.join(ROOT, "include", "tlcgnn.h")).read()
    cut = {k: int(v) for k, v in re.findall(r"#define\s+TLC_SW_(\w+)\s+(\d+)", header)}
    assert cut == {"WAVE_NMAX": _lib.SW_WAVE_NMAX, "LDS_NMAX": _lib.SW_LDS_NMAX, "MAX_DIRS": _lib.SW_MAX_DIRS}
    assert _lib.SW_WAVE_NMAX == 64 and _lib.SW_LDS_NMAX >= 2048
    assert (cases.WAVE_NMAX, cases.LDS_NMAX, cases.MAX_DIRS) == (_lib.SW_WAVE_NMAX, _lib.SW_LDS_NMAX, MAX_DIRS)
    # both lists as (8-byte key, 2-byte index) and two sign bytes per element fit the 160 KiB of LDS
    assert _lib.SW_LDS_NMAX * (2 * 10 + 2) <= 160 * 1024


def test_directions_equal_the_literal_loop():
    M = 50
    want = []
    theta = 0.5
    step = 1.0 / M
    for i in range(M):
        want.append([float(np.float32(np.cos(theta * np.pi))), float(np.float32(np.sin(theta * np.pi)))])
        theta += step
    dirs, scale = ops.sliced_directions(M)
    assert dirs.dtype == np.float64 and dirs.shape == (M, 2) and scale == step == 0.02
    assert np.array_equal(dirs, np.array(want))
    assert np.array_equal(dirs, dirs.astype(np.float32).astype(np.float64))          # float32 values, widened
    assert dirs[0, 0] == float(np.float32(np.cos(np.pi / 2))) and dirs[0, 1] == 1.0
    assert ops.sliced_directions()[0].shape == (50, 2)
    with pytest.raises(ValueError):
        ops.sliced_directions(0)


def test_directions_of_an_exact_step():
    """1 / 64 is exact, so the accumulated theta is exactly 0.5 + i / 64"""
    dirs, scale = ops.sliced_directions(64)
    assert scale == 1.0 / 64
    for i in range(64):
        theta = 0.5 + i / 64
        assert dirs[i, 0] == float(np.float32(np.cos(theta * np.pi))) and dirs[i, 1] == float(np.float32(np.sin(theta * np.pi))), i
    assert dirs[32, 0] == -1.0                          # theta = 1 exactly


def test_work_bytes_monotone():
    Lmax = LDS_NMAX
    for N in (0, 1, 64, 65, Lmax):
        assert need(5, 10 * N, N, 50) == 0, N
    assert need(1, Lmax + 1, Lmax + 1, 1) > 0
    pts = (0, 64, Lmax, Lmax + 1, 3 * Lmax, 44325 * 2, 1 << 20, (1 << 27) // 50, (1 << 27) // 50 + 1, (1 << 26) - 1, 1 << 26, (1 << 26) + 1,
           1 << 27, (1 << 27) + 5)
    for M in (1, 2, 8, 50, MAX_DIRS):
        seq = [need(1, N, N, M) for N in pts]
        assert seq == sorted(seq) and seq[-1] > 0, (M, seq)
    for N in (Lmax + 1, 3 * Lmax, 88650, 1 << 22, 1 << 27):
        seq = [need(1, N, N, M) for M in range(1, MAX_DIRS + 1)]
        assert seq == sorted(seq), N
        assert seq[0] < seq[-1]
    # the number of problems and the total do not shrink it either
    base = need(1, 5000, 5000, 8)
    assert need(2, 5000, 5000, 8) >= base and need(1000, 5000, 5000, 8) >= base and need(1, 10 ** 9, 5000, 8) >= base
    assert ops.sliced_w_work_bytes(1, 5000, 5000, 8) == base
    # one direction is the least, and 16 bytes of (key, payload) twice over per item is what dominates
    assert need(1, 88650, 88650, 1) >= 2 * 88650 * 32


def test_work_bytes_refusals():
    assert need(-1, 0, 0, 1) == -1
    assert need(1, -1, 0, 1) == -1
    assert need(1, 0, -1, 1) == -1
    assert need(1, 10, 10, 0) == -1
    assert need(1, 10, 10, MAX_DIRS + 1) == -1
    with pytest.raises(_lib.TlcError):
        ops.sliced_w_work_bytes(1, 10, 10, 0)


def test_entry_refusals():
    L = _lib.lib()
    assert call(n_problems=-1) == INVALID
    assert call(max_points=-1) == INVALID
    assert call(work_bytes=-1) == INVALID
    for bad in (0, -3, MAX_DIRS + 1):
        assert call(n_dirs=bad) == INVALID
        assert b"n_dirs" in L.tlc_last_error()
        assert call(n_problems=0, n_dirs=bad) == INVALID            # refused whatever the batch
    for k in (0, 2, 4, 5, 8):                                       # xoff, yoff, dirs, loss, status
        assert call(null_at=k) == INVALID, k
        assert b"null pointer" in L.tlc_last_error()
    # a workspace below one direction of the largest problem: refused at once, and the message names both numbers
    big = _lib.SW_LDS_NMAX + 1
    least = need(1, big, big, 1)
    assert call(max_points=big, work_bytes=least - 1) == INVALID
    msg = L.tlc_last_error().decode()
    assert str(least) in msg and str(least - 1) in msg
    assert call(max_points=big, work_bytes=0, work=None) == INVALID
    assert call(max_points=big, work_bytes=least, work=None) == INVALID       # bytes without a pointer
    # no problem: nothing to do, whatever the pointers
    assert call(n_problems=0, ptr=None, work=None) == 0


def test_wrappers_refuse_offsets_past_the_arrays():
    """the check runs where the offsets live, before a device is asked for: CPU tensors reach it without a GPU"""
    import torch
    from tlc_gnn_amd import autograd
    X, Y = torch.zeros(3, 2, dtype=torch.float64), torch.zeros(2, 2, dtype=torch.float64)
    for xo, yo in (([0, 4], [0, 2]), ([0, 3], [0, 3]), ([0, 2, 5], [0, 1, 2])):
        with pytest.raises(ValueError, match="offsets end at"):
            ops.sliced_wasserstein(torch.tensor(xo), X, torch.tensor(yo), Y, M=3)
        with pytest.raises(ValueError, match="offsets end at"):
            autograd.sliced_diagram_loss(X, Y, M=3, xoff=torch.tensor(xo), yoff=torch.tensor(yo))
    with pytest.raises(ValueError):
        ops.sliced_wasserstein(torch.tensor([0, 3]), X, torch.tensor([0, 1, 2]), Y, M=3)          # two batches of different length
    from tlc_gnn_amd import topo
    with pytest.raises(ValueError):
        topo.sliced_wasserstein_to(None, None, None, None, None, None, which="ord0+rel1")


def test_the_restatement_on_a_case_worked_by_hand():
    """X = {(0, 2)}, Y = {(2, 4)}, direction (1, 1), scale 1: V1 = [2, 6], V2 = [6, 2] -> sorted equal, loss 0.  Direction (1, 0): V1 =
    [0, 3], V2 = [2, 1] -> sorted [0, 3] and [1, 2]: loss 2; the signs at ranks (0, 1) are (-1, +1)."""
    X, Y = np.array([[0.0, 2.0]]), np.array([[2.0, 4.0]])
    loss, gx, gy = cases.restate(X, Y, [[1.0, 1.0]], 1.0)
    assert loss == 0.0 and not gx.any() and not gy.any()
    loss, gx, gy = cases.restate(X, Y, [[1.0, 0.0]], 1.0)
    assert loss == 2.0
    # X's point: V1 element 0 (rank 0, s = -1) contributes -1 * t; its diagonal element sits in V2 at listing 1 (value 1, rank 0, s = -1):
    # minus (-1) * sigma * u with u = 0.5
    assert gx.tolist() == [[-1.0 + 0.5, 0.0 + 0.5]]
    # Y's point: V2 element 0 (value 2, rank 1, s = +1) contributes -(+1) * t; its diagonal element in V1 at listing 1 (value 3, rank 1,
    # s = +1): plus (+1) * tau * u
    assert gy.tolist() == [[-1.0 + 0.5, 0.0 + 0.5]]
    assert cases.exact_loss(*cases.even_grid(np.random.RandomState(0), 5, 3)) == cases.restate(
        *cases.even_grid(np.random.RandomState(0), 5, 3), cases.EXACT_DIRS, cases.EXACT_SCALE)[0]
    assert math.isfinite(loss)

"""Host side of tlc_landscape / tlc_landscape_vjp (no GPU): the restatement of tests/landscape_cases.py against a brute force and
against closed forms, the exported symbols and mirrored constants, the workspace arithmetic, what the entries refuse before they read
a pointer and what the wrappers refuse before they call them."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import landscape_cases as cases
from tlc_gnn_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1                                           # TLC_ERR_INVALID_ARG
NAMES = ("tlc_landscape_work_bytes", "tlc_landscape", "tlc_landscape_vjp")
WAVE_NMAX, LDS_NMAX, KMAX, TMAX = _lib.LS_WAVE_NMAX, _lib.LS_LDS_NMAX, _lib.LS_KMAX, _lib.LS_TMAX


def need(n_dgms, max_points, K, T):
    """-> (full, least)"""
    least = C.c_int64(-7)
    full = _lib.lib().tlc_landscape_work_bytes(C.c_int32(n_dgms), C.c_int64(max_points), C.c_int32(K), C.c_int32(T), C.byref(least))
    return int(full), int(least.value)


def call(n_dgms=1, T=8, K=3, max_points=10, work_bytes=0, ptr=0x1000, work=0x1000, null_at=None):
    """tlc_landscape with made-up device pointers: every case here must be refused (or be done) before one of them is read.
    null_at: which of (offs, pts, ts, out, winner, status) is NULL."""
    p = [C.c_void_p(ptr) for _ in range(6)]
    if null_at is not None:
        p[null_at] = None
    return _lib.lib().tlc_landscape(C.c_int32(n_dgms), p[0], p[1], C.c_int32(T), p[2], C.c_int32(K), C.c_int64(max_points), p[3], p[4], p[5],
                                    C.c_void_p(work) if work else None, C.c_int64(work_bytes), None)


def call_vjp(n_dgms=1, T=8, K=3, max_points=10, ptr=0x1000, null_at=None):
    """tlc_landscape_vjp the same way; null_at: which of (offs, pts, ts, winner, grad_out, grad_pts) is NULL"""
    p = [C.c_void_p(ptr) for _ in range(6)]
    if null_at is not None:
        p[null_at] = None
    return _lib.lib().tlc_landscape_vjp(C.c_int32(n_dgms), p[0], p[1], C.c_int32(T), p[2], C.c_int32(K), C.c_int64(max_points), p[3], p[4],
                                        p[5], None)


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,T,K", [(0, 3, 2), (1, 5, 3), (7, 9, 1), (40, 17, 5), (40, 17, 16), (90, 6, 16)])
def test_restatement_equals_the_brute_force(n, T, K):
    rs = np.random.RandomState(n + T + K)
    for pts, ts in ((cases.random_diagram(rs, n), cases.grid(T)), (cases.integer_diagram(rs, n), cases.integer_grid())):
        out, win, st = cases.restate(pts, ts, K)
        bo, bw = cases.brute(pts, ts, K)
        assert st == 0 and np.array_equal(out.view(np.uint64), bo.view(np.uint64)) and np.array_equal(win, bw)
        assert not np.signbit(out).any() and ((win == -1) == (out == 0)).all()


def test_restatement_on_nested_intervals():
    for N, K in ((1, 1), (5, 3), (5, 8), (12, 5)):
        t, want, wwin = cases.nested_closed_form(N, K)
        out, win, _ = cases.restate(cases.nested(N), t, K)
        assert np.array_equal(out, want) and np.array_equal(win, wwin)
        assert np.array_equal(out, np.round(out))                      # exact integers
        assert out[0, N] == N and (K < 2 or N < 2 or out[1, N] == N - 1)


def test_restatement_on_copies_and_disjoint_intervals():
    N, K = 6, 4
    ts = np.array([0.25, 0.5, 0.75, 1.0, 1.5])
    out, win, _ = cases.restate(np.tile([[0.0, 1.0]], (N, 1)), ts, K)
    inside = np.array([0.25, 0.5, 0.25, 0.0, 0.0])
    assert np.array_equal(out, np.tile(inside, (K, 1)))
    assert np.array_equal(win[:, :3], np.tile(np.arange(K)[:, None], (1, 3))) and (win[:, 3:] == -1).all()
    # disjoint intervals: one point at most is present at any sample
    pts = np.array([[0.0, 1.0], [1.0, 2.0], [2.5, 3.0]])
    ts = np.linspace(-0.5, 3.5, 33)
    out, win, _ = cases.restate(pts, ts, 3)
    assert not out[1:].any() and (win[1:] == -1).all() and out[0].max() == 0.5
    # the gradient of the hand case: the peak goes to the birth, the right flank to the death
    pts, ts = np.array([[1.0, 3.0]]), np.array([1.5, 2.0, 2.5, 3.0])
    out, win, _ = cases.restate(pts, ts, 1)
    assert out.tolist() == [[0.5, 1.0, 0.5, 0.0]] and win.tolist() == [[0, 0, 0, -1]]
    g = cases.restate_vjp(pts, ts, win, np.array([[1.0, 10.0, 100.0, 1000.0]]))
    assert g.tolist() == [[-11.0, 100.0]]
    # a NaN / Inf coordinate
    for bad in (np.nan, np.inf, -np.inf):
        out, win, st = cases.restate(np.array([[0.0, 1.0], [bad, 2.0]]), ts, 2)
        assert st == 3 and np.isnan(out).all() and (win == -1).all()


def test_gradcheck_input_is_found_and_kink_free():
    dgms, ts, draws = cases.gradcheck_input()
    assert draws <= 100 and cases.kink_free(dgms, ts)
    assert not cases.kink_free([np.array([[0.0, 1.0]])], np.array([0.5]))              # a sample on the peak
    assert not cases.kink_free([np.array([[0.0, 1.0], [0.0, 1.0]])], np.array([0.3]))  # two equal values


# ---- the library ----------------------------------------------------------------------------------------------------------------------
def test_symbols_and_constants():
    L = _lib.lib()
    for name in NAMES:
        assert hasattr(L, name) and name in _lib.SYMBOLS, name
        assert getattr(L, name).argtypes is not None, name
    assert L.tlc_landscape_work_bytes.restype is C.c_int64
    assert len(L.tlc_landscape.argtypes) == 13 and len(L.tlc_landscape_vjp.argtypes) == 11
    header = open(os.path.join(ROOT, "include", "tlcgnn.h")).read()
    cut = {k: int(v) for k, v in re.findall(r"#define\s+TLC_LS_(\w+)\s+(\d+)", header)}
    assert cut == {"WAVE_NMAX": WAVE_NMAX, "LDS_NMAX": LDS_NMAX, "KMAX": KMAX, "TMAX": TMAX}
    assert WAVE_NMAX == 64 and KMAX == 16
    # the staged points of the workgroup class, 16 bytes each, leave room for two workgroups per CU (160 KiB of LDS)
    assert LDS_NMAX * 16 <= 80 * 1024
    layouts = open(os.path.join(ROOT, "tlc-gnn_amd", "csrc", "scratch_layouts.h")).read()
    assert re.search(r"struct TlcLandscapeScratch \{\s*static constexpr int64_t SLICE = %d," % LDS_NMAX, layouts)


def test_work_bytes():
    for n in (0, 1, WAVE_NMAX, WAVE_NMAX + 1, LDS_NMAX):
        assert need(5, n, 5, 100) == (0, 0), n
    sizes = (LDS_NMAX + 1, 2 * LDS_NMAX, 2 * LDS_NMAX + 1, 70000, 1 << 20, 1 << 27, (1 << 27) + 5)
    for K, T in ((1, 1), (5, 100), (KMAX, TMAX)):
        full = [need(1, n, K, T)[0] for n in sizes]
        least = [need(1, n, K, T)[1] for n in sizes]
        assert full == sorted(full) and full[0] > 0, (K, T, full)
        assert len(set(least)) == 1 and 0 < least[0] <= full[0], (K, T, least)      # one slice and the running list, whatever n
        assert least[0] >= 2 * K * T * 12
    # monotone in K and in T; two slices in flight need more than one
    assert need(1, 70000, 5, 100)[0] <= need(1, 70000, 6, 100)[0] <= need(1, 70000, 6, 101)[0]     # (arrays round up to 256 bytes)
    assert need(1, 70000, 5, 100)[0] < need(1, 70000, 10, 100)[0] < need(1, 70000, 10, 200)[0]
    assert need(1, 2 * LDS_NMAX + 1, 5, 100)[1] < need(1, 2 * LDS_NMAX + 1, 5, 100)[0]
    assert need(1000, 70000, 5, 100) == need(1, 70000, 5, 100)
    # a NULL least is allowed
    assert _lib.lib().tlc_landscape_work_bytes(C.c_int32(1), C.c_int64(70000), C.c_int32(5), C.c_int32(100), None) == need(1, 70000, 5, 100)[0]
    for bad in ((-1, 10, 5, 100), (1, -1, 5, 100), (1, 10, 0, 100), (1, 10, KMAX + 1, 100), (1, 10, 5, 0), (1, 10, 5, TMAX + 1)):
        assert need(*bad)[0] == -1, bad
    from tlc_gnn_amd import engine
    assert engine.landscape_work_bytes(1, 70000, 5, 100) == need(1, 70000, 5, 100)
    with pytest.raises(_lib.TlcError):
        engine.landscape_work_bytes(1, 10, 0, 100)


def test_entry_refusals():
    L = _lib.lib()
    for fn in (call, call_vjp):
        assert fn(n_dgms=-1) == INVALID
        assert fn(max_points=-1) == INVALID
        for bad in (0, -2, KMAX + 1):
            assert fn(K=bad) == INVALID and b"K outside" in L.tlc_last_error()
            assert fn(n_dgms=0, K=bad) == INVALID                       # refused whatever the batch
        for bad in (0, -2, TMAX + 1):
            assert fn(T=bad) == INVALID and b"T outside" in L.tlc_last_error()
        assert fn(n_dgms=0, ptr=None) == 0                              # no diagram: nothing to do, whatever the pointers
    assert call(work_bytes=-1) == INVALID
    for k in (0, 1, 2, 3, 5):                                           # offs, pts, ts, out, status (winner may be NULL)
        assert call(null_at=k) == INVALID, k
        assert b"null pointer" in L.tlc_last_error()
    for k in range(6):                                                  # offs, pts, ts, winner, grad_out, grad_pts
        assert call_vjp(null_at=k) == INVALID, k
        assert b"null pointer" in L.tlc_last_error()
    # a workspace below the least of the largest diagram: refused at once, and the message names both numbers
    big = LDS_NMAX + 1
    full, least = need(1, big, 3, 8)
    assert call(max_points=big, work_bytes=least - 1) == INVALID
    msg = L.tlc_last_error().decode()
    assert str(least) in msg and str(least - 1) in msg
    assert call(max_points=big, work_bytes=0, work=None) == INVALID
    assert call(max_points=big, work_bytes=least, work=None) == INVALID     # bytes without a pointer


def test_wrappers_refuse_before_they_call():
    """the checks run on the arguments, before a device is asked for: CPU tensors reach them without a GPU"""
    import torch
    from tlc_gnn_amd import autograd, ops, topo
    pts, offs = torch.zeros(3, 2, dtype=torch.float64), torch.tensor([0, 3])
    ts = torch.linspace(0, 1, 8, dtype=torch.float64)
    for fn in (lambda **kw: autograd.diagram_landscape(pts, offs, **kw), lambda **kw: topo.landscapes(None, None, None, None, **kw)):
        with pytest.raises(ValueError, match="1-D"):
            fn(ts=ts.reshape(2, 4), K=2)
        with pytest.raises(ValueError, match="requires grad"):
            fn(ts=ts.clone().requires_grad_(True), K=2)
        for K in (0, KMAX + 1):
            with pytest.raises(ValueError, match="K = "):
                fn(ts=ts, K=K)
        for T in (0, TMAX + 1):
            with pytest.raises(ValueError, match="samples"):
                fn(ts=torch.zeros(T, dtype=torch.float64), K=2)
    with pytest.raises(ValueError, match="1-D"):
        ops.landscape(pts, offs, ts.reshape(2, 4), K=2)
    with pytest.raises(ValueError, match="K = "):
        ops.landscape(pts, offs, ts, K=KMAX + 1)
    with pytest.raises(ValueError, match="samples"):
        ops.landscape(pts, offs, torch.zeros(TMAX + 1, dtype=torch.float64), K=2)
    with pytest.raises(ValueError, match="offsets end at"):
        ops.landscape(pts, torch.tensor([0, 4]), ts, K=2)
    with pytest.raises(ValueError, match="which"):
        topo.landscapes(None, None, None, None, ts, which="ord0+rel1")

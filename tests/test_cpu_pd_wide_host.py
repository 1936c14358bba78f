"""Host side of tlc_pd_wide (no GPU): the exported symbols, the workspace arithmetic and what the two entries refuse before they
touch the device."""
import ctypes as C

import pytest

from tlc_gnn_amd import _lib, engine


def work_bytes(nodes, edges):
    need = C.c_int64(-1)
    S = len(nodes)
    rc = _lib.lib().tlc_pd_wide_work_bytes((C.c_int64 * max(S, 1))(*nodes), (C.c_int64 * max(S, 1))(*edges), C.c_int64(S), C.byref(need))
    return rc, need.value


def call(n_graphs=1, sel=(0,), work_bytes=1 << 20, flags=0, ptr=0x1000, n_sel=None, work=0x1000):
    """tlc_pd_wide with made-up device pointers: every case here must be refused before one of them is read"""
    S = len(sel)
    p = C.c_void_p(ptr)
    return _lib.lib().tlc_pd_wide(C.c_int64(n_graphs), p, p, p, p, C.c_uint32(flags), (C.c_int64 * max(S, 1))(*sel),
                                  C.c_int64(S if n_sel is None else n_sel), p, p, p, p, p, None, C.c_void_p(work), C.c_int64(work_bytes),
                                  None, None)


def test_symbols_and_constants():
    L = _lib.lib()
    assert hasattr(L, "tlc_pd_wide") and hasattr(L, "tlc_pd_wide_work_bytes")
    assert "tlc_pd_wide" in _lib.SYMBOLS and "tlc_pd_wide_work_bytes" in _lib.SYMBOLS
    assert _lib.PD_WIDE_SORT_TILE == 16 * _lib.PD_WIDE_BLOCK and _lib.PD_WIDE_SCAN_CHUNK == 8 * _lib.PD_WIDE_BLOCK


def test_work_bytes_is_monotone():
    assert work_bytes([], []) == (0, 0)
    last = 0
    for n, m in ((1, 0), (2, 1), (100, 99), (100, 300), (5000, 300), (5000, 20000), (19717, 44324), (200000, 300000), (1 << 20, 1 << 22)):
        rc, b = work_bytes([n], [m])
        assert rc == 0 and b > last, (n, m, b, last)
        assert work_bytes([n + 1], [m])[1] >= b and work_bytes([n], [m + 1])[1] >= b
        last = b
    # the largest graph of a selection decides
    assert work_bytes([100, 5000, 7], [300, 20000, 3])[1] == work_bytes([5000], [20000])[1]
    assert engine.pd_wide_work_bytes([5000], [20000]) == work_bytes([5000], [20000])[1]


def test_work_bytes_refusals():
    L = _lib.lib()
    one = (C.c_int64 * 1)(5)
    need = C.c_int64(0)
    assert L.tlc_pd_wide_work_bytes(one, one, C.c_int64(1), None) == 1                       # TLC_ERR_INVALID_ARG
    assert L.tlc_pd_wide_work_bytes(None, one, C.c_int64(1), C.byref(need)) == 1
    assert L.tlc_pd_wide_work_bytes(one, None, C.c_int64(1), C.byref(need)) == 1
    assert L.tlc_pd_wide_work_bytes(one, one, C.c_int64(-1), C.byref(need)) == 1
    assert work_bytes([-1], [3])[0] == 1 and work_bytes([3], [-1])[0] == 1
    top = _lib.PD_WIDE_MAX_ITEMS
    assert work_bytes([top - 10], [10])[0] == 0
    assert work_bytes([top - 10], [11])[0] == 4                                              # TLC_ERR_UNSUPPORTED
    assert work_bytes([1], [top])[0] == 4 and work_bytes([1 << 40], [0])[0] == 4
    assert b"TLC_PD_WIDE_MAX_ITEMS" in L.tlc_last_error()


def test_entry_refusals():
    L = _lib.lib()
    assert call(n_graphs=-1) == 1
    assert call(n_sel=-1) == 1
    assert call(work_bytes=-1) == 1
    assert call(sel=(1,)) == 1 and call(sel=(-1,)) == 1                                       # outside 0 .. n_graphs-1
    assert call(flags=0x2) == 1                                                               # not a flag of this entry
    assert call(ptr=None) == 1 and call(work=None) == 1
    p = C.c_void_p(0x1000)
    assert L.tlc_pd_wide(C.c_int64(1), p, p, p, p, C.c_uint32(0), None, C.c_int64(1), p, p, p, p, p, None, p, C.c_int64(1 << 20), None, None) == 1
    # a workspace below the smallest graph's: refused at once, and the message names the bytes needed
    least = work_bytes([1], [0])[1]
    assert call(work_bytes=least - 1) == 1
    msg = L.tlc_last_error().decode()
    assert str(least) in msg and str(least - 1) in msg
    # nothing selected: nothing to do, whatever the pointers
    assert call(sel=(), ptr=None, work=None, work_bytes=0) == 0
    # the debug bit belongs to this entry alone
    assert L.tlc_pd_from_filtration(C.c_int32(1), p, p, p, p, C.c_uint32(_lib.PD_WIDE_FORCE_FALLBACK), p, p, p, p, p, None, None) == 1


def test_check_pd_large():
    assert engine.check_pd_large("host") == "host" and engine.check_pd_large("device") == "device"
    for bad in ("gpu", "", None, True, "Device"):
        with pytest.raises(ValueError):
            engine.check_pd_large(bad)

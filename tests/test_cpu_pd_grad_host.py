"""Host side of tlc_pd_point_vertices / tlc_pd_filtration_grad (no GPU): the exported symbols, the mirrored cut constants, the
workspace arithmetic and what the entries refuse before they read a pointer."""
import ctypes as C
import os
import re

import pytest

from tlc_gnn_amd import _lib, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1                                           # TLC_ERR_INVALID_ARG
NAMES = ("tlc_pd_grad_work_bytes", "tlc_pd_point_vertices", "tlc_pd_filtration_grad")


def work_bytes(n, m):
    need = C.c_int64(-1)
    rc = _lib.lib().tlc_pd_grad_work_bytes(C.c_int64(n), C.c_int64(m), C.byref(need))
    return rc, need.value


def vertices(n_graphs=1, work_bytes=0, ptr=0x1000, work=0x1000, null_at=None):
    """tlc_pd_point_vertices with made-up device pointers: every case here must be refused (or be done) before one of them is read.
    null_at: the index (0 .. 12) of the one required pointer that is NULL."""
    p = [C.c_void_p(ptr) for _ in range(13)]
    if null_at is not None:
        p[null_at] = None
    return _lib.lib().tlc_pd_point_vertices(C.c_int64(n_graphs), *p, C.c_void_p(work), C.c_int64(work_bytes), None)


GRAD_REQUIRED = (0, 1, 2, 3, 4, 5, 6, 11, 12)         # offsets, counts, the four id arrays, status, grad_f; 7 .. 10 are the gradients


def grad(n_graphs=1, work_bytes=0, ptr=0x1000, work=0x1000, null_at=None):
    p = [C.c_void_p(ptr) for _ in range(13)]
    if null_at is not None:
        p[null_at] = None
    return _lib.lib().tlc_pd_filtration_grad(C.c_int64(n_graphs), *p, C.c_void_p(work), C.c_int64(work_bytes), None)


def test_symbols_and_constants():
    L = _lib.lib()
    for name in NAMES:
        assert hasattr(L, name) and name in _lib.SYMBOLS, name
    header = open(os.path.join(ROOT, "include", "tlcgnn.h")).read()
    cut = {k: int(v) for k, v in re.findall(r"#define\s+TLC_PD_VERT_(\w+)\s+(\d+)", header)}
    assert cut == {"WAVE_NMAX": _lib.PD_VERT_WAVE_NMAX, "LDS_NMAX": _lib.PD_VERT_LDS_NMAX}
    assert _lib.PD_VERT_WAVE_NMAX == 64 and _lib.PD_VERT_LDS_NMAX == _lib.PD_L_NMAX


def test_work_bytes():
    # nothing up to the LDS class, whatever the edges
    for n, m in ((0, 0), (1, 0), (64, 10 ** 6), (65, 100), (_lib.PD_VERT_LDS_NMAX, 1 << 24)):
        assert work_bytes(n, m) == (0, 0), (n, m)
    last = 0
    for n, m in ((2049, 0), (2049, 2048), (3000, 2048), (5000, 20000), (19717, 44324), (65536, 65535), (1 << 20, 1 << 22)):
        rc, b = work_bytes(n, m)
        assert rc == 0 and b > last, (n, m, b, last)
        assert work_bytes(n + 1, m)[1] >= b and work_bytes(n, m + 1)[1] >= b
        last = b
    # monotone across the cut and up to (and beyond) the size limit
    top = _lib.PD_WIDE_MAX_ITEMS
    seq = [work_bytes(n, 3000)[1] for n in (0, 64, 65, 2048, 2049, 4096, 1 << 16, 1 << 22, top - 3000, top, top + 5)]
    assert seq == sorted(seq)
    seq = [work_bytes(3000, m)[1] for m in (0, 1, 4096, 4097, 1 << 16, 1 << 22, top - 3000, top)]
    assert seq == sorted(seq)
    assert engine.pd_grad_work_bytes(5000, 20000) == work_bytes(5000, 20000)[1]


def test_work_bytes_refusals():
    L = _lib.lib()
    need = C.c_int64(0)
    assert L.tlc_pd_grad_work_bytes(C.c_int64(5000), C.c_int64(5000), None) == INVALID
    assert L.tlc_pd_grad_work_bytes(C.c_int64(-1), C.c_int64(5), C.byref(need)) == INVALID
    assert L.tlc_pd_grad_work_bytes(C.c_int64(5), C.c_int64(-1), C.byref(need)) == INVALID


@pytest.mark.parametrize("entry,required", [(vertices, tuple(range(13))), (grad, GRAD_REQUIRED)], ids=["vertices", "grad"])
def test_entry_refusals(entry, required):
    L = _lib.lib()
    assert entry(n_graphs=-1) == INVALID
    assert entry(work_bytes=-1) == INVALID
    assert entry(n_graphs=0, work_bytes=-1) == INVALID
    for k in required:
        assert entry(null_at=k) == INVALID, k
        assert b"null pointer" in L.tlc_last_error()
    # a workspace that could not hold the smallest graph that needs one: refused at once, and the message names both numbers
    least = work_bytes(_lib.PD_VERT_LDS_NMAX + 1, 0)[1]
    assert least > 0
    assert entry(work_bytes=least - 1) == INVALID
    msg = L.tlc_last_error().decode()
    assert str(least) in msg and str(least - 1) in msg
    assert entry(work_bytes=least, work=None) == INVALID                     # bytes without a pointer
    # no graph: nothing to do, whatever the pointers
    assert entry(n_graphs=0, ptr=None, work=None, work_bytes=0) == 0
    assert entry(n_graphs=0, ptr=None, work=None, work_bytes=1 << 20) == 0


def test_optional_gradients_are_not_required():
    # (the call itself would go on to read the offsets: only the order of the checks is visible here -- a NULL gradient with a NULL
    # required pointer is refused for the required one)
    L = _lib.lib()
    p = [C.c_void_p(0x1000)] * 7 + [None] * 4 + [None, C.c_void_p(0x1000)]
    assert L.tlc_pd_filtration_grad(C.c_int64(1), *p, None, C.c_int64(0), None) == INVALID
    assert b"null pointer" in L.tlc_last_error()


def test_topo_rejects_an_unknown_diagram_before_the_gpu():
    from tlc_gnn_amd import topo
    for bad in ("ord0+rel1", "", None, "Ord0"):
        with pytest.raises(ValueError):
            topo.images(None, None, None, None, which=bad)
        with pytest.raises(ValueError):
            topo.wasserstein_to(None, None, None, None, None, None, which=bad)

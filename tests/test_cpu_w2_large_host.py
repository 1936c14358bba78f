"""Host side of tlc_w2_large_matching (no GPU): the exported symbols and their argtypes, the mirrored constants, the workspace arithmetic
against the layout's formula, what the entry refuses before it reads a pointer, and the `large=` / `w2_large=` keyword of its callers."""
import ctypes as C
import inspect
import os
import re

import pytest

from tlc_gnn_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID = 0, 1                                    # TLC_OK, TLC_ERR_INVALID_ARG
NAMES = ("tlc_w2_large_work_bytes", "tlc_w2_large_matching")


def need(max_rows, slots):
    return _lib.lib().tlc_w2_large_work_bytes(C.c_int64(max_rows), C.c_int32(slots))


def up256(v):
    return (v + 255) & ~255


def slot_formula(rows):
    """TlcW2LargeScratch of csrc/scratch_layouts.h restated: 256 control bytes, then u, v, minv f64 | pcol, way int32 | used, rdone u8,
    each on a multiple of 256; rows above the cap need no state."""
    rows = min(rows, _lib.W2_LARGE_NMAX)
    return 256 + 3 * up256(8 * rows) + 2 * up256(4 * rows) + 2 * up256(rows)


def call(n_problems=1, order=2, infer=0, min_rows=0, work=0x1000, work_bytes=1 << 20, null_at=None):
    """tlc_w2_large_matching with made-up device pointers: every case here must be refused (or be done) before one of them is read.
    null_at: which of (xoff, X, yoff, Y, loss, wxy, wxd, wyd, assign_x, assign_y, gradX, status) is NULL."""
    p = [C.c_void_p(0x1000) for _ in range(12)]
    for k in (null_at if isinstance(null_at, tuple) else (null_at,)):
        if k is not None:
            p[k] = None
    return _lib.lib().tlc_w2_large_matching(C.c_int32(n_problems), p[0], p[1], p[2], p[3], C.c_int(order), C.c_int(infer), C.c_int32(min_rows),
                                            p[4], p[5], p[6], p[7], p[8], p[9], p[10], p[11], C.c_void_p(work) if work else None,
                                            C.c_int64(work_bytes), None)


def test_symbols_argtypes_and_constants():
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "tlcgnn.h")).read()
    for name in NAMES:
        assert hasattr(L, name) and name in _lib.SYMBOLS, name
        assert re.search(r"\b%s\s*\(" % name, header), name
    assert L.tlc_w2_large_work_bytes.argtypes == [C.c_int64, C.c_int32] and L.tlc_w2_large_work_bytes.restype is C.c_int64
    a = L.tlc_w2_large_matching.argtypes
    assert len(a) == 19 and a[0] is C.c_int32 and a[5] is C.c_int and a[6] is C.c_int and a[7] is C.c_int32 and a[17] is C.c_int64
    assert all(t is C.c_void_p for t in a[1:5] + a[8:17] + a[18:])
    cut = {k: int(v) for k, v in re.findall(r"#define\s+TLC_W2_(\w+)\s+(\d+)", header)}
    assert cut == {"LDS_NMAX": _lib.W2_LDS_NMAX, "LARGE_NMAX": _lib.W2_LARGE_NMAX, "LARGE_COUNTERS": _lib.W2_LARGE_COUNTERS}
    assert _lib.W2_LDS_NMAX == 4096 and _lib.W2_LARGE_NMAX == 65536
    # the cap covers the reference's 30 000-point limit in both forms
    assert _lib.W2_LARGE_NMAX >= 2 * 30000
    layouts = open(os.path.join(ROOT, "tlc-gnn_amd", "csrc", "scratch_layouts.h")).read()
    m = re.search(r"struct TlcW2LargeScratch \{\s*static constexpr int64_t HEAD = (\d+), COUNTERS = (\d+), NMAX = (\d+),", layouts)
    assert m and (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (256, _lib.W2_LARGE_COUNTERS, _lib.W2_LARGE_NMAX)
    assert 8 * _lib.W2_LARGE_COUNTERS <= 256


def test_work_bytes_equal_the_layouts_formula_and_are_linear_in_slots():
    for rows in (4097, 30000, 65536):
        assert need(rows, 1) == slot_formula(rows), rows
        for slots in (0, 1, 2, 3, 64, 256):
            assert need(rows, slots) == slots * need(rows, 1), (rows, slots)
    # about 34 bytes per row: 2.2 MB at the cap
    assert 34 * 65536 <= need(65536, 1) <= 34 * 65536 + 8 * 256
    assert need(0, 1) == 256 and need(0, 0) == 0


def test_work_bytes_monotone_in_both_arguments():
    pts = (0, 1, 2, 31, 32, 33, 255, 256, 257, 4096, 4097, 8192, 30000, 44000, 65535, 65536, 65537, 1 << 20, 1 << 40)
    for slots in (1, 2, 7, 256):
        seq = [need(r, slots) for r in pts]
        assert seq == sorted(seq) and seq[0] < seq[-1], (slots, seq)
    for rows in pts:
        seq = [need(rows, s) for s in range(0, 40)]
        assert seq == sorted(seq) and len(set(seq)) == len(seq), rows
    # rows above the cap are refused by the kernel and need no state
    assert need(65537, 1) == need(65536, 1) == need(1 << 40, 1)
    assert need(-1, 1) == -1 and need(10, -1) == -1


def test_entry_refusals_before_any_pointer_is_read():
    L = _lib.lib()
    assert call(n_problems=-1) == INVALID
    for order in (0, 3, -1):
        assert call(order=order) == INVALID and call(n_problems=0, order=order) == INVALID
    assert b"order" in L.tlc_last_error()
    for infer in (-1, 2):
        assert call(infer=infer) == INVALID and call(n_problems=0, infer=infer) == INVALID
    assert call(min_rows=-2) == INVALID
    # nothing to do: fine whatever the pointers are
    assert call(n_problems=0) == OK and call(n_problems=0, work=0, work_bytes=0, null_at=tuple(range(12))) == OK
    # null pointers: the offsets, the outputs, the status
    for k in (0, 2, 4, 5, 6, 8, 11):
        assert call(null_at=k) == INVALID, k
        assert b"null" in L.tlc_last_error()
    # wyd and assign_y may be null in the training form only
    for k in (7, 9):
        assert call(infer=1, null_at=k) == INVALID, k
    # the workspace: none, a negative size, a misaligned one
    assert call(work=0) == INVALID
    assert call(work_bytes=-1) == INVALID
    assert call(work=0x1010) == INVALID and b"aligned" in L.tlc_last_error()


def test_the_keyword_defaults_to_refuse_everywhere():
    from tlc_gnn_amd import autograd, topo
    from tlc_gnn_amd.Knowledge_Distillation.Teacher_model import Teacher_Model
    for fn, kw in ((ops.w2_partial_matching, "large"), (ops.w2_inference_matching, "large"), (autograd.diagram_loss, "large"),
                   (topo.wasserstein_to, "w2_large"), (Teacher_Model.forward, "w2_large")):
        assert inspect.signature(fn).parameters[kw].default == "refuse", fn
    sig = inspect.signature(ops.w2_large_matching).parameters
    assert [sig[k].default for k in ("min_rows", "want_grad", "work")] == [0, True, None]
    for bad in ("host", None, True, "Device"):
        with pytest.raises(ValueError, match="refuse"):
            ops.check_w2_large(bad)
        with pytest.raises(ValueError, match="refuse"):
            autograd.diagram_loss(None, None, large=bad)
    ops.check_w2_large("refuse")
    ops.check_w2_large("device")

"""Host side of tlc_dgm_gram / tlc_dgm_gram_vjp (no GPU): the exported symbols and mirrored constants, the workspace arithmetic, what the
entries refuse before they read a pointer, and the restatements of tests/dgm_gram_cases.py -- against brute-force loops, finite
differences, closed forms, the symmetry of the kernel and its positive definiteness."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dgm_gram_cases as cases
from tlc_gnn_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1                                           # TLC_ERR_INVALID_ARG
NAMES = ("tlc_dgm_gram_work_bytes", "tlc_dgm_gram", "tlc_dgm_gram_vjp")
ALL, PAIRED, SYMMETRIC, MIRROR = _lib.DG_ALL, _lib.DG_PAIRED, _lib.DG_SYMMETRIC, _lib.DG_MIRROR


def need(nx, ny, max_nx, max_ny, flags):
    """-> (full, least)"""
    least = C.c_int64(-7)
    full = _lib.lib().tlc_dgm_gram_work_bytes(C.c_int32(nx), C.c_int32(ny), C.c_int64(max_nx), C.c_int64(max_ny), C.c_uint32(flags), C.byref(least))
    return int(full), int(least.value)


def call(nx=2, ny=2, gamma=1.0, scale=1.0, flags=ALL, max_nx=10, max_ny=10, work_bytes=0, work=0, null_at=None, same=False, vjp=False):
    """Either entry with made-up device pointers: every case here must be refused (or be done) before one of them is read.
    null_at: which of (x_offs, x_pts, x_w, y_offs, y_pts, y_w, then out / status_x / status_y, or for the VJP status_x / status_y /
    grad_out / grad_pts / grad_w) is NULL; same: Y's three pointers are X's."""
    p = [C.c_void_p(0x1000 * (k + 1)) for k in range(11)]
    if same:
        p[3:6] = p[0:3]
    if null_at is not None:
        p[null_at] = None
    fn = _lib.lib().tlc_dgm_gram_vjp if vjp else _lib.lib().tlc_dgm_gram
    tail = p[6:11] if vjp else p[6:9]
    return fn(C.c_int32(nx), p[0], p[1], p[2], C.c_int32(ny), p[3], p[4], p[5], C.c_double(gamma), C.c_double(scale), C.c_uint32(flags),
              C.c_int64(max_nx), C.c_int64(max_ny), *tail, C.c_void_p(work) if work else None, C.c_int64(work_bytes), None)


# ---- the library ----------------------------------------------------------------------------------------------------------------------
def test_symbols_and_constants():
    L = _lib.lib()
    for name in NAMES:
        assert hasattr(L, name) and name in _lib.SYMBOLS, name
        assert getattr(L, name).argtypes is not None, name
    assert L.tlc_dgm_gram_work_bytes.restype is C.c_int64
    assert len(L.tlc_dgm_gram_work_bytes.argtypes) == 6 and len(L.tlc_dgm_gram.argtypes) == 19 and len(L.tlc_dgm_gram_vjp.argtypes) == 21
    header = open(os.path.join(ROOT, "include", "tlcgnn.h")).read()
    cut = {k: int(v.rstrip("u"), 0) for k, v in re.findall(r"#define\s+TLC_DG_(\w+)\s+(\w+)", header)}
    assert cut == {"ALL": ALL, "PAIRED": PAIRED, "SYMMETRIC": SYMMETRIC, "MIRROR": MIRROR, "SLICE": _lib.DG_SLICE, "GROUP": _lib.DG_GROUP}
    assert (cases.ALL, cases.PAIRED, cases.SYMMETRIC, cases.MIRROR) == (ALL, PAIRED, SYMMETRIC, MIRROR)
    assert (cases.SLICE, cases.GROUP) == (_lib.DG_SLICE, _lib.DG_GROUP) and cases.GROUP % cases.CHUNK == 0
    # the argument lists of the header, name by name
    for name, count in (("tlc_dgm_gram", 19), ("tlc_dgm_gram_vjp", 21)):
        args = re.search(r"\bint %s\((.*?)\);" % name, header, re.S).group(1)
        assert len(args.split(",")) == count


def test_kernel_params_match_the_wrappers():
    from tlc_gnn_amd import ops
    for kernel in ("pss", "gauss"):
        for sigma in (0.01, 0.5, 1.0, 7.0):
            assert ops.dgm_kernel_params(kernel, sigma) == cases.kernel_params(kernel, sigma)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ops.dgm_kernel_params("pss", bad)
    with pytest.raises(ValueError):
        ops.dgm_kernel_params("sliced", 1.0)


def test_work_bytes_arithmetic():
    S, G = _lib.DG_SLICE, _lib.DG_GROUP
    assert need(100, 100, 64, G, ALL) == (0, 0) and need(100, 100, 0, 0, PAIRED | MIRROR) == (0, 0)
    assert need(0, 5, 5000, 5000, ALL) == (0, 0)
    # prefix arrays alone: a diagram of X above one chunk (the VJP's chunk prefix), nothing above a slice or a group
    full, least = need(10, 10, 65, 10, PAIRED)
    assert full == least and 0 < least <= 2 * 11 * 8 + 4 * 256
    head = least
    # partials: one X diagram's pairs at least, every pair at most
    for nx, ny, mx, my, flags in ((10, 10, S + 1, 10, ALL), (10, 10, 10, G + 1, ALL), (10, 10, 5 * S, 3 * G + 1, ALL),
                                  (10, 10, 5 * S, 3 * G + 1, PAIRED), (1, 1, 70000, 70000, ALL), (1, 1, 70000, 70000, PAIRED | MIRROR),
                                  (7, 7, 2 * S, 2 * S, ALL | SYMMETRIC)):
        full, least = need(nx, ny, mx, my, flags)
        per_pair = cases.slices_of(mx) * cases.groups_of(my)
        row = per_pair * (1 if flags & PAIRED else ny)
        assert 0 < least <= full and least >= 8 * row and least - 8 * row <= head + 8 * (nx + ny)
        assert full - least == 8 * row * (nx - 1)
        assert need(nx, ny, mx, my, flags | MIRROR) == (full, least)
    # the cap of 1 GiB of partials, never below the least size
    full, least = need(4096, 4096, 70000, 70000, ALL)
    assert least <= full <= least + (1 << 30) and full - least < 8 * 69 * 69 * 4096 * 4095
    # -1: negative sizes, unknown or contradictory flags, a size beyond int64
    for args in ((-1, 1, 1, 1, ALL), (1, -1, 1, 1, ALL), (1, 1, -1, 1, ALL), (1, 1, 1, -1, ALL), (1, 1, 1, 1, 0), (1, 1, 1, 1, ALL | PAIRED),
                 (1, 1, 1, 1, ALL | 16), (2, 3, 1, 1, PAIRED), (2, 2, 1, 1, PAIRED | SYMMETRIC), (2, 3, 1, 1, ALL | SYMMETRIC),
                 (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 62, 2 ** 62, ALL)):
        least = C.c_int64(-7)
        assert _lib.lib().tlc_dgm_gram_work_bytes(C.c_int32(args[0]), C.c_int32(args[1]), C.c_int64(args[2]), C.c_int64(args[3]),
                                                  C.c_uint32(args[4]), C.byref(least)) == -1, args
        assert least.value == 0
    assert _lib.lib().tlc_dgm_gram_work_bytes(C.c_int32(1), C.c_int32(1), C.c_int64(5000), C.c_int64(5000), C.c_uint32(ALL), None) > 0


@pytest.mark.parametrize("vjp", [False, True])
def test_refusals_before_any_pointer_is_read(vjp):
    assert call(nx=0, vjp=vjp) == 0 and call(ny=0, nx=0, vjp=vjp) == 0 and call(nx=0, ny=0, flags=PAIRED, vjp=vjp) == 0
    assert call(ny=0, vjp=False) == 0
    for kw in (dict(nx=-1), dict(ny=-1), dict(max_nx=-1), dict(max_ny=-1), dict(work_bytes=-1),
               dict(gamma=0.0), dict(gamma=-1.0), dict(gamma=float("nan")), dict(gamma=float("inf")),
               dict(scale=float("nan")), dict(scale=float("inf")), dict(scale=-float("inf")),
               dict(flags=0), dict(flags=ALL | PAIRED), dict(flags=ALL | 16), dict(flags=ALL | 0x80000000), dict(flags=MIRROR),
               dict(flags=PAIRED, nx=2, ny=3), dict(flags=PAIRED | SYMMETRIC, same=True), dict(flags=ALL | SYMMETRIC),
               dict(flags=ALL | SYMMETRIC, same=True, ny=3), dict(flags=ALL | SYMMETRIC, same=True, max_ny=11),
               dict(null_at=0), dict(null_at=1), dict(null_at=3), dict(null_at=4), dict(null_at=6), dict(null_at=7), dict(null_at=8)):
        assert call(vjp=vjp, **kw) == INVALID, kw
        assert _lib.lib().tlc_last_error()
    # a d_work below the least size, or none at all -- asked of an entry only where it uses one: the forward when a pair can have more
    # than one unit, the VJP for its chunk prefix (PAIRED, a diagram of X above 64 points)
    wide = dict(max_nx=5000, max_ny=5000, flags=PAIRED if vjp else ALL)
    least = need(2, 2, 5000, 5000, wide["flags"])[1]
    assert call(vjp=vjp, work_bytes=least - 1, work=0x1000, **wide) == INVALID and call(vjp=vjp, work_bytes=least, work=0, **wide) == INVALID
    if vjp:
        assert call(vjp=True, max_nx=65, flags=PAIRED, work_bytes=need(2, 2, 65, 10, PAIRED)[1] - 1, work=0x1000) == INVALID
        assert call(vjp=True, null_at=9) == INVALID                  # grad_pts
        assert call(vjp=True, null_at=10) == INVALID                 # x_w without grad_w
        assert call(vjp=True, null_at=2) == INVALID                  # grad_w without x_w
    # the weights are optional, and X's points are when no diagram of X may hold one
    assert call(flags=ALL | SYMMETRIC, same=True, nx=0, ny=0, vjp=vjp) == 0


def test_wrappers_refuse_before_the_library():
    import torch
    from tlc_gnn_amd import autograd, ops, topo
    x = torch.zeros(3, 2, dtype=torch.float64)
    with pytest.raises(ValueError):
        ops.diagram_gram(x, None, kernel="sliced")
    with pytest.raises(ValueError):
        ops.diagram_gram(x, None, sigma=0.0)
    with pytest.raises(ValueError):
        ops.diagram_gram(x, None, yoff=torch.tensor([0, 3]))
    with pytest.raises(ValueError):
        autograd.diagram_gram(x, None, wy=torch.ones(3))
    with pytest.raises(ValueError):
        topo.gram(None, None, None, None, which="ord0+rel1")
    with pytest.raises(ValueError):
        topo.kernel_distance_to(None, None, None, None, None, None, which="ord0+rel1")
    w = ops.pwg_weights(torch.tensor([[0.0, 1.0], [0.5, 0.5], [1.0, 3.0]], dtype=torch.float64), C=2.0, p=2.0)
    assert torch.equal(w, torch.atan(torch.tensor([2.0, 0.0, 8.0], dtype=torch.float64)))


# ---- the restatements -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mirror", [False, True])
@pytest.mark.parametrize("weights", [False, True])
def test_restatement_equals_the_brute_force(mirror, weights):
    rs = np.random.RandomState(11 + 2 * mirror + weights)
    for n in range(6):
        for m in range(6):
            X, Y = cases.random_diagram(rs, n), cases.random_diagram(rs, m)
            wx, wy = (cases.random_weights(rs, n), cases.random_weights(rs, m)) if weights else (None, None)
            for gamma, scale in ((0.125, 0.04), (3.0, -2.0)):
                got = cases.restate_pair(X, wx, Y, wy, gamma, scale, mirror)
                want = cases.brute_pair(X.tolist(), None if wx is None else wx.tolist(), Y.tolist(), None if wy is None else wy.tolist(),
                                        gamma, scale, mirror)
                assert np.float64(got).view(np.uint64) == np.float64(want).view(np.uint64), (n, m, got, want)
                ref = cases.ref_pair(X, wx, Y, wy, gamma, scale, mirror)
                assert abs(got - float(ref["k"])) <= cases.value_bound(ref, scale)
                if n == 0 or m == 0:
                    assert got == 0.0 and not np.signbit(got)


def test_restatement_across_the_cuts_against_longdouble():
    rs = np.random.RandomState(5)
    for n, m in ((65, 130), (cases.SLICE + 1, 3), (3, cases.GROUP + 1), (cases.SLICE + 70, cases.GROUP + 70)):
        X, Y = cases.random_diagram(rs, n), cases.random_diagram(rs, m)
        wx, wy = cases.random_weights(rs, n), cases.random_weights(rs, m)
        got = cases.restate_pair(X, wx, Y, wy, 2.0, 0.5, True)
        ref = cases.ref_pair(X, wx, Y, wy, 2.0, 0.5, True)
        assert abs(got - float(ref["k"])) <= cases.value_bound(ref, 0.5)
        assert cases.chain(n, m) == min(n, 1024) + 6 + min(-(-m // 64), 16) + cases.slices_of(n) * cases.groups_of(m)


@pytest.mark.parametrize("mirror", [False, True])
def test_gradient_against_finite_differences(mirror):
    rs = np.random.RandomState(3 + mirror)
    LD = cases.LD
    X, dY = cases.random_diagram(rs, 5), [cases.random_diagram(rs, k) for k in (4, 0, 7)]
    wx, wY = cases.random_weights(rs, 5), [cases.random_weights(rs, len(Y)) for Y in dY]
    G = rs.uniform(-1.0, 1.0, 3)
    gamma, scale = 1.7, 0.3

    def total(Xv, wv):
        return sum(LD(G[j]) * cases.ref_pair(Xv, wv, dY[j], wY[j], gamma, scale, mirror)["k"] for j in range(3))

    pairs = [cases.ref_pair(X, wx, dY[j], wY[j], gamma, scale, mirror) for j in range(3)]
    gp, gw, bp, bw = cases.ref_grad(pairs, G, wx, gamma, scale, 3)
    h = LD(1e-7)
    for p in range(5):
        for c in range(2):
            Xp, Xm = X.astype(LD), X.astype(LD)
            Xp[p, c] += h
            Xm[p, c] -= h
            fd = (total(Xp, wx) - total(Xm, wx)) / (2 * h)
            assert abs(float(fd - gp[p, c])) <= 1e-9 * (1 + abs(float(fd)))
        wp, wm = wx.astype(LD), wx.astype(LD)
        wp[p] += h
        wm[p] -= h
        fd = (total(X, wp) - total(X, wm)) / (2 * h)
        assert abs(float(fd - gw[p])) <= 1e-9 * (1 + abs(float(fd)))
    # and the fp64 restatement of the documented order lies within the bound of the longdouble one
    rp, rw = cases.restate_grad_rows(X, wx, dY, wY, G, gamma, scale, mirror)
    assert (np.abs(rp - gp.astype(np.float64)) <= bp).all() and (np.abs(rw - gw.astype(np.float64)) <= bw).all()
    assert (bp <= 1e-12).all() and (bw <= 1e-12).all()


def test_the_kernel_is_symmetric_in_its_arguments():
    rs = np.random.RandomState(17)
    dX, dY = cases.pd_batch(rs, 6, 40), cases.pd_batch(rs, 5, 40)
    for mirror in (False, True):
        a = cases.restate_gram(dX, None, dY, None, 0.7, 1.3, mirror)
        b = cases.restate_gram(dY, None, dX, None, 0.7, 1.3, mirror)
        for i in range(6):
            for j in range(5):
                ref = cases.ref_pair(dX[i], None, dY[j], None, 0.7, 1.3, mirror)
                assert abs(a[i, j] - b[j, i]) <= 2 * cases.value_bound(ref, 1.3)


def test_exact_closed_forms():
    one = np.tile([[0.25, 0.75]], (65, 1))
    assert cases.restate_pair(one, None, one, None, 3.0, 1.0, False) == 65.0 * 65.0
    far = one + 40.0
    assert cases.restate_pair(one, None, far, None, 1.0, 1.0, False) == 0.0
    assert cases.restate_pair(one, None, far, None, 1.0, 1.0, True) == 0.0
    assert float(cases.ref_pair(one, None, one, None, 3.0, 1.0, False)["k"]) == 65.0 * 65.0
    # a point and its mirror image cancel exactly: a diagram on the diagonal has a zero PSS kernel against everything
    diag = np.stack([np.arange(5.0), np.arange(5.0)], 1)
    assert cases.restate_pair(diag, None, one, None, 0.5, 1.0, True) == 0.0


@pytest.mark.parametrize("sigma", [0.01, 0.1, 1.0])
def test_the_pss_gram_is_positive_semidefinite(sigma):
    rs = np.random.RandomState(23)
    dgms = cases.pd_batch(rs, 48, 69)
    assert min(len(d) for d in dgms) <= 2 and max(len(d) for d in dgms) >= 65            # (both sides of the 64-point chunk)
    gamma, scale, mirror = cases.kernel_params("pss", sigma)
    K = cases.restate_gram(dgms, None, dgms, None, gamma, scale, mirror)
    K = 0.5 * (K + K.T)
    lam = np.linalg.eigvalsh(K)
    print("sigma %g: least eigenvalue / trace = %.3g" % (sigma, lam[0] / np.trace(K)))
    assert lam[0] >= -1e-12 * np.trace(K)
    # without the mirror's sign (e1 + e2 instead of e1 - e2) the same matrix is still a Gram matrix, but of another kernel; with the
    # mirror term on the wrong point it is not one
    bad = np.array([[cases.restate_pair(a, None, b[:, ::-1] * [1.0, -1.0], None, gamma, scale, True) for b in dgms] for a in dgms])
    assert np.linalg.eigvalsh(0.5 * (bad + bad.T))[0] < -1e-12 * np.trace(K)

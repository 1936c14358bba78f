"""CPU: the yardstick of the exact Ollivier-Ricci curvature (method "OTD") against itself -- the closed forms of
tests/ricci_otd_cases.py against its LP reference -- and the host-side surface of the feature: the two symbols and the TLC_OTD_*
constants of include/tlcgnn.h with their mirrors in _lib, the wrapper's fraction check, and the method argument of the drop-ins.
The kernels themselves: tests/test_gpu_ricci_otd.py."""
import ctypes as C
import inspect
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import ricci_otd_cases as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _kappa(g, s, t, num=1, den=2):
    w, d = oc.exact_wd(g[0], g[1], s, t, num, den)
    return 1 - Fraction(w, d)


def test_closed_forms_agree_with_the_lp_reference():
    for n in (2, 3, 4, 5, 8):
        assert _kappa(oc.complete(n), 0, n - 1) == oc.kappa_complete(n), n
    for n in (3, 4, 5, 6, 7, 9):
        assert _kappa(oc.cycle(n), 0, 1) == oc.kappa_cycle(n), n
    for d in (1, 2, 5, 9):
        assert _kappa(oc.star(d), 0, d) == oc.kappa_star(d) == _kappa(oc.star(d), d, 0), d
    for p, q in ((2, 3), (4, 4), (3, 7), (1, 6)):
        assert _kappa(oc.bipartite(p, q), 0, p) == oc.kappa_bipartite(p, q), (p, q)
    for k in range(5):
        assert _kappa(oc.path(6), k, k + 1) == oc.kappa_path(6, k), k
    for d, c, m, want in ((6, 2, 1, Fraction(0)), (12, 0, 5, Fraction(-5, 12)), (10, 4, 0, Fraction(-1, 5)), (3, 0, 0, Fraction(-1, 3)),
                          (10, 0, 0, Fraction(-4, 5))):            # c = m = 0: 1 - 2 (d - 1) / d
        got = _kappa(oc.two_hubs(d, d, c, m), 0, 1)
        assert got == oc.kappa_two_hubs(d, c, m), (d, c, m)
        assert got == want, (d, c, m)


def test_reference_is_symmetric_and_follows_alpha():
    g = oc.gnp(24, 0.4, 5)
    for s, t in g[1][:12].tolist():
        assert oc.exact_wd(g[0], g[1], s, t, 1, 2) == oc.exact_wd(g[0], g[1], t, s, 1, 2)
        w, d = oc.exact_wd(g[0], g[1], s, t, 1, 1)                  # alpha = 1: all mass on the endpoints, one hop apart
        assert w == d
        w4, d4 = oc.exact_wd(g[0], g[1], s, t, 1, 4)
        w8, d8 = oc.exact_wd(g[0], g[1], s, t, 2, 8)                 # the same alpha on another scale
        assert Fraction(w4, d4) == Fraction(w8, d8)
    # all four hop distances occur between the supports of the tier family's hub edge
    n, e = oc.two_hubs(12, 9, 2, cross=6, outside=3, seed=1)
    import scipy.sparse as sp
    from scipy.sparse.csgraph import shortest_path
    a = sp.coo_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(n, n))
    d = shortest_path(((a + a.T) > 0).astype(float).tocsr(), unweighted=True)
    xs, ys = np.flatnonzero(d[0] <= 1), np.flatnonzero(d[1] <= 1)
    assert len(xs) == 13 and len(ys) == 10 and set(np.unique(d[np.ix_(xs, ys)]).tolist()) == {0.0, 1.0, 2.0, 3.0}


def test_otd_constants_mirror_the_header_and_the_symbols_are_bound():
    from tlc_gnn_amd import _lib
    _lib.build()                                                  # make: nothing to do when the library is up to date
    header = open(os.path.join(ROOT, "include", "tlcgnn.h")).read()
    val = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, header).group(1))
    assert val("TLC_OTD_WAVE_PRODUCT") == _lib.OTD_WAVE_PRODUCT
    assert val("TLC_OTD_WAVE_SUPPORT") == _lib.OTD_WAVE_SUPPORT
    assert val("TLC_OTD_WAVE_DENOM") == _lib.OTD_WAVE_DENOM == 2 ** 16 - 1          # u16 flow cells
    assert 2 * (_lib.OTD_WAVE_PRODUCT - 1) <= _lib.OTD_WAVE_DENOM                   # alpha = 1/2: the product limit implies the other
    assert val("TLC_OTD_MAX_SUPPORT") == _lib.OTD_MAX_SUPPORT
    assert val("TLC_OTD_LDS_BYTES") == _lib.OTD_LDS_BYTES <= 160 * 1024
    assert 12 * _lib.OTD_MAX_SUPPORT + 64 <= _lib.OTD_LDS_BYTES < 12 * (_lib.OTD_MAX_SUPPORT + 1) + 64
    L = _lib.lib()
    for sym in ("tlc_ollivier_ricci_otd", "tlc_ollivier_ricci_otd_work_bytes"):
        assert sym in _lib.SYMBOLS and getattr(L, sym).argtypes, sym
        assert re.search(r"\bint\s+%s\s*\(" % sym, header), sym
    assert len(L.tlc_ollivier_ricci_otd.argtypes) == 15 and len(L.tlc_ollivier_ricci_otd_work_bytes.argtypes) == 4


def test_work_bytes_sizes_and_refusals():
    from tlc_gnn_amd import _lib, engine
    _lib.build()
    L = _lib.lib()
    need = C.c_int64(-1)
    assert L.tlc_ollivier_ricci_otd_work_bytes(10, 400, 40000, None) == 1
    assert L.tlc_ollivier_ricci_otd_work_bytes(-1, 400, 40000, C.byref(need)) == 1
    assert L.tlc_ollivier_ricci_otd_work_bytes(10, 1, 40000, C.byref(need)) == 1
    assert L.tlc_ollivier_ricci_otd_work_bytes(10, _lib.OTD_MAX_SUPPORT + 1, 40000, C.byref(need)) == 1
    assert b"max_support" in L.tlc_last_error()
    assert L.tlc_ollivier_ricci_otd_work_bytes(10, 400, 0, C.byref(need)) == 1
    assert L.tlc_ollivier_ricci_otd_work_bytes(10, 400, 40000, C.byref(need)) == 0
    assert need.value == 16 + 48 + 10 * (10000 + 160000)             # counter, list, ten slots of 2-bit codes + u32 cells
    assert L.tlc_ollivier_ricci_otd_work_bytes(1000, 400, 40000, C.byref(need)) == 0
    assert need.value == 16 + 4000 + 32 * (10000 + 160000)
    assert L.tlc_ollivier_ricci_otd_work_bytes(1, _lib.OTD_MAX_SUPPORT, 40000, C.byref(need)) == 0
    assert need.value == 16 + 16 + (10000 + 320000)                  # supports that could carry 2^32: u64 cells
    assert L.tlc_ollivier_ricci_otd_work_bytes(0, 400, 40000, C.byref(need)) == 0 and need.value > 16
    # the LDS <-> slot boundary of the hub kernel's codes, as the wrapper exports it
    assert engine.otd_lds_codes(2) == 4 * (_lib.OTD_LDS_BYTES - 32 - 32)
    assert engine.otd_lds_codes(1600) == 4 * (_lib.OTD_LDS_BYTES - 19200 - 32) < 800 * 800
    assert engine.otd_lds_codes(_lib.OTD_MAX_SUPPORT) >= 0


def test_alpha_must_be_an_exact_fraction():
    """validated before the GPU is asked for: 0.3 is not p/q with q <= 1024, 0.5 and 0.25 are"""
    from tlc_gnn_amd import engine
    rowptr, col, edges = np.array([0, 1, 2]), np.array([1, 0]), np.array([[0, 1]])
    for bad in (0.3, 1.0 / 3.0, 1.5, -0.25, Fraction(1, 1025), float("nan"), "half"):
        with pytest.raises(ValueError):
            engine.ollivier_ricci_otd(rowptr, col, edges, alpha=bad)
    assert engine._otd_fraction(0.5) == (1, 2) and engine._otd_fraction(0.25) == (1, 4)
    assert engine._otd_fraction(Fraction(1, 3)) == (1, 3) and engine._otd_fraction(1) == (1, 1) and engine._otd_fraction(0) == (0, 1)
    assert engine._otd_fraction(Fraction(3, 1024)) == (3, 1024)


def test_unknown_method_is_a_value_error_before_any_work():
    from tlc_gnn_amd import loaddatas
    from tlc_gnn_amd.data import Data
    from tlc_gnn_amd.Knowledge_Distillation import data_utils_LP, ConvCurv_GIN
    data = Data(x=None, edge_index=np.array([[0, 1], [1, 0]]), y=np.zeros(2))
    for bad in ("nonsense", "otd", "sinkhorn", None):
        with pytest.raises(ValueError):
            loaddatas.compute_ricci_curvature(data, method=bad)
        with pytest.raises(ValueError):
            data_utils_LP.compute_ricci_curvature(data, "toy", cache_dir=None, method=bad)
    assert loaddatas.RICCI_METHODS == ("Sinkhorn", "OTD")
    assert inspect.signature(loaddatas.compute_ricci_curvature).parameters["method"].default == "Sinkhorn"
    assert inspect.signature(data_utils_LP.compute_ricci_curvature).parameters["method"].default == "Sinkhorn"
    assert inspect.signature(ConvCurv_GIN.Net.__init__).parameters["ricci_method"].default == "Sinkhorn"
    assert inspect.signature(ConvCurv_GIN.call).parameters["ricci_method"].default == "Sinkhorn"
    assert "pipelines_GIN.py:79" in ConvCurv_GIN.Net.__init__.__doc__

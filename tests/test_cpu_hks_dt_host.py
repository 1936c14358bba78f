"""CPU: the derivative of the heat-kernel signature in its diffusion time (tlc_hks_batch_dt, tlc_hks_large_batch_dt) as far as it
needs no device: the numpy restatement of tests/hks_dt_cases.py (the oracle of tests/test_gpu_hks_dt.py) against closed forms and
against central differences of its own values, the two symbols, and the refusals both entries decide on the host before anything is
launched."""
import ctypes as C

import numpy as np
import pytest

import hks_dt_cases as hc

TIMES = (0.0, 0.1, 0.5, 1.0, 10.0, 64.0)


def _lib_built():
    import __graft_entry__ as ge
    ge.build()
    from tlc_gnn_amd import _lib
    return _lib


def test_eigen_form_against_closed_forms():
    """K_33, K_257, the stars K(1,600) and K(1,2000), C_400, K(150,170) at t = 0 .. 64: the eigen form of the derivative within 1e-12 of
    the closed forms (2.7e-14 measured: LAPACK's own error on these degenerate spectra); at t = 0 it is -1 for every node."""
    cases = [(hc.complete(33), lambda t: hc.d_complete(33, t)), (hc.complete(257), lambda t: hc.d_complete(257, t)),
             (hc.star(601), lambda t: hc.d_star(601, t)), (hc.star(2001), lambda t: hc.d_star(2001, t)),
             (hc.cycle(400), lambda t: hc.d_cycle(400, t)), (hc.bipartite(150, 170), lambda t: hc.d_bipartite(150, 170, t))]
    worst = 0.0
    for (n, e), closed in cases:
        pairs = hc.eigenpairs(n, e)
        for t in TIMES:
            val, dval = hc.eigen_form(n, e, t, pairs)
            worst = max(worst, np.abs(dval - closed(t)).max())
            assert np.all(np.abs(dval) <= 2.0 * val + 1e-13)            # every eigenvalue lies in [0, 2]
        assert np.abs(hc.eigen_form(n, e, 0.0, pairs)[1] + 1.0).max() <= 1e-12
    print("worst |eigen form - closed form| %.2e" % worst)
    assert worst <= 1e-12


def test_small_and_isolated():
    for n in (1, 2, 3):
        assert np.array_equal(hc.eigen_form(*hc.path_plus_isolated(n), 0.7)[1], np.zeros(n))      # no edges: derivative exactly 0
        assert np.array_equal(hc.eigen_form(*hc.path_plus_isolated(n), 0.7)[0], np.ones(n))
    assert np.abs(hc.eigen_form(*hc.complete(2), 0.3)[1] - hc.d_complete(2, 0.3)).max() <= 1e-15
    assert np.abs(hc.eigen_form(*hc.star(2), 0.3)[1] - hc.d_star(2, 0.3)).max() <= 1e-15
    n, e = hc.path_plus_isolated(9)
    d = hc.eigen_form(n, e, 1.0)[1]
    assert np.array_equal(d[-2:], np.zeros(2)) and np.all(d[:-2] < 0)
    assert hc.eigen_form(0, np.zeros((0, 2)), 1.0)[1].shape == (0,)


def test_neighbour_form_is_the_eigen_form():
    """-[K]_vv + sum_u [K]_uv / sqrt(d_u d_v) on a random 300-node graph with isolated nodes (1.6e-15 measured)"""
    n, e = hc.gnp(300, 0.01, 5)
    assert (np.bincount(e.reshape(-1), minlength=n) == 0).any()
    for t in (0.3, 10.0, 64.0):
        assert np.abs(hc.neighbour_form(n, e, t) - hc.eigen_form(n, e, t)[1]).max() <= 1e-13


def test_derivative_against_central_differences():
    """raw and normalised: (v(t + h) - v(t - h)) / 2h with h = 1e-5 differs from the derivative by h^2 / 6 |v'''| <= 1.4e-10 (|v'''|
    <= 8) plus the rounding of the values over 2h (1e-15 / 1e-5)"""
    h = 1e-5
    for n, e in (hc.gnp(40, 0.1, 1), hc.gnp(97, 0.1, 2), hc.cycle(12), hc.complete(7), hc.path_plus_isolated(11)):
        pairs = hc.eigenpairs(n, e)
        for t in (0.1, 1.0, 10.0):
            val, dval = hc.eigen_form(n, e, t, pairs)
            lo, hi = hc.eigen_form(n, e, t - h, pairs)[0], hc.eigen_form(n, e, t + h, pairs)[0]
            assert np.abs((hi - lo) / (2 * h) - dval).max() <= 1e-9
            f, df = hc.quotient(val, dval)
            flo, fhi = hc.quotient(lo, dval)[0], hc.quotient(hi, dval)[0]
            assert np.abs((fhi - flo) / (2 * h) - df).max() <= 4e-9 / val.max()


def test_quotient_rule_takes_the_first_index_of_the_maximum():
    val, dval = np.array([0.5, 1.0, 1.0, 0.25]), np.array([-0.5, -0.25, -0.75, -0.125])
    f, df = hc.quotient(val, dval)
    den = 1.0 + 1e-10
    assert np.array_equal(f, val / den)
    assert np.array_equal(df, (dval - f * (-0.25)) / den)               # hks'(a) of a = 1, not of a = 2


def test_symbols_and_argtypes():
    _lib = _lib_built()
    L = _lib.lib()
    assert "tlc_hks_batch_dt" in _lib.SYMBOLS and len(L.tlc_hks_batch_dt.argtypes) == len(L.tlc_hks_batch.argtypes) + 1 == 15
    assert "tlc_hks_large_batch_dt" in _lib.SYMBOLS and len(L.tlc_hks_large_batch_dt.argtypes) == len(L.tlc_hks_large_batch.argtypes) + 1 == 18


FAKE = C.c_void_p(0x1000)           # a non-null, 16-byte aligned address that a refused call never reads


def _jacobi(L, n_times=1, flags=0, dout=FAKE, times=(0.1,) * 9):
    h = (C.c_double * 9)(*times)
    return L.tlc_hks_batch_dt(FAKE, FAKE, FAKE, 1, 3, 2, h, n_times, flags, FAKE, dout, FAKE, FAKE, 1 << 30, None)


def test_jacobi_entry_refusals_on_the_host():
    """decided before the device is asked for anything: they return TLC_ERR_INVALID_ARG on a machine without a GPU too"""
    _lib = _lib_built()
    L = _lib.lib()
    assert _jacobi(L, dout=None) == 1 and "d_dout" in L.tlc_last_error().decode()
    assert _jacobi(L, n_times=0) == 1 and _jacobi(L, n_times=_lib.HKS_TMAX + 1) == 1
    assert _jacobi(L, flags=2) == 1 and _jacobi(L, flags=_lib.HKS_NORMALISE | 0x100) == 1
    assert L.tlc_hks_batch_dt(FAKE, FAKE, FAKE, 1, 3, 2, None, 1, 0, FAKE, FAKE, FAKE, FAKE, 1 << 30, None) == 1
    assert L.tlc_hks_batch_dt(FAKE, FAKE, FAKE, -1, 3, 2, (C.c_double * 1)(0.1), 1, 0, FAKE, FAKE, FAKE, FAKE, 1 << 30, None) == 1
    # an empty batch is no work and no refusal -- but a null d_dout is refused even then
    assert L.tlc_hks_batch_dt(None, None, None, 0, 0, 0, (C.c_double * 1)(0.1), 1, 0, None, FAKE, None, None, 0, None) == 0
    assert L.tlc_hks_batch_dt(None, None, None, 0, 0, 0, (C.c_double * 1)(0.1), 1, 0, None, None, None, None, 0, None) == 1


def _large(L, times=(0.1,), n_times=None, flags=0, dout=FAKE, sel=(0,), nodes=(300,), work_bytes=1 << 40, n_graphs=2):
    h = (C.c_double * max(len(times), 1))(*times)
    s, c = (C.c_int64 * max(len(sel), 1))(*sel), (C.c_int64 * max(len(nodes), 1))(*nodes)
    return L.tlc_hks_large_batch_dt(FAKE, FAKE, FAKE, n_graphs, 600, 10, s, c, len(sel), h, len(times) if n_times is None else n_times, flags,
                                    FAKE, dout, FAKE, FAKE, work_bytes, None)


def test_large_entry_refusals_on_the_host():
    _lib = _lib_built()
    L = _lib.lib()
    assert _large(L, dout=None) == 1 and "d_dout" in L.tlc_last_error().decode()
    assert _large(L, n_times=0) == 1 and _large(L, times=(0.1,) * 9) == 1
    assert _large(L, flags=2) == 1
    for t in (-1.0, 65.0, float("nan"), float("inf")):
        assert _large(L, times=(0.1, t)) == 1, t
    assert _large(L, sel=(1, 0), nodes=(300, 300)) == 1 and _large(L, sel=(0, 0), nodes=(300, 300)) == 1
    assert _large(L, sel=(2,), nodes=(300,)) == 1 and _large(L, nodes=(-1,)) == 1
    lo, hi = C.c_int64(0), C.c_int64(0)
    assert L.tlc_hks_large_work_bytes((C.c_int64 * 1)(300), 1, 1, C.byref(lo), C.byref(hi)) == 0
    assert _large(L, work_bytes=lo.value - 1) == 1 and "min_bytes" in L.tlc_last_error().decode()
    # an empty selection is no work and no refusal -- but a null d_dout is refused even then
    assert _large(L, sel=(), nodes=()) == 0
    assert _large(L, sel=(), nodes=(), dout=None) == 1


def test_python_layers_check_their_arguments_without_a_device():
    import torch
    from tlc_gnn_amd import autograd, topo
    no = torch.tensor([0, 3])
    eo = torch.tensor([0, 2])
    E = torch.tensor([[0, 1], [1, 2]], dtype=torch.int32)
    for bad in (torch.zeros(0), torch.zeros(9), torch.zeros(2, 2), torch.tensor([1, 2]), 0.5):
        with pytest.raises(ValueError):
            autograd.hks_signature(bad, no, eo, E)
    for bad in (torch.zeros(2), 0.5):
        with pytest.raises(ValueError):
            topo.hks_filtration(bad, no, eo, E)
    assert "HKS time" in topo.__doc__ and "hks_filtration" in topo.__doc__

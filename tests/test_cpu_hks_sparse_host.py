"""Host side of tlc_hks_sparse_batch (no GPU): the exported symbols and mirrored constants, the new keyword of the wrappers, the number
of Taylor terms against exact Poisson tails, the workspace arithmetic, what the entry refuses before it reads a pointer, and the numpy
restatement of the kernel (tests/hks_sparse_cases.py) against a dense eigendecomposition and closed forms.

Bounds: 1e-11 (value) and 2e-11 (derivative) absolute, the bounds of the other HKS tiers' tests (tests/test_gpu_hks_large.py,
tests/test_gpu_hks_dt.py).  The method sums non-negative terms only; the restatement stays below 2e-14 on these cases."""
import ctypes as C
import inspect
import os
import re
from decimal import Decimal, getcontext

import numpy as np
import pytest

import hks_sparse_cases as cases
from tlc_gnn_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1                                           # TLC_ERR_INVALID_ARG
TIMES = (0.0, 1e-9, 0.1, 10.0, 64.0)


def work_bytes(nodes, edges, n_times=1):
    lo, hi = C.c_int64(-1), C.c_int64(-1)
    S = len(nodes)
    rc = _lib.lib().tlc_hks_sparse_work_bytes((C.c_int64 * max(S, 1))(*nodes), (C.c_int64 * max(S, 1))(*edges), C.c_int64(S), C.c_int32(n_times),
                                              C.byref(lo), C.byref(hi))
    return rc, lo.value, hi.value


def test_symbols_and_constants():
    L = _lib.lib()
    for name in ("tlc_hks_sparse_terms", "tlc_hks_sparse_work_bytes", "tlc_hks_sparse_batch", "tlc_hks_sparse_batch_dt"):
        assert hasattr(L, name) and name in _lib.SYMBOLS, name
    header = open(os.path.join(ROOT, "include", "tlcgnn.h")).read()
    cut = dict(re.findall(r"#define\s+TLC_HKS_SPARSE_(\w+)\s+([\d.]+)", header))
    assert {k: float(v) for k, v in cut.items()} == {"TIME_MAX": _lib.HKS_SPARSE_TIME_MAX, "PANEL": _lib.HKS_SPARSE_PANEL,
                                                     "LONG_ROW": _lib.HKS_SPARSE_LONG_ROW}
    assert _lib.HKS_SPARSE_PANEL == 64 == cases.PANEL and _lib.HKS_SPARSE_TIME_MAX == cases.TIME_MAX
    assert _lib.HKS_SPARSE_LONG_ROW % _lib.HKS_SPARSE_PANEL == 0
    # the arity of the bindings is the arity of the declarations
    for name in ("tlc_hks_sparse_terms", "tlc_hks_sparse_work_bytes", "tlc_hks_sparse_batch", "tlc_hks_sparse_batch_dt"):
        decl = re.search(r"\b%s\(([^;]*?)\);" % name, header, re.S).group(1)
        assert len(getattr(L, name).argtypes) == len(decl.split(",")), name
    assert len(L.tlc_hks_sparse_batch.argtypes) == len(L.tlc_hks_large_batch.argtypes) + 1
    assert len(L.tlc_hks_sparse_batch_dt.argtypes) == len(L.tlc_hks_large_batch_dt.argtypes) + 1


def test_keyword_defaults_to_host_and_refuses_unknown_values():
    import torch
    from tlc_gnn_amd import autograd, topo
    from tlc_gnn_amd.Knowledge_Distillation import data_utils_GC as gc, data_utils_LP as lp, data_utils_NC as nc
    fns = [lp.hks_filtration_device, lp.Vicinities.batch, nc.NodeVicinities.batch, lp.compute_persistence_image, nc.compute_persistence_image,
           gc.compute_persistence_image_batch, gc.compute_persistence_image, gc.call, gc.ground_truth_packed, gc.call_packed,
           autograd.hks_signature, topo.hks_filtration]
    for fn in fns:
        assert inspect.signature(fn).parameters["hks_sparse"].default == 'host', fn
    assert lp.HKS_SPARSE == ("host", "device") and lp.hks_sparse_device == 0
    z = torch.zeros(1, dtype=torch.int64)
    e = torch.zeros((0, 2), dtype=torch.int32)
    calls = [lambda: lp.hks_filtration_device(z, z, e, 0.1, 0, hks_sparse='gpu'),
             lambda: lp.compute_persistence_image(None, 0, 1, hks_sparse='gpu'),
             lambda: nc.compute_persistence_image(None, 0, hks_sparse='gpu'),
             lambda: gc.compute_persistence_image_batch([], hks_sparse='gpu'),
             lambda: gc.compute_persistence_image(None, hks_sparse='gpu'),
             lambda: gc.ground_truth_packed(z, z, e, hks_sparse='gpu'),
             lambda: gc.call_packed(None, "x", hks_sparse='gpu'),
             lambda: gc.call([], "x", hks_sparse='gpu'),
             lambda: gc.call([(3, np.array([[0, 1], [1, 2]]))], "x", gn=1, hks_sparse='gpu'),
             lambda: lp.Vicinities.batch(None, [], 1, hks_sparse='gpu'),
             lambda: nc.NodeVicinities.batch(None, [], 1, hks_sparse='gpu'),
             lambda: autograd.hks_signature(torch.ones(1), z, z, e, hks_sparse='gpu'),
             lambda: topo.hks_filtration(torch.ones(1), z, z, e, hks_sparse='gpu')]
    for f in calls:
        with pytest.raises(ValueError, match="hks_sparse"):
            f()


def _tail(tau, k):
    """P(Poisson(tau) > k) to 60 digits"""
    tau = Decimal(tau)
    term, s = Decimal(1), Decimal(0)
    for j in range(1, k + 1):
        term = term * tau / j
    for j in range(k + 1, k + 500):
        term = term * tau / j
        s += term
    return s * (-tau).exp()


def test_terms_mirror_and_tail_bound():
    getcontext().prec = 60
    L = _lib.lib()
    rs = np.random.RandomState(7)
    grid = list(TIMES) + [1.0, 2.0, 5e-324, 1e-300, 63.999, 37.1] + list(rs.uniform(0, 64, 60)) + list(10.0 ** rs.uniform(-12, 1.8, 60))
    limit = Decimal(2) ** -64
    for t in grid:
        K = L.tlc_hks_sparse_terms(C.c_double(t))
        assert K == _lib.hks_sparse_terms(t) == cases.terms(t) and K >= 0, t
        tau = float(t) * 0.5
        assert _tail(tau, K) <= limit, t
        assert K <= 2 or _tail(tau, K - 3) > limit, t          # at most 2 above the least such k
    assert [_lib.hks_sparse_terms(t) for t in (0.0, 0.1, 1.0, 10.0, 64.0)] == [0, 9, 16, 36, 96]
    for t in (-1e-300, 64.0000001, float("inf"), float("nan")):
        assert L.tlc_hks_sparse_terms(C.c_double(t)) == -1 == _lib.hks_sparse_terms(t)


def test_work_bytes():
    assert work_bytes([], []) == (0, 0, 0)
    P = _lib.HKS_SPARSE_PANEL
    prev = None
    for n, m in ((1, 0), (2, 1), (64, 100), (65, 100), (65, 2000), (5000, 4999), (5000, 20000), (19717, 44324), (200000, 300000)):
        rc, lo, hi = work_bytes([n], [m])
        assert rc == 0 and 0 < lo <= hi, (n, m)
        # the arrays the header names: keys twice, columns, row starts, r_u; a panel's three vectors; every panel
        fixed = 2 * 8 * 2 * m + 4 * 2 * m + 4 * (n + 1) + 8 * n
        assert lo >= fixed + 3 * 8 * P * n and hi >= fixed + 3 * 8 * P * n * ((n + P - 1) // P), (n, m)
        if prev is not None:
            assert lo >= prev[0] and hi >= prev[1], (n, m)     # monotone in n and in m
        prev = (lo, hi)
    # a selection: min grows with the largest graph only, all with every graph
    _, lo1, hi1 = work_bytes([5000], [4999])
    _, lo2, hi2 = work_bytes([5000, 300], [4999, 600])
    assert lo2 >= lo1 and hi2 > hi1 and hi2 - hi1 > lo2 - lo1
    assert work_bytes([10], [5], n_times=0)[0] == INVALID and work_bytes([10], [5], n_times=_lib.HKS_TMAX + 1)[0] == INVALID
    assert work_bytes([-1], [0])[0] == INVALID and work_bytes([1], [-1])[0] == INVALID
    assert work_bytes([1 << 31], [0])[0] == INVALID and work_bytes([10], [1 << 30])[0] == INVALID
    assert work_bytes([1 << 30, 1 << 30], [0, 0])[0] == INVALID


def _call(dt=False, n_graphs=2, sel=(0, 1), nodes=(5, 6), edges=(4, 5), times=(0.1,), flags=0, work_bytes=1 << 30, work=0x1000, null_at=None):
    """the entry with made-up device pointers: every case here must be refused before one of them is read"""
    p = [C.c_void_p(0x1000) for _ in range(6)]                  # node_ptr, edge_ptr, edges, out, dout, status
    if null_at is not None:
        p[null_at] = None
    S, T = len(sel), len(times)
    head = (p[0], p[1], p[2], C.c_int64(n_graphs), C.c_int64(100), C.c_int64(100), (C.c_int64 * max(S, 1))(*sel), (C.c_int64 * max(S, 1))(*nodes),
            (C.c_int64 * max(S, 1))(*edges), C.c_int64(S), (C.c_double * max(T, 1))(*times), C.c_int32(T), C.c_uint32(flags), p[3])
    tail = (p[5], C.c_void_p(work), C.c_int64(work_bytes), None)
    if dt:
        return _lib.lib().tlc_hks_sparse_batch_dt(*head, p[4], *tail)
    return _lib.lib().tlc_hks_sparse_batch(*head, *tail)


def test_entry_refusals():
    for dt in (False, True):
        assert _call(dt, times=()) == INVALID and _call(dt, times=(0.1,) * (_lib.HKS_TMAX + 1)) == INVALID
        for t in (-0.1, 64.5, float("nan"), float("inf")):
            assert _call(dt, times=(0.1, t)) == INVALID, t
        assert _call(dt, flags=2) == INVALID
        assert _call(dt, sel=(1, 0)) == INVALID and _call(dt, sel=(0, 0)) == INVALID and _call(dt, sel=(0, 2)) == INVALID
        assert _call(dt, sel=(0, 1, 2), nodes=(1, 1, 1), edges=(0, 0, 0)) == INVALID      # n_sel > n_graphs
        assert _call(dt, nodes=(5, -1)) == INVALID and _call(dt, edges=(4, -1)) == INVALID
        assert _call(dt, nodes=(5, 1 << 31)) == INVALID
        assert _call(dt, work_bytes=1000) == INVALID             # below min_bytes
        assert _call(dt, work=0x1008) == INVALID                 # misaligned
        for k in (0, 1, 2, 3, 5):
            assert _call(dt, null_at=k) == INVALID, k
        assert _call(dt, work=None) == INVALID
        assert _call(dt, sel=(), nodes=(), edges=()) == 0        # an empty selection: done, nothing read
    assert _call(True, null_at=4) == INVALID
    assert b"tlc_hks_sparse_batch_dt" in _lib.lib().tlc_last_error()


@pytest.mark.parametrize("n,seed", [(1, 0), (2, 0), (65, 3), (300, 4), (700, 1), (900, 2)])
def test_restatement_against_eigh(n, seed):
    e = cases.random_connected(n, seed)
    csr = cases.Csr(n, e)
    for t in TIMES:
        v, d = cases.restate(n, e, t, csr=csr)
        rv, rd = cases.eigh_reference(n, e, t)
        ev, ed = np.abs(v - rv).max(), np.abs(d - rd).max()
        print("n %d t %g K %d: value %.2e derivative %.2e" % (n, t, cases.terms(t), ev, ed))
        assert ev <= 1e-11 and ed <= 2e-11


def test_restatement_against_closed_forms():
    for t in TIMES:
        n, e = cases.star(5000)
        cols = [0, 1, 77, 5000]
        v, d = cases.restate(n, e, t, cols=cols)
        cv, cd = cases.star_closed(5000, t)
        assert np.abs(v - cv[cols]).max() <= 1e-11 and np.abs(d - cd[cols]).max() <= 2e-11, t
        n, e = cases.union(cases.cycle(101), cases.bipartite(3, 70), cases.star(130), isolated=3)
        v, d = cases.restate(n, e, t)
        cv, cd = cases.union_closed([cases.cycle_closed(101, t), cases.bipartite_closed(3, 70, t), cases.star_closed(130, t)], isolated=3)
        assert np.abs(v - cv).max() <= 1e-11 and np.abs(d - cd).max() <= 2e-11, t
    # a graph without edges: 1 and 0; normalised by the lowest index of the maximum
    v, d = cases.restate(5, np.zeros((0, 2), dtype=np.int64), 3.0)
    assert (v == 1.0).all() and (d == 0.0).all()
    f, df = cases.normalise(np.array([0.5, 2.0, 2.0]), np.array([1.0, 3.0, 5.0]))
    assert f[1] == 2.0 / (2.0 + 1e-10) and df[1] == (3.0 - f[1] * 3.0) / (2.0 + 1e-10) and df[2] == (5.0 - f[2] * 3.0) / (2.0 + 1e-10)

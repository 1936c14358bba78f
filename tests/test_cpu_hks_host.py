"""CPU: the host-side surface of the device HKS filtration (hks_backend of the Knowledge_Distillation drop-ins, the TLC_HKS_*
constants of include/tlcgnn.h and their mirrors in _lib).  The kernels themselves: tests/test_gpu_hks.py."""
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _modules():
    from tlc_gnn_amd.Knowledge_Distillation import data_utils_NC as kd_nc, data_utils_LP as kd_lp, data_utils_GC as kd_gc
    return kd_lp, kd_nc, kd_gc


def test_defaults_are_the_host_backend():
    kd_lp, kd_nc, kd_gc = _modules()
    for fn in (kd_lp.compute_persistence_image, kd_nc.compute_persistence_image, kd_gc.compute_persistence_image,
               kd_gc.compute_persistence_image_batch, kd_lp.Vicinities.batch, kd_nc.NodeVicinities.batch):
        assert inspect.signature(fn).parameters["hks_backend"].default == 'host', fn
    assert kd_lp.HKS_BACKENDS == ("host", "device") and kd_lp.hks_host_fallback == 0


def test_unknown_backend_is_a_value_error_before_any_work():
    kd_lp, kd_nc, kd_gc = _modules()
    edges = np.array([[0, 1], [1, 2], [0, 2]])
    for bad in ('gpu', 'Device', None, 1):
        with pytest.raises(ValueError):
            kd_lp.compute_persistence_image(edges, 0, 1, hks_backend=bad)
        with pytest.raises(ValueError):
            kd_nc.compute_persistence_image(edges, 0, hks_backend=bad)
        with pytest.raises(ValueError):
            kd_gc.compute_persistence_image((3, edges), hks_backend=bad)
        with pytest.raises(ValueError):
            kd_gc.compute_persistence_image_batch([(3, edges)], filt='degree', hks_backend=bad)
        with pytest.raises(ValueError):
            kd_lp.Vicinities.batch(None, [[0, 1]], 1, filt='hks', hks_backend=bad)
        with pytest.raises(ValueError):
            kd_nc.NodeVicinities.batch(None, [0], 1, filt='hks', hks_backend=bad)


def test_hks_constants_mirror_the_header_and_the_symbols_are_bound():
    import __graft_entry__ as ge
    ge.build()
    from tlc_gnn_amd import _lib
    header = open(os.path.join(ROOT, "include", "tlcgnn.h")).read()
    val = lambda name: int(re.search(r"#define\s+%s\s+(0x[0-9a-fA-F]+|\d+)" % name, header).group(1), 0)
    assert val("TLC_HKS_NMAX") == _lib.HKS_NMAX >= 256
    assert val("TLC_HKS_LDS_NMAX") == _lib.HKS_LDS_NMAX               # two n x (n + 1) fp64 arrays in 160 KiB of LDS
    assert 2 * _lib.HKS_LDS_NMAX * (_lib.HKS_LDS_NMAX + 1) * 8 < 160 * 1024
    assert val("TLC_HKS_TMAX") == _lib.HKS_TMAX and val("TLC_HKS_NORMALISE") == _lib.HKS_NORMALISE
    assert val("TLC_ST_TOO_LARGE") == _lib.ST_TOO_LARGE == 5
    assert val("TLC_ST_NOT_CONVERGED") == _lib.ST_NOT_CONVERGED and val("TLC_ST_BAD_INPUT") == _lib.ST_BAD_INPUT
    L = _lib.lib()
    for sym in ("tlc_hks_batch", "tlc_hks_batch_work_bytes"):
        assert sym in _lib.SYMBOLS and getattr(L, sym).argtypes, sym


def test_device_backend_has_no_cpu_fallback():
    """Without a GPU hks_backend='device' raises (TlcError: no device); it never computes on the host instead."""
    import torch
    from tlc_gnn_amd import engine, _lib
    if torch.cuda.is_available():
        return
    kd_lp, kd_nc, kd_gc = _modules()
    with pytest.raises((_lib.TlcError, RuntimeError, AssertionError)):
        kd_gc.compute_persistence_image((3, np.array([[0, 1], [1, 2], [0, 2]])), filt='hks', hks_backend='device')
    with pytest.raises(_lib.TlcError):
        engine.hks_batch(torch.tensor([0, 3]), torch.tensor([0, 2]), torch.tensor([[0, 1], [1, 2]], dtype=torch.int32), [0.1])


# ---- what tests/test_gpu_hks_batches.py leans on: the closed forms and the host route's semantics ------------------------------------
def test_closed_forms_and_the_stationary_limit_against_the_host_route():
    """Complete graphs, stars, cycles, complete bipartite graphs at the tier-edge sizes and all eight times: `hks_signature` (scipy's
    eigh) within 1e-11 * max(1, t / 10) of the closed forms of tests/helpers.py, and within the same bound of deg / (2m) at t = 1000
    on random connected graphs.  The worst figure is LAPACK's own error on these degenerate spectra (about 1e-12): it is the margin
    the GPU test's bound has over its reference."""
    from helpers import HKS_CLOSED_FORM_SIZES, HKS_CLOSED_FORM_TIMES, hks_bound, hks_closed_form_cases, hks_stationary, random_connected
    kd_lp, _, _ = _modules()
    cases = hks_closed_form_cases()
    assert len(cases) == 4 * len(HKS_CLOSED_FORM_SIZES) - 1            # no cycle at n = 2
    worst = {t: 0.0 for t in HKS_CLOSED_FORM_TIMES}
    for name, n, e, f in cases:
        for t in HKS_CLOSED_FORM_TIMES:
            d = np.abs(kd_lp.hks_signature(n, e, t) - f(t)).max()
            worst[t] = max(worst[t], d)
            assert d <= hks_bound(t), (name, t, d)
    worst_lim = 0.0
    for n in HKS_CLOSED_FORM_SIZES:
        e = random_connected(n, 1000 + n)
        d = np.abs(kd_lp.hks_signature(n, e, 1000.0) - hks_stationary(n, e)).max()
        worst_lim = max(worst_lim, d)
        assert d <= hks_bound(1000.0), (n, d)
    print("worst |host - closed form| per t: %s; worst |host(t=1000) - deg/2m| %.2e"
          % (", ".join("t=%g %.2e" % kv for kv in worst.items()), worst_lim))
    assert max(worst.values()) <= 5e-12                                # measured 1.0e-12


MULTI = np.array([(0, 1), (1, 2), (2, 3), (1, 3)])


def test_host_route_multigraph_semantics():
    """scipy's CSR sums repeated entries: every edge in both directions is the Laplacian of 2A, i.e. that of A (equal to 1e-14);
    one edge repeated is a different, weighted graph (values differ by more than 1e-4).  The device route refuses both."""
    kd_lp, _, _ = _modules()
    both = np.concatenate([MULTI, MULTI[:, ::-1]])
    once_more = np.concatenate([MULTI, MULTI[:1]])
    for t in (0.1, 10.0):
        simple = kd_lp.hks_signature(4, MULTI, t)
        assert np.abs(kd_lp.hks_signature(4, both, t) - simple).max() <= 1e-14
        assert np.abs(kd_lp.hks_signature(4, once_more, t) - simple).max() > 1e-4


def test_host_route_isolated_nodes_and_no_edges():
    """A node of degree 0 has Laplacian row 0: signature exactly 1 at every t.  (5, [(0,1),(3,4)]) at t = 10: two K2 and an isolated
    node, normalised [.5, .5, 1, .5, .5] up to exp(-20)/2.  m = 0: all 1.0 un-normalised, 1 / (1 + 1e-10) normalised."""
    kd_lp, _, kd_gc = _modules()
    v = kd_lp.hks_signature(5, np.array([(0, 1), (3, 4)]), 10.0)
    assert v[2] == 1.0 and np.abs(v - [.5, .5, 1, .5, .5]).max() <= 1e-8 + 1e-15
    assert np.abs(kd_gc.hks_filtration(5, np.array([(0, 1), (3, 4)]), 10.0) - [.5, .5, 1, .5, .5]).max() <= 1e-8
    for n in (1, 2, 7, 33):
        for t in (0.0, 0.1, 1000.0):
            v = kd_lp.hks_signature(n, np.zeros((0, 2), dtype=np.int64), t)
            assert v.shape == (n,) and np.array_equal(v, np.ones(n)), (n, t)
            assert np.array_equal(kd_gc.hks_filtration(n, np.zeros((0, 2), dtype=np.int64), t), np.ones(n) / (1.0 + 1e-10))

"""CPU: the host-side surface of the large HKS tier (tlc_hks_large_batch, csrc/hks_large.hip): the TLC_HKS_LARGE_* constants and their
mirrors in _lib, the two symbols, the hks_large keyword of the Knowledge_Distillation drop-ins, and the workspace arithmetic of
tlc_hks_large_work_bytes, which needs no device.  The kernels themselves: tests/test_gpu_hks_large.py."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _modules():
    from tlc_gnn_amd.Knowledge_Distillation import data_utils_NC as kd_nc, data_utils_LP as kd_lp, data_utils_GC as kd_gc
    return kd_lp, kd_nc, kd_gc


def _lib_built():
    import __graft_entry__ as ge
    ge.build()
    from tlc_gnn_amd import _lib
    return _lib


def test_large_constants_mirror_the_header_and_the_symbols_are_bound():
    _lib = _lib_built()
    header = open(os.path.join(ROOT, "include", "tlcgnn.h")).read()
    assert int(re.search(r"#define\s+TLC_HKS_LARGE_NMAX\s+(\d+)", header).group(1)) == _lib.HKS_LARGE_NMAX == 4096
    assert float(re.search(r"#define\s+TLC_HKS_LARGE_TIME_MAX\s+([0-9.]+)", header).group(1)) == _lib.HKS_LARGE_TIME_MAX == 64.0
    assert _lib.HKS_LARGE_NMAX > _lib.HKS_NMAX
    src = open(os.path.join(ROOT, "tlc-gnn_amd", "csrc", "hks_large.hip")).read()
    assert int(re.search(r"#define\s+HKSL_T\s+(\d+)", src).group(1)) == _lib.HKS_LARGE_TILE
    assert int(re.search(r"#define\s+HKSL_KS\s+(\d+)", src).group(1)) == _lib.HKS_LARGE_KSTEP
    L = _lib.lib()
    assert "tlc_hks_large_work_bytes" in _lib.SYMBOLS and len(L.tlc_hks_large_work_bytes.argtypes) == 5
    assert "tlc_hks_large_batch" in _lib.SYMBOLS and len(L.tlc_hks_large_batch.argtypes) == 17


def test_keyword_defaults_and_check():
    kd_lp, kd_nc, kd_gc = _modules()
    assert kd_lp.HKS_LARGE == ("host", "device") and kd_lp.HKS_BACKENDS == ("host", "device")
    assert kd_lp.hks_large_device == 0
    fns = (kd_lp.compute_persistence_image, kd_nc.compute_persistence_image, kd_gc.compute_persistence_image,
           kd_gc.compute_persistence_image_batch, kd_lp.Vicinities.batch, kd_nc.NodeVicinities.batch, kd_lp.hks_filtration_device)
    assert len(fns) == 7
    for fn in fns:
        assert inspect.signature(fn).parameters["hks_large"].default == 'host', fn
    kd_lp.check_hks_large('host')
    kd_lp.check_hks_large('device')
    for bad in ('gpu', 'Device', None, 1):
        with pytest.raises(ValueError):
            kd_lp.check_hks_large(bad)


def test_unknown_hks_large_is_a_value_error_before_any_work():
    kd_lp, kd_nc, kd_gc = _modules()
    edges = np.array([[0, 1], [1, 2], [0, 2]])
    with pytest.raises(ValueError):
        kd_lp.compute_persistence_image(edges, 0, 1, hks_large='gpu')
    with pytest.raises(ValueError):
        kd_nc.compute_persistence_image(edges, 0, hks_large='gpu')
    with pytest.raises(ValueError):
        kd_gc.compute_persistence_image((3, edges), hks_large='gpu')
    with pytest.raises(ValueError):
        kd_gc.compute_persistence_image_batch([(3, edges)], filt='degree', hks_large='gpu')
    with pytest.raises(ValueError):
        kd_lp.Vicinities.batch(None, [[0, 1]], 1, filt='hks', hks_large='gpu')
    with pytest.raises(ValueError):
        kd_nc.NodeVicinities.batch(None, [0], 1, filt='hks', hks_large='gpu')


def _work_bytes(L, nodes, n_times=1):
    lo, hi = C.c_int64(-1), C.c_int64(-1)
    arr = (C.c_int64 * max(len(nodes), 1))(*nodes)
    rc = L.tlc_hks_large_work_bytes(arr, len(nodes), n_times, C.byref(lo), C.byref(hi))
    return rc, lo.value, hi.value


def test_work_bytes_contract():
    """Pure host arithmetic: min_bytes <= all_bytes, both 0 for an empty selection; min_bytes depends on the largest count only,
    all_bytes grows with every graph (an empty or an over-large one included: each has a descriptor); three np x np fp64 matrices,
    np = n rounded up to the tile, dominate; refusals are return codes."""
    _lib = _lib_built()
    from tlc_gnn_amd import engine
    L = _lib.lib()
    assert _work_bytes(L, []) == (0, 0, 0)
    lo = C.c_int64(-1)
    assert L.tlc_hks_large_work_bytes(None, 0, 1, C.byref(lo), C.byref(lo)) == 0 and lo.value == 0
    rc, lo1, hi1 = _work_bytes(L, [300])
    assert rc == 0 and 0 < lo1 == hi1
    T = _lib.HKS_LARGE_TILE
    mats = lambda n: 3 * 8 * (-(-n // T) * T) ** 2
    assert mats(300) <= lo1 <= mats(300) + 64 * 1024
    rc, lo2, hi2 = _work_bytes(L, [300, 257, 300, 1205, 40])
    assert rc == 0 and lo2 <= hi2
    assert lo2 == _work_bytes(L, [1205])[1] == _work_bytes(L, [1, 1205, 1205])[1]           # the largest count only
    assert mats(1205) <= lo2 <= mats(1205) + 64 * 1024
    assert hi2 >= sum(mats(n) for n in (300, 257, 300, 1205, 40))
    grow, prev = [], 0
    for k in range(1, 8):
        rc, _, hi = _work_bytes(L, [300, 257, 0, 1205, 40, 5000, 300][:k])
        assert rc == 0 and hi > prev
        prev = hi
    assert _work_bytes(L, [300], 8)[0] == 0
    assert _work_bytes(L, [_lib.HKS_LARGE_NMAX])[1] >= mats(4096) == 3 * 8 * 4096 * 4096
    assert engine.hks_large_work_bytes([300, 257, 300, 1205, 40]) == (lo2, hi2)
    # refusals
    assert _work_bytes(L, [300], 0)[0] == 1 and _work_bytes(L, [300], _lib.HKS_TMAX + 1)[0] == 1
    assert _work_bytes(L, [300, -1])[0] == 1
    a, b = C.c_int64(0), C.c_int64(0)
    arr = (C.c_int64 * 1)(300)
    assert L.tlc_hks_large_work_bytes(None, 1, 1, C.byref(a), C.byref(b)) == 1
    assert L.tlc_hks_large_work_bytes(arr, 1, 1, None, C.byref(b)) == 1
    assert L.tlc_hks_large_work_bytes(arr, 1, 1, C.byref(a), None) == 1
    assert L.tlc_hks_large_work_bytes(arr, -1, 1, C.byref(a), C.byref(b)) == 1
    with pytest.raises(_lib.TlcError):
        engine.hks_large_work_bytes([300], 0)


def test_large_tier_has_no_cpu_fallback():
    """Without a GPU engine.hks_large_batch raises (TlcError: no device); it never computes on the host instead."""
    import torch
    from tlc_gnn_amd import engine, _lib
    if torch.cuda.is_available():
        return
    with pytest.raises(_lib.TlcError):
        engine.hks_large_batch(torch.tensor([0, 3]), torch.tensor([0, 2]), torch.tensor([[0, 1], [1, 2]], dtype=torch.int32), [0], [3], [0.1])

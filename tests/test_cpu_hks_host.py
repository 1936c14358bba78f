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

"""CPU: the host-side surface of the device degree / centrality / clustering filtrations (struct_backend of the Knowledge_Distillation
drop-ins, the TLC_STRUCT_* constants of include/tlcgnn.h and their mirrors in _lib), and the host function's exact values on the small
graphs that tests/test_gpu_struct.py compares the kernels against.  The kernels themselves: tests/test_gpu_struct.py."""
import inspect
import os
import re

import numpy as np
import pytest

import struct_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _modules():
    from tlc_gnn_amd.Knowledge_Distillation import data_utils_NC as kd_nc, data_utils_LP as kd_lp, data_utils_GC as kd_gc
    return kd_lp, kd_nc, kd_gc


def _callables():
    kd_lp, kd_nc, kd_gc = _modules()
    return (kd_lp.compute_persistence_image, kd_nc.compute_persistence_image, kd_gc.compute_persistence_image,
            kd_gc.compute_persistence_image_batch, kd_lp.Vicinities.batch, kd_nc.NodeVicinities.batch)


def test_defaults_are_the_host_backend():
    kd_lp, _, _ = _modules()
    for fn in _callables():
        assert inspect.signature(fn).parameters["struct_backend"].default == 'host', fn
        assert inspect.signature(fn).parameters["hks_backend"].default == 'host', fn
    assert kd_lp.STRUCT_BACKENDS == ("host", "device")
    assert kd_lp.STRUCT_DEVICE_FILTS == sc.KINDS


def test_unknown_backend_is_a_value_error_before_any_work():
    kd_lp, kd_nc, kd_gc = _modules()
    edges = np.array([[0, 1], [1, 2], [0, 2]])
    for bad in ('gpu', 'Device', None, 1):
        with pytest.raises(ValueError):
            kd_lp.check_struct_backend(bad)
        with pytest.raises(ValueError):
            kd_lp.compute_persistence_image(edges, 0, 1, filt='degree', struct_backend=bad)
        with pytest.raises(ValueError):
            kd_nc.compute_persistence_image(edges, 0, filt='clustering', struct_backend=bad)
        with pytest.raises(ValueError):
            kd_gc.compute_persistence_image((3, edges), filt='degree', struct_backend=bad)
        with pytest.raises(ValueError):
            kd_gc.compute_persistence_image_batch([(3, edges)], filt='clustering', struct_backend=bad)
        with pytest.raises(ValueError):                                   # self = None: nothing of the object is touched before the check
            kd_lp.Vicinities.batch(None, [[0, 1]], 1, filt='degree', struct_backend=bad)
        with pytest.raises(ValueError):
            kd_nc.NodeVicinities.batch(None, [0], 1, filt='centrality', struct_backend=bad)
    for ok in ('host', 'device'):
        kd_lp.check_struct_backend(ok)


def test_host_backend_refusals_are_unchanged():
    """struct_backend='host' (the default): the graph-classification batch still refuses 'centrality' and 'clustering' without
    `filtrations`, before any device work."""
    _, _, kd_gc = _modules()
    edges = np.array([[0, 1], [1, 2], [0, 2]])
    for filt in ('centrality', 'clustering'):
        with pytest.raises(NotImplementedError):
            kd_gc.compute_persistence_image_batch([(3, edges)], filt=filt)
        with pytest.raises(NotImplementedError):
            kd_gc.compute_persistence_image_batch([(3, edges)], filt=filt, struct_backend='host')
        with pytest.raises(NotImplementedError):
            kd_gc.compute_persistence_image((3, edges), filt=filt)


def test_struct_constants_mirror_the_header_and_the_symbols_are_bound():
    from tlc_gnn_amd import _lib
    _lib.build()                                                  # make: nothing to do when the library is up to date
    header = open(os.path.join(ROOT, "include", "tlcgnn.h")).read()
    val = lambda name: int(re.search(r"#define\s+%s\s+(0x[0-9a-fA-F]+|\d+)" % name, header).group(1), 0)
    assert val("TLC_STRUCT_DEGREE") == _lib.STRUCT_DEGREE == 0x1
    assert val("TLC_STRUCT_CENTRALITY") == _lib.STRUCT_CENTRALITY == 0x2
    assert val("TLC_STRUCT_CLUSTERING") == _lib.STRUCT_CLUSTERING == 0x4
    assert val("TLC_STRUCT_NORMALISE") == _lib.STRUCT_NORMALISE == 0x100
    assert val("TLC_STRUCT_WAVE_NMAX") == _lib.STRUCT_WAVE_NMAX == 64          # a u64 adjacency row per lane
    assert val("TLC_STRUCT_LDS_SMALL_NMAX") == _lib.STRUCT_LDS_SMALL_NMAX
    assert val("TLC_STRUCT_LDS_NMAX") == _lib.STRUCT_LDS_NMAX
    assert val("TLC_STRUCT_BITMAP_BITS") == _lib.STRUCT_BITMAP_BITS
    assert _lib.STRUCT_WAVE_NMAX < _lib.STRUCT_LDS_SMALL_NMAX < _lib.STRUCT_LDS_NMAX < _lib.STRUCT_BITMAP_BITS
    assert val("TLC_ST_BAD_INPUT") == _lib.ST_BAD_INPUT
    assert list(_lib.STRUCT_KINDS) == list(sc.KINDS) and list(_lib.STRUCT_KINDS.values()) == [0x1, 0x2, 0x4]
    L = _lib.lib()
    for sym in ("tlc_struct_batch", "tlc_struct_batch_work_bytes"):
        assert sym in _lib.SYMBOLS and getattr(L, sym).argtypes, sym
    assert len(L.tlc_struct_batch.argtypes) == 13 and len(L.tlc_struct_batch_work_bytes.argtypes) == 5


def test_lds_budget_of_the_bitmap_tiers():
    """The adjacency bitmap of the largest LDS-tier graph -- TLC_STRUCT_LDS_NMAX rows of ceil(n / 64) + 1 u64 words (the odd row
    length of the bank rule) -- with its two u32 count arrays and the control block, and the CSR tier's sixteen neighbour bitmaps with
    its scan scratch, both stay below the 160 KiB of a gfx950 workgroup."""
    from tlc_gnn_amd import _lib
    n = _lib.STRUCT_LDS_NMAX
    assert n % 64 == 0 and _lib.STRUCT_LDS_SMALL_NMAX % 64 == 0
    rows = n * (n // 64 + 1) * 8
    assert n * (n // 64) * 8 <= 128 * 1024                       # the bitmap proper
    assert rows + 2 * 4 * n + 32 < 160 * 1024
    assert 16 * _lib.STRUCT_BITMAP_BITS // 8 + 1024 * 8 + 32 < 160 * 1024
    assert n * (n - 1) < 2 ** 32                                  # t of the LDS tiers fits 32 bits
    assert _lib.STRUCT_BITMAP_BITS >= 65535


def test_device_backend_has_no_cpu_fallback():
    """Without a GPU struct_backend='device' raises (TlcError: no device); it never computes on the host instead."""
    import torch
    from tlc_gnn_amd import engine, _lib
    if torch.cuda.is_available():
        return
    _, _, kd_gc = _modules()
    tri = np.array([[0, 1], [1, 2], [0, 2]])
    for filt in sc.KINDS:
        with pytest.raises((_lib.TlcError, RuntimeError, AssertionError)):
            kd_gc.compute_persistence_image_batch([(3, tri)], filt=filt, struct_backend='device')
    with pytest.raises((_lib.TlcError, RuntimeError, AssertionError)):
        kd_gc.compute_persistence_image((3, tri), filt='degree', mode='filtration', struct_backend='device')
    with pytest.raises(_lib.TlcError):
        engine.struct_batch(torch.tensor([0, 3]), torch.tensor([0, 2]), torch.tensor([[0, 1], [1, 2]], dtype=torch.int32), 'clustering')


def test_struct_kinds_names_and_row_order():
    from tlc_gnn_amd import engine
    assert engine.struct_kinds('clustering') == (0x4, ['clustering'])
    assert engine.struct_kinds(['clustering', 'degree']) == (0x5, ['degree', 'clustering'])
    assert engine.struct_kinds(sc.KINDS) == (0x7, list(sc.KINDS))
    for bad in ([], 'hks', ['degree', 'degree'], ['degree', 'ricci']):
        with pytest.raises(ValueError):
            engine.struct_kinds(bad)


def test_host_function_on_the_closed_forms():
    """K5, a star, K2,3, one node and three isolated nodes: `structural_filtration` returns exactly raw / (max + 1e-10) of the values
    worked out by hand -- d; d * (1 / (n - 1)), 1 for the one-node graph; t / (d (d - 1)), 0 without triangles -- alone and in one
    packed batch.  These are the values the GPU file compares the kernels against."""
    cases = sc.closed_form_cases()
    assert [c[0] for c in cases] == ["K5", "star7", "K2,3", "one node", "three isolated"]
    one = cases[3][2]
    assert (one["degree"], one["centrality"], one["clustering"]) == ([0.0], [1.0], [0.0])      # before the normalisation
    packed = sc.pack([g for _, g, _ in cases])
    for kind in sc.KINDS:
        whole = sc.host(kind, packed)
        for k, (name, g, raw) in enumerate(cases):
            want = sc.normalised(raw[kind])
            assert np.array_equal(sc.host(kind, sc.pack([g])), want), (name, kind)
            assert np.array_equal(whole[packed[0][k]:packed[0][k + 1]], want), (name, kind)
    # K5: every value is the maximum; 4 / (4 + 1e-10) and 1 / (1 + 1e-10) are not 1.0
    assert sc.host("degree", sc.pack([cases[0][1]]))[0] == 4.0 / (4.0 + 1e-10) < 1.0
    assert sc.host("clustering", sc.pack([cases[0][1]]))[0] == 1.0 / (1.0 + 1e-10) < 1.0
    assert np.array_equal(sc.host("clustering", sc.pack([cases[1][1]])), np.zeros(7))           # 0 / (0 + 1e-10)


def test_planted_clique_has_the_expected_counts():
    """the planted clique of the GPU file's large cases: its k members have d = k - 1 and t = (k - 1)(k - 2), so the host function
    gives them the graph's maximum of 'clustering', 1 / (1 + 1e-10)"""
    n, e, members = sc.planted_clique(300, 40, 1)
    assert len(np.unique(e, axis=0)) == len(e) and (e[:, 0] < e[:, 1]).all()
    deg = np.bincount(e.reshape(-1), minlength=n)
    assert (deg[members] == 39).all()
    f = sc.host("clustering", sc.pack([(n, e)]))
    assert np.array_equal(f[members], np.full(40, (39.0 * 38.0) / (39.0 * 38.0) / (1.0 + 1e-10)))

"""No GPU: the host side of tlc_graph_components and of the packed route of data_utils_GC -- the numpy restatement of the contract
(tests/gc_cases.py) against `data_utils_GC.largest_component` and scipy, the exported symbols and the mirrored constant, the workspace
arithmetic, the entry's refusals that come before any launch, `pack_dataset`'s arithmetic and the keyword checks."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gc_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from tlc_gnn_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize("name", [c[0] for c in gc.cases()])
def test_restatement_equals_largest_component(name):
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    from tlc_gnn_amd.Knowledge_Distillation.data_utils_GC import largest_component
    n, e = dict(gc.cases())[name]
    r = gc.references()[name]
    assert r["new_id"].shape == (n,) and r["out_edges"].shape == (r["m"], 2)
    if n == 0:
        assert (r["k"], r["m"], r["c"], r["s"]) == (0, 0, 0, 0)
        return
    k, ce = largest_component(n, e)
    assert r["k"] == k and np.array_equal(r["out_edges"], ce), name
    _, de = gc.dedup(n, e)
    assert r["s"] == len(de)
    a = sp.coo_matrix((np.ones(len(de), dtype=np.int8), (de[:, 0], de[:, 1])), shape=(n, n))
    assert r["c"] == connected_components(a, directed=False)[0]
    kept = np.flatnonzero(r["new_id"] >= 0)
    assert len(kept) == k and np.array_equal(r["new_id"][kept], np.arange(k))             # ascending order of the old ids
    if name.startswith("subset") or name.startswith("twin"):
        assert 1 < k < n, "the case is meant to have a largest component that is a strict subset"
    if name.startswith("isolated"):
        assert (r["k"], r["m"], r["c"]) == (1, 0, n) and r["new_id"][0] == 0               # the tie goes to node 0
    if name.startswith("pairs"):
        assert (r["k"], r["m"], r["c"]) == (2, 1, n // 2) and r["new_id"][0] == 0 and not (e[0] == 0).any()
    if name.startswith("path") or name.startswith("star"):
        assert (r["k"], r["m"], r["c"], r["s"]) == (n, n - 1, 1, n - 1)


def test_the_examples_of_the_contract():
    from tlc_gnn_amd.Knowledge_Distillation.data_utils_GC import largest_component
    k, ce = largest_component(*gc.FIVE)
    assert k == 2 and ce.tolist() == [[0, 1]]
    r = gc.restate(*gc.FIVE)
    assert (r["k"], r["m"], r["c"], r["s"]) == (2, 1, 3, 2) and r["new_id"].tolist() == [0, -1, 1, -1, -1] and r["out_edges"].tolist() == [[0, 1]]
    r = gc.restate(7, gc.E0)
    assert (r["k"], r["m"], r["c"], r["s"]) == (1, 0, 7, 0) and r["new_id"].tolist() == [0] + [-1] * 6
    assert largest_component(7, gc.E0)[0] == 1


def test_symbols_and_constant(L):
    from tlc_gnn_amd import _lib
    header = open(os.path.join(ROOT, "include", "tlcgnn.h")).read()
    assert int(re.search(r"#define\s+TLC_CC_WAVE_NMAX\s+(\d+)", header).group(1)) == _lib.CC_WAVE_NMAX == 64
    for sym in ("tlc_graph_components", "tlc_graph_components_work_bytes"):
        assert sym in _lib.SYMBOLS and hasattr(L, sym) and re.search(r"\b%s\s*\(" % sym, header)
    assert len(L.tlc_graph_components.argtypes) == 14 and len(L.tlc_graph_components_work_bytes.argtypes) == 4


def _bytes(L, B, N, M):
    need = C.c_int64(-1)
    rc = L.tlc_graph_components_work_bytes(B, N, M, C.byref(need))
    return rc, need.value


def test_work_bytes_are_monotone_and_refuse_nonsense(L):
    grid = [0, 1, 63, 64, 65, 1000, 4096, 4097, 70000, 1 << 20, (1 << 31) - 1]
    for fixed in ((5, 100, 300), (1, 64, 10), (4096, 1 << 20, 1 << 22), (0, 0, 0)):
        for axis in range(3):
            last = -1
            for v in grid:
                args = list(fixed)
                args[axis] = v
                rc, b = _bytes(L, *args)
                assert rc == 0 and b >= last and b >= 256, (args, b, last)
                last = b
    from tlc_gnn_amd import engine
    assert engine.graph_components_work_bytes(5, 100, 300) == _bytes(L, 5, 100, 300)[1]
    # a batch that cannot hold a WIDE graph needs the head and the list only
    assert _bytes(L, 100, 64, 1 << 20)[1] < 4096 < _bytes(L, 100, 65, 1 << 20)[1]
    for args in ((-1, 1, 1), (1, -1, 1), (1, 1, -1), (1 << 31, 1, 1), (1, 1 << 31, 1), (1, 1, 1 << 31)):
        assert _bytes(L, *args) == (1, -1), args
    assert L.tlc_graph_components_work_bytes(1, 1, 1, None) == 1


def test_the_entry_refuses_before_any_launch(L):
    """Null pointers, negative or oversized totals, a short or misaligned workspace: TLC_ERR_INVALID_ARG from the host checks alone --
    no device is needed to get there.  The pointers handed in are never dereferenced."""
    fake = C.c_void_p(1 << 20)                     # 16-byte aligned, non-null, never touched
    need = _bytes(L, 3, 100, 50)[1]

    def call(np_=fake, ep=fake, ed=fake, B=3, N=100, M=50, mx=-1, info=fake, nid=fake, oe=fake, st=fake, w=fake, wb=need):
        return L.tlc_graph_components(np_, ep, ed, B, N, M, mx, info, nid, oe, st, w, wb, None)
    for kw in (dict(np_=None), dict(ep=None), dict(ed=None), dict(info=None), dict(nid=None), dict(oe=None), dict(st=None), dict(w=None),
               dict(B=-1), dict(N=-1), dict(M=-1), dict(N=1 << 31), dict(M=1 << 31), dict(wb=need - 1), dict(wb=0),
               dict(w=C.c_void_p((1 << 20) + 8))):
        assert call(**kw) == 1, kw
        assert L.tlc_last_error()
    assert call(B=0, np_=None, ep=None, ed=None, info=None, nid=None, oe=None, st=None, w=None, wb=0) == 0      # nothing to do, nothing read


class _Item:
    def __init__(self, n, e):
        import torch
        self.num_nodes, self.edge_index = n, torch.from_numpy(np.ascontiguousarray(np.asarray(e, dtype=np.int64).reshape(-1, 2).T))


def test_pack_dataset_against_a_per_item_concatenation(monkeypatch):
    """PyG-like items and tuples mixed, an edgeless item among them; the device copy is replaced by the identity (no GPU here)."""
    import torch
    from tlc_gnn_amd.Knowledge_Distillation import data_utils_GC as kd
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **k: self)
    graphs = gc.route_graphs(n_graphs=40)
    data = [_Item(*g) if i % 3 == 0 else g for i, g in enumerate(graphs)]
    for gn in (None, 17, 0):
        node_ptr, edge_ptr, edges = kd.pack_dataset(data, gn)
        use = graphs if gn is None else graphs[:gn]
        assert node_ptr.dtype == edge_ptr.dtype == torch.int64 and edges.dtype == torch.int32 and tuple(edges.shape) == (sum(len(g[1]) for g in use), 2)
        assert node_ptr.tolist() == np.concatenate([[0], np.cumsum([g[0] for g in use])]).tolist()
        for i, (n, e) in enumerate(use):
            assert np.array_equal(edges[edge_ptr[i]:edge_ptr[i + 1]].numpy(), e)


def test_unknown_keywords_are_refused():
    """component / hks_large / pd_large are checked before anything touches the device."""
    import torch
    from tlc_gnn_amd.Knowledge_Distillation import data_utils_GC as kd
    ptr, e = torch.tensor([0, 3]), torch.tensor([[0, 1], [1, 2]], dtype=torch.int32)
    for kw in (dict(component="biggest"), dict(hks_large="gpu"), dict(pd_large="no")):
        with pytest.raises(ValueError):
            kd.ground_truth_packed(ptr, ptr, e, **kw)
    with pytest.raises(NotImplementedError):
        kd.ground_truth_packed(ptr, ptr, e, filt="ricci")
    assert kd.COMPONENTS == ("largest", "whole")

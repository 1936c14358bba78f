"""GPU: tlc_graph_components (csrc/gc_prep.hip) against the numpy restatement of its contract (tests/gc_cases.py, itself pinned to
`data_utils_GC.largest_component` and scipy by tests/test_cpu_gc_packed_host.py), and the packed route of data_utils_GC
(`ground_truth_packed`, `call_packed`, `evaluate_packed`) against today's per-graph route with the device backends.

Every comparison is np.array_equal / torch.equal: the kernel is integer arithmetic, and the packed route runs the same kernels on the
same packed input as the route it is compared with.  The golden's bounds are those of tests/test_gpu_pdgnn.py for the same file."""
import ctypes as C
import os

import numpy as np
import pytest

import gc_cases as gc
from helpers import same_multiset

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SENTINEL = -7


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _cuda(packed):
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in packed)


def _run(packed, **kw):
    """engine.graph_components -> (info, new_id, out_edges, status) as numpy; untouched entries hold -1"""
    from tlc_gnn_amd import engine
    r = engine.graph_components(*_cuda(packed), **kw)
    return tuple(r[k].cpu().numpy() for k in ("info", "new_id", "out_edges", "status"))


def _check(got, packed, refs, what="", sentinel=-1):
    info, new_id, out_edges, status = got
    e_info, e_new, e_out = gc.expected(packed, refs, sentinel)
    assert np.array_equal(status, [7 if r is None else 0 for r in refs]), what
    assert np.array_equal(info, e_info), (what, info[(info != e_info).any(1)][:4], e_info[(info != e_info).any(1)][:4])
    assert np.array_equal(new_id, e_new), what
    assert np.array_equal(out_edges, e_out), what


class Raw:
    """the C entry on caller-held buffers: outputs prefilled with SENTINEL, one workspace, a graph's solo call written into its own slot"""

    def __init__(self, torch, packed, work_factor=1, misalign=0):
        from tlc_gnn_amd import _lib, engine
        self.torch, self.L, self._lib = torch, _lib.lib(), _lib
        self.np_, self.ep, self.ed = _cuda(packed)
        self.B, self.N, self.M = len(packed[0]) - 1, int(packed[0][-1]) if len(packed[0]) else 0, len(packed[2])
        full = lambda shape, dt: torch.full(shape, SENTINEL & 0xFF if dt == torch.uint8 else SENTINEL, dtype=dt).cuda()
        self.info, self.new_id = full((max(self.B, 1), 4), torch.int32), full((max(self.N, 1),), torch.int32)
        self.out_edges, self.status = full((max(self.M, 1), 2), torch.int32), full((max(self.B, 1),), torch.uint8)
        self.need = engine.graph_components_work_bytes(self.B, self.N, self.M)
        self.work = torch.empty(self.need * work_factor + 64, dtype=torch.uint8).cuda()
        # per graph [0, n] and [0, m]: the offsets of its solo call
        solo = np.zeros((max(self.B, 1), 4), dtype=np.int64)
        solo[:self.B, 1], solo[:self.B, 3] = np.diff(packed[0]), np.diff(packed[1])
        self.solo_ptr, self.h = torch.from_numpy(solo).cuda(), (np.asarray(packed[0]), np.asarray(packed[1]))

    def call(self, work_bytes=None, work_off=0, **null):
        p = lambda name, t: None if null.get(name) else C.c_void_p(t.data_ptr())
        return self.L.tlc_graph_components(p("node_ptr", self.np_), p("edge_ptr", self.ep), p("edges", self.ed), self.B, self.N, self.M, -1, p("info", self.info),
                                           p("new_id", self.new_id), p("out_edges", self.out_edges), p("status", self.status),
                                           None if null.get("work") else C.c_void_p(self.work.data_ptr() + work_off),
                                           self.work.numel() - 64 if work_bytes is None else work_bytes, self._lib.stream_ptr())

    def solo(self, g):
        """graph g alone (B = 1, its own totals), reading its slice of the input and writing its slots of the same output buffers"""
        n0, e0 = int(self.h[0][g]), int(self.h[1][g])
        n, m = int(self.h[0][g + 1]) - n0, int(self.h[1][g + 1]) - e0
        at = lambda t, off, size: C.c_void_p(t.data_ptr() + off * size)
        return self.L.tlc_graph_components(at(self.solo_ptr, 4 * g, 8), at(self.solo_ptr, 4 * g + 2, 8), at(self.ed, e0, 8), 1, n, m, -1, at(self.info, g, 16),
                                           at(self.new_id, n0, 4), at(self.out_edges, e0, 8), at(self.status, g, 1), C.c_void_p(self.work.data_ptr()),
                                           self.work.numel() - 64, self._lib.stream_ptr())

    def outputs(self):
        self.torch.cuda.synchronize()
        return tuple(t.cpu().numpy() for t in (self.info[:self.B], self.new_id[:self.N], self.out_edges[:self.M], self.status[:self.B]))


# ---- the kernel against the restatement -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in gc.cases()])
def test_each_case_alone(torch_cuda, name):
    g = dict(gc.cases())[name]
    packed = gc.pack([g])
    _check(_run(packed), packed, [gc.references()[name]], name)
    _check(_run(packed, total_nodes=g[0], max_nodes=g[0]), packed, [gc.references()[name]], name)       # the caller's bound changes nothing


def test_all_cases_in_one_batch(torch_cuda):
    """Both classes in one call, the WIDE graphs together in its device-wide passes -- among them, adjacent, two graphs with identical
    local edge lists, an edgeless one and another one, where the segments of the sort and of the scans meet."""
    names = [c[0] for c in gc.cases()]
    assert names[-4:] == ["twin a", "twin b", "edgeless wide", "after the edgeless"]
    packed = gc.pack([c[1] for c in gc.cases()])
    refs = [gc.references()[n] for n in names]
    _check(_run(packed), packed, refs)
    rev = gc.pack([c[1] for c in gc.cases()][::-1])
    _check(_run(rev), rev, refs[::-1], "reversed")


def test_a_bound_of_64_nodes_runs_the_wave_class_alone(torch_cuda):
    """max_nodes <= TLC_CC_WAVE_NMAX: the same results for the graphs under it, TLC_ST_BAD_INPUT for one above it."""
    cases = [c for c in gc.cases() if c[1][0] <= 64]
    packed = gc.pack([c[1] for c in cases] * 3)                                 # more than 64 nodes in all
    assert packed[0][-1] > 64
    _check(_run(packed, max_nodes=64), packed, [gc.references()[c[0]] for c in cases] * 3)
    mixed = gc.pack([gc.FIVE, dict(gc.cases())["n65"], gc.FIVE])
    _check(_run(mixed, max_nodes=64), mixed, [gc.restate(*gc.FIVE), None, gc.restate(*gc.FIVE)])


# ---- slots and status ---------------------------------------------------------------------------------------------------------------------
def test_bad_ids_between_good_graphs(torch_cuda):
    """An id == n and an id of -1, in a graph of either class, between good graphs of both classes: only those are refused, their slots
    and info rows keep the sentinel, the neighbours equal their solo results (the references)."""
    c = dict(gc.cases())
    good = ["five", "n129", "n64", "subset200"]
    bad = [(5, np.array([[0, 1], [1, 5], [2, 3]])), (5, np.array([[0, 1], [-1, 2]])), (100, np.array([[0, 1], [3, 100], [7, 8]])),
           (100, np.array([[99, 98], [5, -1]]))]
    graphs, refs = [], []
    for i, b in enumerate(bad):
        graphs += [c[good[i]], (b[0], b[1].astype(np.int64))]
        refs += [gc.references()[good[i]], None]
    graphs.append(c["path64"])
    refs.append(gc.references()["path64"])
    packed = gc.pack(graphs)
    _check(_run(packed), packed, refs)
    raw = Raw(torch_cuda, packed)
    assert raw.call() == 0
    info, new_id, out_edges, status = raw.outputs()
    e_info, e_new, e_out = gc.expected(packed, refs, SENTINEL)
    assert np.array_equal(info, e_info) and np.array_equal(new_id, e_new) and np.array_equal(out_edges, e_out)    # rows beyond m keep it too
    assert status.tolist() == [0, 7] * 4 + [0]


def test_offsets_out_of_order(torch_cuda):
    """A graph whose offsets decrease, or pass the totals, is refused and nothing of it is written."""
    g = [gc.FIVE, (3, np.array([[0, 1]])), gc.FIVE]
    node_ptr, edge_ptr, edges = gc.pack(g)
    for which, arr in (("nodes", node_ptr), ("edges", edge_ptr)):
        a = arr.copy()
        a[1], a[2] = arr[2], arr[1]                                           # graph 1 runs backwards (its neighbours overlap now)
        packed = (a, edge_ptr, edges) if which == "nodes" else (node_ptr, a, edges)
        raw = Raw(torch_cuda, packed)
        assert raw.call() == 0
        info, _, _, status = raw.outputs()
        assert status[1] == 7 and (info[1] == SENTINEL).all(), which
    raw = Raw(torch_cuda, (node_ptr, edge_ptr, edges))
    raw.N -= 1                                                                 # node_ptr[-1] passes the total handed in
    assert raw.call() == 0
    info, new_id, out_edges, status = raw.outputs()
    assert status.tolist() == [0, 0, 7] and (info[2] == SENTINEL).all() and (new_id[8:] == SENTINEL).all()
    assert info[0].tolist() == [2, 1, 3, 2] and info[1].tolist() == [2, 1, 2, 1]


def test_invalid_arguments_launch_nothing(torch_cuda):
    packed = gc.pack([gc.FIVE, dict(gc.cases())["n129"]])
    raw = Raw(torch_cuda, packed)
    for kw in (dict(node_ptr=True), dict(edge_ptr=True), dict(edges=True), dict(info=True), dict(new_id=True), dict(out_edges=True), dict(status=True),
               dict(work=True), dict(work_bytes=raw.need - 1), dict(work_off=8)):
        assert raw.call(**kw) == 1, kw
    for out in raw.outputs():
        assert (out == (SENTINEL & 0xFF if out.dtype == np.uint8 else SENTINEL)).all()
    assert raw.call() == 0
    _check(raw.outputs(), packed, [gc.restate(*gc.FIVE), gc.references()["n129"]], sentinel=SENTINEL)


# ---- batch independence ---------------------------------------------------------------------------------------------------------------------
def test_many_small_graphs_equal_their_solo_calls(torch_cuda):
    """20 000 graphs of at most 16 nodes (more than the grid holds wavefronts: every one draws several tickets) and three WIDE ones:
    the batch equals every graph's solo call written into the same slots, a second run, and a run in a workspace four times larger."""
    graphs, packed = gc.many_small_batch()
    a = Raw(torch_cuda, packed)
    assert a.call() == 0
    first = a.outputs()
    assert not first[3].any()
    assert a.call() == 0
    again = a.outputs()
    b = Raw(torch_cuda, packed, work_factor=4)
    b.work.fill_(0xA5)
    assert b.call() == 0
    large = b.outputs()
    s = Raw(torch_cuda, packed)
    for g in range(len(graphs)):
        assert s.solo(g) == 0
    solo = s.outputs()
    for x, y, z, w in zip(first, again, large, solo):
        assert np.array_equal(x, y) and np.array_equal(x, z) and np.array_equal(x, w)
    for g in (0, 137, 5000, 9999, 19990, 19999):                             # and a few of them against the restatement
        r = gc.restate(*graphs[g])
        assert first[0][g].tolist() == [r["k"], r["m"], r["c"], r["s"]], g
        assert np.array_equal(first[1][packed[0][g]:packed[0][g + 1]], r["new_id"])


# ---- the packed route -------------------------------------------------------------------------------------------------------------------
def _same_tuples(got, ref, what):
    assert len(got) == len(ref), what
    for i, (a, b) in enumerate(zip(got, ref)):
        assert len(a) == len(b), (what, i)
        if len(b) == 2:
            assert a == (None, None) and b == (None, None), (what, i)
            continue
        for j in (0, 1, 2, 5, 6):                                             # d0, d1, the three images
            assert np.array_equal(np.asarray(a[j]), np.asarray(b[j])), (what, i, j)
        assert a[3] == b[3] and a[4].dtype == b[4].dtype and np.array_equal(a[4].numpy(), b[4].numpy()), (what, i)
        assert a[7:] == b[7:]


@pytest.fixture(scope="module")
def route(torch_cuda):
    from tlc_gnn_amd.Knowledge_Distillation import data_utils_GC as kd
    graphs = gc.route_graphs()
    comps = [kd.largest_component(*g) for g in graphs]
    assert any(n > 64 for n, _ in graphs) and any(len(e) == 0 for _, e in graphs) and any(k < n and len(ce) for (n, _), (k, ce) in zip(graphs, comps))
    return graphs, comps, kd.pack_dataset(graphs)


@pytest.mark.parametrize("kw", [dict(filt="degree"), dict(filt="centrality"), dict(filt="clustering"), dict(filt="hks", hks_time=0.1),
                                dict(filt="hks", hks_time=10)], ids=lambda kw: "%s%s" % (kw["filt"], kw.get("hks_time", "")))
def test_ground_truth_packed_largest(route, kw):
    from tlc_gnn_amd.Knowledge_Distillation import data_utils_GC as kd
    graphs, comps, packed = route
    gt = kd.ground_truth_packed(*packed, component="largest", **kw)
    ref = kd.compute_persistence_image_batch(comps, struct_backend="device", hks_backend="device", **kw)
    got = gt.tuples()
    _same_tuples(got, ref, kw)
    assert sum(len(r) > 2 for r in ref) > 200 and sum(len(r) == 2 for r in ref) > 20
    if kw["filt"] != "degree":
        return
    # the packed tensors themselves, against the tuples
    ok = gt.ok.cpu().numpy()
    assert ok.tolist() == [len(r) > 2 for r in ref]
    h = {k: getattr(gt, k).cpu().numpy() for k in gt.FIELDS}
    for i, gi in enumerate(np.flatnonzero(ok)):
        t = ref[gi]
        assert np.array_equal(h["d0"][h["o0"][i]:h["o0"][i + 1]], t[0]) and np.array_equal(h["d1"][h["o1"][i]:h["o1"][i + 1]], t[1])
        assert np.array_equal(h["f"][h["node_ptr"][i]:h["node_ptr"][i + 1]], np.asarray(t[3]))
        assert np.array_equal(h["edges"][h["edge_ptr"][i]:h["edge_ptr"][i + 1]], comps[gi][1])
        r = gc.restate(*graphs[gi])
        assert np.array_equal(h["old_id"][h["node_ptr"][i]:h["node_ptr"][i + 1]], np.flatnonzero(r["new_id"] >= 0))
    assert not h["img"][~ok].any() and not h["PI0"][~ok].any() and not h["PI1"][~ok].any()
    # `filtrations`: values over the ORIGINAL nodes, gathered through the kept old ids
    import torch
    vals = torch.rand(int(packed[0][-1]), dtype=torch.float64, generator=torch.Generator().manual_seed(3)).cuda()
    gtf = kd.ground_truth_packed(*packed, filtrations=vals)
    node_ptr = packed[0].cpu().numpy()
    fs = [vals.cpu().numpy()[node_ptr[gi]:node_ptr[gi + 1]][gc.restate(*graphs[gi])["new_id"] >= 0] for gi in range(len(graphs))]
    _same_tuples(gtf.tuples(), kd.compute_persistence_image_batch(comps, filtrations=fs), "filtrations")


def test_ground_truth_packed_whole(route):
    from tlc_gnn_amd.Knowledge_Distillation import data_utils_GC as kd
    graphs, _, packed = route
    simple = [gc.dedup(*g) for g in graphs]
    ref = kd.compute_persistence_image_batch(simple, filt="degree", struct_backend="device")
    _same_tuples(kd.ground_truth_packed(*packed, filt="degree", component="whole").tuples(), ref, "whole")
    assert sum(len(r) == 2 for r in ref) > 60 and sum(len(r) > 2 for r in ref) > 100


def test_ground_truth_packed_names_the_refused_graph(torch_cuda):
    from tlc_gnn_amd.Knowledge_Distillation import data_utils_GC as kd
    packed = kd.pack_dataset([gc.FIVE, gc.FIVE, (4, np.array([[0, 4]])), (4, np.array([[9, 1]]))])
    with pytest.raises(RuntimeError, match="graph 2"):
        kd.ground_truth_packed(*packed)
    gt = kd.ground_truth_packed(*kd.pack_dataset([(3, gc.E0), (1, gc.E0)]))                  # nothing has a ground truth
    assert gt.tuples() == [(None, None)] * 2 and gt.img.shape == (2, 25) and not gt.img.any()


def test_golden_through_the_packed_route(torch_cuda):
    """The graphs of G4b kd_gc.npz, handed over raw (both orientations), reproduce the reference's filtration (bit for bit), diagrams
    (as multisets) and images (1e-9 relative to max(1, |ref|)): the bounds of tests/test_gpu_pdgnn.py for this golden."""
    from tlc_gnn_amd.Knowledge_Distillation import data_utils_GC as kd
    d = np.load(os.path.join(G, "kd_gc.npz"))
    graphs = []
    for g in range(len(d["n"])):
        e = d["edges"][d["e_offs"][g]:d["e_offs"][g + 1]].astype(np.int64)
        graphs.append((int(d["n"][g]), np.concatenate([e, e[:, ::-1]])))
    for component in kd.COMPONENTS:
        res = kd.ground_truth_packed(*kd.pack_dataset(graphs), filt="degree", component=component).tuples()
        for g, r in enumerate(res):
            d0, d1, img, fv, ei, pi0, pi1, _, _ = r
            assert np.array_equal(np.array(fv), d["f"][d["f_offs"][g]:d["f_offs"][g + 1]])
            assert same_multiset(d0, d["ord0"][d["ord0_offs"][g]:d["ord0_offs"][g + 1]])
            assert same_multiset(d1, d["ext1"][d["ext1_offs"][g]:d["ext1_offs"][g + 1]])
            for got, ref in ((img, d["pi"][g]), (pi0, d["pi0"][g]), (pi1, d["pi1"][g])):
                assert np.abs(got - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max())


class _Item:
    def __init__(self, n, e):
        import torch
        self.num_nodes, self.edge_index = n, torch.from_numpy(np.ascontiguousarray(np.asarray(e, dtype=np.int64).T))


def test_call_packed_leaves_the_store_of_call(torch_cuda, tmp_path):
    """12 graphs, tuples and PyG-like items mixed, one of them the case of test_call_takes_the_largest_component in small: a component
    that is a strict subset, under a random relabelling, with both directions and a self loop."""
    import pickle
    from tlc_gnn_amd.Knowledge_Distillation import data_utils_GC as kd
    graphs = gc.route_graphs(seed=5, n_graphs=11)
    rs = np.random.RandomState(31)
    perm = rs.permutation(400)
    tree = lambda n, off: np.stack([(rs.random_sample(n - 1) * np.arange(1, n)).astype(np.int64), np.arange(1, n)], 1) + off
    E = perm[np.concatenate([tree(300, 0), tree(50, 300)])]
    graphs.insert(4, (400, np.concatenate([E, E[:, ::-1], [[7, 7]]])))
    data = [_Item(*g) if i % 2 else g for i, g in enumerate(graphs)]
    ref, got = {}, {}
    assert kd.call(data, "synthetic", filt="degree", gn=12, struct_backend="device", store=ref) == (0, 0)
    assert kd.call_packed(data, "synthetic", filt="degree", gn=12, store=got, save_dir=str(tmp_path)) == (0, 0)
    assert sorted(got) == sorted(ref) == list(range(12)) and len(got[4][3]) == 300
    _same_tuples([got[i] for i in range(12)], [ref[i] for i in range(12)], "call")
    with open(tmp_path / "synthetic_degree_total_test.pkl", "rb") as fh:
        _same_tuples(list(pickle.load(fh).values()), [ref[i] for i in range(12)], "pickle")
    for kw in (dict(hks_large="gpu"), dict(pd_large="no")):
        with pytest.raises(ValueError):
            kd.call_packed(data, "synthetic", gn=1, **kw)


def test_evaluate_packed_equals_evaluate_batch(route):
    import torch
    from tlc_gnn_amd.Knowledge_Distillation import data_utils_GC as kd
    from tlc_gnn_amd.Knowledge_Distillation.Teacher_model import Teacher_Model
    _, _, packed = route
    torch.manual_seed(5)
    model = Teacher_Model(type='GAT').cuda().eval()
    gt = kd.ground_truth_packed(*packed, filt="degree")
    img, kept = kd.evaluate_packed(model, gt)
    ref_img, ref_kept = kd.evaluate_batch(model, gt.tuples())
    assert kept == ref_kept and len(kept) > 200 and torch.equal(img, ref_img)


def test_pd_large_device_inside_a_packed_batch(torch_cuda):
    """One 5 000-node graph among small ones: with pd_large='device' its diagrams come from tlc_pd_wide on both routes."""
    from tlc_gnn_amd.Knowledge_Distillation import data_utils_GC as kd
    rs = np.random.RandomState(9)
    n = 5000
    big = np.concatenate([np.stack([(rs.random_sample(n - 1) * np.arange(1, n)).astype(np.int64), np.arange(1, n)], 1), rs.randint(0, n, size=(3000, 2))])
    graphs = gc.route_graphs(seed=6, n_graphs=8)
    graphs.insert(3, (n, gc.raw(rs.permutation(n)[big], 10, loops=5, n=n)))
    comps = [kd.largest_component(*g) for g in graphs]
    assert comps[3][0] == n
    got = kd.ground_truth_packed(*kd.pack_dataset(graphs), filt="degree", pd_large="device").tuples()
    _same_tuples(got, kd.compute_persistence_image_batch(comps, filt="degree", struct_backend="device", pd_large="device"), "pd_large")
    assert len(got[3]) == 9 and len(got[3][3]) == n

"""GPU: the degree / centrality / clustering filtrations on the device (tlc_struct_batch, csrc/struct_filt.hip; struct_backend='device' of
the three Knowledge_Distillation drop-ins) against the host route (`data_utils_LP.structural_filtration`, itself pinned bit for bit to
the reference by G4d kd_struct.npz and to closed forms by tests/test_cpu_struct_host.py) and against the reference's goldens.

Every comparison of values is np.array_equal: the arithmetic is integer counting followed by one or two fp64 roundings."""
import ctypes as C
import os

import numpy as np
import pytest

import struct_cases as sc
from helpers import ragged_slice

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BOUNDARIES = (64, 256, 1024, 65536)          # TLC_STRUCT_WAVE_NMAX, _LDS_SMALL_NMAX, _LDS_NMAX (the LDS cap), _BITMAP_BITS (the window)


def _cuda(packed):
    import torch
    return tuple(torch.from_numpy(a).cuda() for a in packed)


def _run(packed, kinds, **kw):
    from tlc_gnn_amd import engine
    f, st = engine.struct_batch(*_cuda(packed), kinds, **kw)
    return f.cpu().numpy(), st.cpu().numpy()


def test_boundaries_are_the_header_constants():
    from tlc_gnn_amd import _lib
    assert BOUNDARIES == (_lib.STRUCT_WAVE_NMAX, _lib.STRUCT_LDS_SMALL_NMAX, _lib.STRUCT_LDS_NMAX, _lib.STRUCT_BITMAP_BITS)


@pytest.mark.parametrize("N", BOUNDARIES)
def test_tier_edges_against_the_host_route(N):
    """Graphs of N - 1, N, N + 1 nodes at every tier boundary N (64 / 65 and the LDS cap 1024 / 1025 among them) -- G(n, p), K_n or a
    planted clique, a star, a complete bipartite graph, two components with isolated nodes -- in one batch: the three kinds one by
    one and all three in one call, bit-equal to the host route; the planted clique's members carry the graph's maximum."""
    cases, packed, ref = sc.tier_edge_batch(N)
    all3, st = _run(packed, sc.KINDS)
    assert all3.shape == (3, packed[0][-1]) and not st.any(), st
    for r, kind in enumerate(sc.KINDS):
        one, st = _run(packed, kind)
        assert one.shape == (1, packed[0][-1]) and not st.any()
        for k, c in enumerate(cases):
            a, b = packed[0][k], packed[0][k + 1]
            assert np.array_equal(one[0, a:b], ref[kind][a:b]), (c[0], kind)
        assert np.array_equal(one[0], ref[kind]) and np.array_equal(all3[r], one[0]), kind
    two, _ = _run(packed, ["clustering", "degree"])                      # rows in the order of the bits, whatever order was asked for
    assert np.array_equal(two[0], ref["degree"]) and np.array_equal(two[1], ref["clustering"])
    for k, c in enumerate(cases):
        a = packed[0][k]
        if len(c) == 3:                                                   # planted clique of k members: t = (k - 1)(k - 2) = d (d - 1)
            assert np.array_equal(all3[2, a + c[2]], np.full(len(c[2]), 1.0 / (1.0 + 1e-10))), c[0]
        if c[0].startswith("star"):
            n = c[1][0]
            assert all3[0, a] == (n - 1.0) / ((n - 1.0) + 1e-10) and not all3[2, a:a + n].any(), c[0]
        if c[0].startswith("K") and "," in c[0]:
            assert not all3[2, a:a + c[1][0]].any(), c[0]


def test_smallest_graphs_and_an_empty_one_between_two_others():
    """n = 1, n = 2, nodes without an edge, the closed forms of the CPU file, and n = 0 between two others (TLC_ST_OK, nothing written:
    its neighbours' slices meet)."""
    empty = np.zeros((0, 2), dtype=np.int64)
    closed = sc.closed_form_cases()
    graphs = [(1, empty), (2, np.array([[0, 1]])), (2, empty), sc.complete(5), (0, empty), sc.star(7), (6, empty)] + [g for _, g, _ in closed]
    packed = sc.pack(graphs)
    f, st = _run(packed, sc.KINDS)
    assert not st.any() and not np.isnan(f).any()
    for r, kind in enumerate(sc.KINDS):
        assert np.array_equal(f[r], sc.host(kind, packed)), kind
        for k, (name, g, raw) in enumerate(closed):
            a, b = packed[0][7 + k], packed[0][8 + k]
            assert np.array_equal(f[r, a:b], sc.normalised(raw[kind])), (name, kind)
    raw, st = _run(packed, sc.KINDS, normalise=False)
    assert raw[:, 0].tolist() == [0.0, 1.0, 0.0]                          # the one-node graph before the normalisation
    assert raw[:, 1:3].tolist() == [[1.0, 1.0], [1.0, 1.0], [0.0, 0.0]]   # n = 2 with its edge
    a = packed[0][3]
    assert raw[:, a:a + 5].tolist() == [[4.0] * 5, [1.0] * 5, [1.0] * 5]  # K5
    # only an empty batch and a batch of empty graphs
    f0, st0 = _run(sc.pack([(0, empty), (0, empty)]), "degree")
    assert f0.shape == (1, 0) and st0.tolist() == [0, 0]


def test_unnormalised_values_divide_to_the_normalised_ones():
    import torch
    from tlc_gnn_amd import engine
    _, packed, ref = sc.tier_edge_batch(256)
    t = _cuda(packed)
    raw, _ = engine.struct_batch(*t, sc.KINDS, normalise=False)
    f, _ = engine.struct_batch(*t, sc.KINDS)
    for k in range(len(packed[0]) - 1):
        sl = raw[:, packed[0][k]:packed[0][k + 1]]
        assert torch.equal(sl / (sl.max(dim=1, keepdim=True).values + 1e-10), f[:, packed[0][k]:packed[0][k + 1]]), k
    assert np.array_equal(raw[0].cpu().numpy(), np.bincount(
        (packed[2].astype(np.int64) + np.repeat(packed[0][:-1], np.diff(packed[1]))[:, None]).reshape(-1), minlength=packed[0][-1]).astype(np.float64))


def test_a_batch_larger_than_every_grid():
    """20 000 random graphs of 1 .. 39 nodes with a few larger ones sprinkled in: every wavefront / workgroup takes several.  The
    whole batch at once against the host route; a graph alone equals the same graph mid-batch; two runs are bit-equal."""
    graphs, packed, ref = sc.many_small_batch()
    assert len(graphs) == 20000
    f1, st1 = _run(packed, sc.KINDS)
    f2, st2 = _run(packed, sc.KINDS)
    assert not st1.any() and not st2.any()
    assert np.array_equal(f1, f2)
    for r, kind in enumerate(sc.KINDS):
        assert np.array_equal(f1[r], ref[kind]), kind
    for k in (0, 137, 4001, 7777, 9999, 12345, 15000, 19990, 19999):
        alone, st = _run(sc.pack([graphs[k]]), sc.KINDS)
        assert not st.any() and np.array_equal(alone, f1[:, packed[0][k]:packed[0][k + 1]]), k


# ---- the reference's goldens ------------------------------------------------------------------------------------------------------------
NAMES = ("degree", "centrality", "clustering", "degree")                 # kd_struct.npz: kind 0..2 node-centred, 3 edge-centred


def test_vicinity_batches_reproduce_the_reference_goldens():
    """Every case of kd_struct.npz, one batched call per (kind, hop) with struct_backend='device', both branches (exact offsets;
    node_cap / edge_cap): ids and f bit for bit, f a CUDA float64 tensor; everything else equal to the host backend's dict."""
    import torch
    from tlc_gnn_amd.Knowledge_Distillation import data_utils_NC as kd_nc, data_utils_LP as kd_lp
    d, g5 = np.load(os.path.join(G, "kd_struct.npz")), np.load(os.path.join(G, "e2e.npz"))
    edges = g5["edges"]
    vic_n, vic_l = kd_nc.NodeVicinities(edges, None), kd_lp.Vicinities(edges, None)
    done = 0
    for kind in range(4):
        for hop in (1, 2):
            sel = np.nonzero((d["kind"] == kind) & (d["hop"] == hop))[0]
            if not len(sel):
                continue
            vic, query = (vic_n, d["u"][sel]) if kind < 3 else (vic_l, np.stack([d["u"][sel], d["v"][sel]], 1))
            host = vic.batch(query, hop, filt=NAMES[kind])
            caps = dict(node_cap=int((host["node_ptr"][1:] - host["node_ptr"][:-1]).max()) + 1,
                        edge_cap=int((host["edge_ptr"][1:] - host["edge_ptr"][:-1]).max()) + 1)
            for kw in ({}, caps):
                b = vic.batch(query, hop, filt=NAMES[kind], struct_backend='device', **kw)
                assert b["f"].is_cuda and b["f"].dtype == torch.float64
                for key in ("node_ptr", "edge_ptr", "ids", "edges", "status", "f"):
                    assert torch.equal(host[key], b[key]), (kind, hop, key)
                node_ptr, ids, f = b["node_ptr"].cpu().numpy(), b["ids"].cpu().numpy(), b["f"].cpu().numpy()
                for k, gi in enumerate(sel):
                    assert np.array_equal(ids[node_ptr[k]:node_ptr[k + 1]], ragged_slice(d["ids"], d["offs"], gi)), (kind, hop, k)
                    assert np.array_equal(f[node_ptr[k]:node_ptr[k + 1]], ragged_slice(d["f"], d["offs"], gi)), (kind, hop, k)
            done += len(sel)
    assert done == len(d["kind"]) == 179
    # no effect on the other filtrations
    for filt in ('ricci', 'hks'):
        a, b = vic_n.batch(d["u"][:8], 1, filt=filt), vic_n.batch(d["u"][:8], 1, filt=filt, struct_backend='device')
        assert torch.equal(a["f"], b["f"]), filt


@pytest.mark.parametrize("kind", range(4))
def test_single_calls_equal_the_host_backend_and_the_goldens(kind):
    """compute_persistence_image(..., struct_backend='device', mode='PI') for every case of kd_struct.npz: the host backend's tuple,
    element for element, f bit-equal to the golden."""
    from tlc_gnn_amd.Knowledge_Distillation import data_utils_NC as kd_nc, data_utils_LP as kd_lp
    d, g5 = np.load(os.path.join(G, "kd_struct.npz")), np.load(os.path.join(G, "e2e.npz"))
    edges = g5["edges"]
    sel = np.nonzero(d["kind"] == kind)[0]
    assert len(sel) >= 8
    for gi in sel:
        hop, u, v = int(d["hop"][gi]), int(d["u"][gi]), int(d["v"][gi])
        if kind < 3:
            call = lambda **kw: kd_nc.compute_persistence_image(edges, u, filt=NAMES[kind], hop=hop, mode='PI', **kw)
        else:
            call = lambda **kw: kd_lp.compute_persistence_image(edges, u, v, filt='degree', hop=hop, mode='PI', **kw)
        dev, host = call(struct_backend='device'), call()
        assert len(dev) == len(host) == 9
        assert np.array_equal(np.array(dev[3]), ragged_slice(d["f"], d["offs"], gi)), gi
        for a, b in zip(dev, host):
            assert np.array_equal(np.asarray(a), np.asarray(b)), gi
    if kind < 3:
        fv, ei = kd_nc.compute_persistence_image(edges, int(d["u"][sel[0]]), filt=NAMES[kind], hop=int(d["hop"][sel[0]]), mode='filtration',
                                                 struct_backend='device')
        assert np.array_equal(np.array(fv), ragged_slice(d["f"], d["offs"], sel[0]))


def test_graph_classification_batch_on_molecule_graphs():
    """About 200 HIV-shaped graphs through compute_persistence_image_batch: 'degree' with struct_backend='device' equals the host
    backend element for element; 'centrality' and 'clustering', which the host backend refuses, equal `filtrations=` precomputed by
    the host function."""
    from tlc_gnn_amd import synth
    from tlc_gnn_amd.Knowledge_Distillation import data_utils_GC as kd_gc
    edges, _, node_offs, edge_offs = synth.hiv_shaped_molecules(200)
    graphs = [(int(node_offs[k + 1] - node_offs[k]), edges[edge_offs[k]:edge_offs[k + 1]].astype(np.int64)) for k in range(200)]

    def same(xs, ys):
        assert len(xs) == len(ys) == 200
        n = 0
        for x, y in zip(xs, ys):
            assert len(x) == len(y)
            for a, b in zip(x, y):
                assert (a is None and b is None) or np.array_equal(np.asarray(a), np.asarray(b))
            n += len(x) == 9
        assert n >= 100
    same(kd_gc.compute_persistence_image_batch(graphs, filt='degree', struct_backend='device'), kd_gc.compute_persistence_image_batch(graphs, filt='degree'))
    for filt in ('centrality', 'clustering'):
        pre = [sc.host(filt, sc.pack([g])) for g in graphs]
        same(kd_gc.compute_persistence_image_batch(graphs, filt=filt, struct_backend='device'),
             kd_gc.compute_persistence_image_batch(graphs, filt=filt, filtrations=pre))
    one = kd_gc.compute_persistence_image(graphs[0], filt='degree', mode='PI', struct_backend='device')
    for a, b in zip(one, kd_gc.compute_persistence_image(graphs[0], filt='degree', mode='PI')):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    fv, _ = kd_gc.compute_persistence_image(graphs[0], filt='degree', mode='filtration', struct_backend='device')
    assert fv == kd_gc.compute_persistence_image(graphs[0], filt='degree', mode='filtration')[0]


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def _bad_edge_cases(n):
    """a good graph of n nodes spoilt in one way each"""
    _, e = sc.gnp(n, min(0.5, 6.0 / n), 900 + n)
    a, b = (int(x) for x in e[len(e) // 2])
    add = lambda rows: (n, np.concatenate([e, np.array(rows, dtype=np.int64).reshape(-1, 2)]))
    return [("id n", add([[0, n]])), ("id -1", add([[-1, 1]])), ("self loop", add([[n - 1, n - 1]])),
            ("(a,b)(a,b)", add([[a, b]])), ("(a,b)(b,a)", add([[b, a]]))]


@pytest.mark.parametrize("n", [40, 200, 700, 1500, 70000])
def test_bad_edges_are_a_status_in_each_tier(n):
    """An id of n, an id of -1, a self loop, (a, b)(a, b) and (a, b)(b, a) in a graph of each tier (and of two bitmap windows), each
    between good neighbours: TLC_ST_BAD_INPUT, its NaN slice untouched, the neighbours exact."""
    from tlc_gnn_amd import _lib
    good = sc.gnp(n, min(0.5, 6.0 / n), 900 + n)
    small = sc.gnp(12, 0.4, 3)
    bads = _bad_edge_cases(n)
    graphs = [small]
    for _, g in bads:
        graphs += [g, good, small]
    packed = sc.pack(graphs)
    f, st = _run(packed, sc.KINDS)
    assert st.tolist() == [0] + [_lib.ST_BAD_INPUT, 0, 0] * len(bads)
    ref_good, ref_small = [sc.host(k, sc.pack([good])) for k in sc.KINDS], [sc.host(k, sc.pack([small])) for k in sc.KINDS]
    for k in range(len(graphs)):
        sl = f[:, packed[0][k]:packed[0][k + 1]]
        if st[k]:
            assert np.isnan(sl).all(), bads[(k - 1) // 3][0]
        else:
            assert np.array_equal(sl, np.stack(ref_small if graphs[k] is small else ref_good)), k


def test_bad_offsets_are_a_status():
    """Offsets out of order or beyond the totals: TLC_ST_BAD_INPUT for the graphs they touch, nothing of them read or written."""
    import torch
    from tlc_gnn_amd import engine, _lib
    g = sc.gnp(10, 0.4, 1)
    packed = sc.pack([g, g, g, g])
    bad = _lib.ST_BAD_INPUT
    ref = sc.host("clustering", sc.pack([g]))
    node_ptr = packed[0].copy()
    node_ptr[2:4] = 25, 20                                                # graph 2 ends before it starts (graphs 1 and 3 then overlap)
    f, st = engine.struct_batch(torch.from_numpy(node_ptr).cuda(), *_cuda(packed[1:]), "clustering", total_nodes=40)
    assert st.cpu().tolist() == [0, 0, bad, 0]
    assert np.array_equal(f[0, :10].cpu().numpy(), ref) and np.array_equal(f[0, 25:30].cpu().numpy(), ref[5:])
    edge_ptr = packed[1].copy()
    edge_ptr[4] += 7                                                      # beyond total_edges
    f, st = engine.struct_batch(torch.from_numpy(packed[0]).cuda(), torch.from_numpy(edge_ptr).cuda(), torch.from_numpy(packed[2]).cuda(), "clustering")
    assert st.cpu().tolist() == [0, 0, 0, bad] and bool(torch.isnan(f[0, 30:]).all()) and np.array_equal(f[0, :10].cpu().numpy(), ref)
    f, st = engine.struct_batch(*_cuda(packed), "clustering", total_nodes=35)   # node_ptr[-1] = 40 beyond the total handed in
    assert st.cpu().tolist() == [0, 0, 0, bad] and f.shape == (1, 35)
    edge_ptr = packed[1].copy()
    edge_ptr[1] = -1
    _, st = engine.struct_batch(torch.from_numpy(packed[0]).cuda(), torch.from_numpy(edge_ptr).cuda(), torch.from_numpy(packed[2]).cuda(), "degree")
    assert st.cpu().tolist()[:2] == [bad, bad]


def test_python_routes_raise_runtime_error():
    from tlc_gnn_amd.Knowledge_Distillation import data_utils_GC as kd_gc, data_utils_LP as kd_lp
    tri = np.array([[0, 1], [1, 2], [0, 2]])
    both = np.concatenate([tri, tri[:, ::-1]])
    for filt in sc.KINDS:
        with pytest.raises(RuntimeError):
            kd_gc.compute_persistence_image_batch([(3, tri), (3, both)], filt=filt, struct_backend='device')
    with pytest.raises(RuntimeError):
        kd_gc.compute_persistence_image((3, np.concatenate([tri, tri[:1]])), filt='degree', mode='filtration', struct_backend='device')
    with pytest.raises(RuntimeError):
        kd_lp.struct_filtration_device("degree", *_cuda(sc.pack([(3, tri), (3, np.array([[0, 1], [1, 1]]))])), 6)
    assert len(kd_gc.compute_persistence_image_batch([(3, both)], filt='degree')[0]) == 9        # the host backend takes it, as before


def test_c_abi_misuse_is_a_return_code():
    import torch
    from tlc_gnn_amd import _lib
    L = _lib.lib()
    need = C.c_int64(-1)
    assert L.tlc_struct_batch_work_bytes(4, 100, 200, 0, C.byref(need)) == 1             # kinds == 0
    assert L.tlc_struct_batch_work_bytes(4, 100, 200, 0x8, C.byref(need)) == 1           # unknown bit
    assert L.tlc_struct_batch_work_bytes(4, 100, 200, 0x7, None) == 1
    assert L.tlc_struct_batch_work_bytes(4, 100, 200, 0x7, C.byref(need)) == 0 and need.value >= 256 + 64
    small = need.value
    assert L.tlc_struct_batch_work_bytes(4, 5000, 200, 0x7, C.byref(need)) == 0 and need.value > small     # room for the CSR tier
    node_ptr, edge_ptr, edges = _cuda(sc.pack([(3, np.array([(0, 1), (1, 2)]))]))
    out = torch.full((3, 3), -1.0, dtype=torch.float64, device="cuda")
    st = torch.zeros(1, dtype=torch.uint8, device="cuda")
    work = torch.empty(small + 16, dtype=torch.uint8, device="cuda")
    assert work.data_ptr() % 16 == 0
    P, s = _lib.ptr, _lib.stream_ptr()
    call = lambda np_=P(node_ptr), ep=P(edge_ptr), ed=P(edges), B=1, kinds=0x7, flags=0x100, o=P(out), stp=P(st), w=P(work), wb=small: \
        L.tlc_struct_batch(np_, ep, ed, B, 3, 2, kinds, flags, o, stp, w, wb, s)
    assert call(kinds=0) == 1 and call(kinds=0x10) == 1 and call(kinds=0x107) == 1
    assert call(flags=0x1) == 1 and call(flags=0x300) == 1
    assert call(wb=small - 1) == 1 and call(wb=16) == 1
    assert call(w=C.c_void_p(work.data_ptr() + 8)) == 1                                   # misaligned
    assert call(np_=None) == 1 and call(ep=None) == 1 and call(ed=None) == 1 and call(o=None) == 1 and call(stp=None) == 1 and call(w=None) == 1
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [[-1.0] * 3] * 3                                         # nothing ran
    assert call(B=0) == 0 and call(B=0, np_=None, w=None, wb=0) == 0                      # n_graphs == 0: TLC_OK
    assert call() == 0
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0] and out[0].cpu().tolist() == [1.0 / (2.0 + 1e-10), 2.0 / (2.0 + 1e-10), 1.0 / (2.0 + 1e-10)]

"""GPU: the heat-kernel-signature filtration on the device (tlc_hks_batch, csrc/hks.hip; hks_backend='device' of the three
Knowledge_Distillation drop-ins) against the reference's goldens (G4e kd_hks.npz) and against the host route
(`data_utils_LP.hks_signature`: scipy's eigh, itself pinned bit for bit to the reference by G4e).

Bounds: 1e-11 absolute on the normalised values, 1e-9 on diagram values, 1e-7 on images -- the bounds the host route's own tests
use for "same quantity, other rounding" (test_oracle_golden.py::test_kd_hks_g4e, test_gpu_variants.py::
test_kd_hks_filtration_golden_g4e).  A backward-stable eigensolver moves hks by at most t * p(n) * u * ||L||, ||L|| <= 2: some
1e-13 at t = 10, n = 256, for LAPACK and for the Jacobi kernel alike."""
import ctypes as C
import os

import numpy as np
import pytest

from helpers import ragged_slice

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TIMES = (0.1, 10.0)


def _close_multiset(a, b, tol):
    """two point sets equal as multisets up to `tol`: same count, and the lexicographically sorted arrays agree within tol after
    rounding both to a grid of 10 x tol (near-equal points may swap places in the sort, rounding puts them on the same key)
    -- the helper of test_oracle_golden.py"""
    a, b = np.asarray(a, dtype=np.float64).reshape(-1, 2), np.asarray(b, dtype=np.float64).reshape(-1, 2)
    if len(a) != len(b):
        return False
    if not len(a):
        return True
    key = lambda x: np.lexsort((np.round(x[:, 1] / (10 * tol)), np.round(x[:, 0] / (10 * tol))))
    return bool(np.abs(np.sort(a[:, 0]) - np.sort(b[:, 0])).max() <= tol and np.abs(np.sort(a[:, 1]) - np.sort(b[:, 1])).max() <= tol
                and np.abs(a.sum(0) - b.sum(0)).max() <= tol * len(a))


def _random_connected(n, seed):
    """a random tree plus about 2n extra edges: simple, connected, each edge once (lower id first)"""
    rs = np.random.RandomState(seed)
    es = {(int(rs.randint(i)), i) for i in range(1, n)}
    for _ in range(2 * n if n > 1 else 0):
        a, b = (int(x) for x in rs.randint(n, size=2))
        if a != b:
            es.add((min(a, b), max(a, b)))
    return np.array(sorted(es), dtype=np.int64).reshape(-1, 2)


def _pack(graphs):
    import torch
    node_ptr = np.concatenate([[0], np.cumsum([n for n, _ in graphs])]).astype(np.int64)
    edge_ptr = np.concatenate([[0], np.cumsum([len(e) for _, e in graphs])]).astype(np.int64)
    edges = np.concatenate([np.asarray(e, dtype=np.int64).reshape(-1, 2) for _, e in graphs]).astype(np.int32)
    return torch.from_numpy(node_ptr).cuda(), torch.from_numpy(edge_ptr).cuda(), torch.from_numpy(edges).cuda(), node_ptr


def _host(n, e, t):
    from tlc_gnn_amd.Knowledge_Distillation.data_utils_LP import hks_signature
    v = hks_signature(n, e, t)
    return v / (max(v) + 1e-10)


def test_device_backend_reference_goldens_all_cases_g4e():
    """All 108 cases of kd_hks.npz through the three signatures with hks_backend='device', mode 'PI': values 1e-11, diagram sizes
    equal and diagrams as multisets 1e-9, the three images 1e-7 * max(1, |ref|), every case on the device."""
    from tlc_gnn_amd.Knowledge_Distillation import data_utils_NC as kd_nc, data_utils_LP as kd_lp, data_utils_GC as kd_gc
    d, g5 = np.load(os.path.join(G, "kd_hks.npz")), np.load(os.path.join(G, "e2e.npz"))
    edges = g5["edges"]
    assert len(d["kind"]) == 108
    n_done, worst_f, worst_img = [0, 0, 0], 0.0, 0.0
    for gi in range(len(d["kind"])):
        kind, hop, u, v, t = int(d["kind"][gi]), int(d["hop"][gi]), int(d["u"][gi]), int(d["v"][gi]), float(d["time"][gi])
        ref_f = ragged_slice(d["f"], d["offs"], gi)
        if kind == 2:
            res = kd_gc.compute_persistence_image((int(d["n"][gi]), ragged_slice(d["edges"], d["e_offs"], gi)), filt='hks', hks_time=t,
                                                  mode='PI', hks_backend='device')
        elif kind == 0:
            res = kd_nc.compute_persistence_image(edges, u, filt='hks', hks_time=t, hop=hop, mode='PI', hks_backend='device')
        else:
            res = kd_lp.compute_persistence_image(edges, u, v, filt='hks', hks_time=t, hop=hop, mode='PI', hks_backend='device')
        assert kd_lp.hks_host_fallback == 0, gi
        o0, e1, img, fv, ei, pi0, pi1, _, _ = res
        df = np.abs(np.array(fv) - ref_f).max()
        worst_f = max(worst_f, df)
        print("case %3d kind %d n %3d t %4.1f  |f - ref| %.2e" % (gi, kind, len(ref_f), t, df))
        assert df <= 1e-11, (gi, df)
        ref0, ref1 = ragged_slice(d["ord0"], d["ord0_offs"], gi), ragged_slice(d["ext1"], d["ext1_offs"], gi)
        assert len(o0) == len(ref0) and len(e1) == len(ref1), gi
        assert _close_multiset(o0, ref0, 1e-9), gi
        assert _close_multiset(e1, ref1, 1e-9), gi
        for got, ref in ((img, d["pi"][gi]), (pi0, d["pi0"][gi]), (pi1, d["pi1"][gi])):
            di = np.abs(np.asarray(got) - ref).max()
            worst_img = max(worst_img, di / max(1.0, np.abs(ref).max()))
            assert di <= 1e-7 * max(1.0, np.abs(ref).max()), (gi, kind, di)
        n_done[kind] += 1
    print("worst |f - ref| %.2e, worst image difference %.2e (relative to max(1, |ref|))" % (worst_f, worst_img))
    assert sum(n_done) == 108 and min(n_done) >= 8


def _size_and_spectrum_cases():
    from tlc_gnn_amd import _lib
    sizes = [1, 2, 3, 5, 17, 31, 32, 33, 63, 64, 65, _lib.HKS_LDS_NMAX - 1, _lib.HKS_LDS_NMAX, _lib.HKS_LDS_NMAX + 1, 200, 256, _lib.HKS_NMAX]
    cases = [("random%d" % n, n, _random_connected(n, 1000 + n)) for n in sorted(set(sizes))]
    cases.append(("star K(1,64)", 65, np.array([(0, i) for i in range(1, 65)])))
    cases.append(("cycle C64", 64, np.array([(i, i + 1) for i in range(63)] + [(0, 63)])))
    cases.append(("complete K32", 32, np.array([(i, j) for i in range(32) for j in range(i + 1, 32)])))
    cases.append(("path P2", 2, np.array([(0, 1)])))
    cases.append(("grid 12x12", 144, np.array([(i * 12 + j, i * 12 + j + 1) for i in range(12) for j in range(11)] +
                                              [(i * 12 + j, i * 12 + j + 12) for i in range(11) for j in range(12)])))
    order = np.random.RandomState(7).permutation(len(cases))
    return [cases[i] for i in order]


def test_sizes_tier_boundaries_and_spectra_in_one_batch_against_host():
    """Random connected graphs at n = 1 .. TLC_HKS_NMAX with every tier boundary (32, 64, TLC_HKS_LDS_NMAX = 96) at b - 1, b, b + 1,
    a star, a cycle, a complete graph, a path and a grid (degenerate spectra), times 0.1 and 10, ONE shuffled batch: every status OK
    and 1e-11 of the host route."""
    from tlc_gnn_amd import engine, _lib
    assert _lib.HKS_NMAX >= 256
    cases = _size_and_spectrum_cases()
    node_ptr, edge_ptr, edges, nptr = _pack([(n, e) for _, n, e in cases])
    f, st = engine.hks_batch(node_ptr, edge_ptr, edges, TIMES, normalise=True)
    f, st = f.cpu().numpy(), st.cpu().numpy()
    assert f.shape == (2, nptr[-1])
    assert np.array_equal(st, np.zeros(len(cases), dtype=np.uint8)), st
    worst = 0.0
    for k, (name, n, e) in enumerate(cases):
        for ti, t in enumerate(TIMES):
            diff = np.abs(f[ti, nptr[k]:nptr[k + 1]] - _host(n, e, t)).max()
            print("%-14s n %3d t %4.1f  |device - host| %.2e" % (name, n, t, diff))
            worst = max(worst, diff)
            assert diff <= 1e-11, (name, t, diff)
    print("worst |device - host| %.2e" % worst)


def test_deterministic_and_independent_of_the_batch():
    """The batch of the size test twice: same bits.  Each graph alone: the bits of its slice.  Two times in one call: the bits of two
    single-time calls.  Un-normalised / (max + 1e-10) in torch fp64: the bits of the normalised output."""
    import torch
    from tlc_gnn_amd import engine
    cases = _size_and_spectrum_cases()
    node_ptr, edge_ptr, edges, nptr = _pack([(n, e) for _, n, e in cases])
    f1, st1 = engine.hks_batch(node_ptr, edge_ptr, edges, TIMES)
    f2, st2 = engine.hks_batch(node_ptr, edge_ptr, edges, TIMES)
    assert int(st1.sum()) == 0 and torch.equal(f1, f2) and torch.equal(st1, st2)
    for k, (name, n, e) in enumerate(cases):
        a = _pack([(n, e)])
        alone, st = engine.hks_batch(a[0], a[1], a[2], TIMES)
        assert int(st.sum()) == 0 and torch.equal(alone, f1[:, nptr[k]:nptr[k + 1]]), name
    for ti, t in enumerate(TIMES):
        single, _ = engine.hks_batch(node_ptr, edge_ptr, edges, [t])
        assert torch.equal(single[0], f1[ti]), t
    raw, _ = engine.hks_batch(node_ptr, edge_ptr, edges, TIMES, normalise=False)
    for k in range(len(cases)):
        sl = raw[:, nptr[k]:nptr[k + 1]]
        assert torch.equal(sl / (sl.max(dim=1, keepdim=True).values + 1e-10), f1[:, nptr[k]:nptr[k + 1]]), cases[k][0]


def test_graph_above_the_cap_takes_the_host_route_and_is_counted():
    """One graph of TLC_HKS_NMAX + 1 nodes between two small ones.  C level: status TLC_ST_TOO_LARGE, its slice of the NaN-filled
    output still NaN, the small ones bit-equal to their stand-alone values.  Wrapper: the large one bit-equal to the host route,
    hks_host_fallback == 1."""
    import torch
    from tlc_gnn_amd import engine, _lib
    from tlc_gnn_amd.Knowledge_Distillation import data_utils_LP as kd_lp, data_utils_GC as kd_gc
    big_n = _lib.HKS_NMAX + 1
    graphs = [(20, _random_connected(20, 1)), (big_n, _random_connected(big_n, 2)), (45, _random_connected(45, 3))]
    node_ptr, edge_ptr, edges, nptr = _pack(graphs)
    f, st = engine.hks_batch(node_ptr, edge_ptr, edges, [0.1])
    assert st.cpu().tolist() == [_lib.ST_OK, _lib.ST_TOO_LARGE, _lib.ST_OK]
    assert bool(torch.isnan(f[0, nptr[1]:nptr[2]]).all())
    alone = []
    for k in (0, 2):
        a = _pack([graphs[k]])
        alone.append(engine.hks_batch(a[0], a[1], a[2], [0.1])[0][0])
        assert torch.equal(alone[-1], f[0, nptr[k]:nptr[k + 1]])
    out = kd_lp.hks_filtration_device(node_ptr, edge_ptr, edges, 0.1, int(nptr[-1]))
    assert kd_lp.hks_host_fallback == 1
    assert torch.equal(out[nptr[0]:nptr[1]], alone[0]) and torch.equal(out[nptr[2]:nptr[3]], alone[1])
    assert np.array_equal(out[nptr[1]:nptr[2]].cpu().numpy(), _host(big_n, graphs[1][1], 0.1))
    res = kd_gc.compute_persistence_image_batch(graphs, filt='hks', hks_time=0.1, hks_backend='device')
    assert kd_lp.hks_host_fallback == 1
    assert np.array_equal(np.array(res[1][3]), _host(big_n, graphs[1][1], 0.1))
    assert np.array_equal(np.array(res[0][3]), alone[0].cpu().numpy())
    kd_gc.compute_persistence_image_batch([graphs[0], graphs[2]], filt='hks', hks_time=0.1, hks_backend='device')
    assert kd_lp.hks_host_fallback == 0


def test_bad_edges_are_a_status_not_a_read():
    """An edge id outside 0 .. n-1 (either sign) or a self loop: TLC_ST_BAD_INPUT for that graph, the neighbours untouched."""
    import torch
    from tlc_gnn_amd import engine, _lib
    good = (10, _random_connected(10, 4))
    graphs = [good, (4, np.array([(0, 1), (1, 7)])), good, (4, np.array([(0, 1), (-3, 2)])), (3, np.array([(1, 1)])), good]
    node_ptr, edge_ptr, edges, nptr = _pack(graphs)
    f, st = engine.hks_batch(node_ptr, edge_ptr, edges, [10.0])
    bad = _lib.ST_BAD_INPUT
    assert st.cpu().tolist() == [0, bad, 0, bad, bad, 0]
    for k in (0, 2, 5):
        assert torch.equal(f[0, nptr[k]:nptr[k + 1]], f[0, :10])
    assert bool(torch.isnan(f[0, nptr[1]:nptr[2]]).all()) and bool(torch.isnan(f[0, nptr[3]:nptr[5]]).all())


def test_c_abi_misuse_is_a_return_code():
    import torch
    from tlc_gnn_amd import _lib
    L = _lib.lib()
    need = C.c_int64(-1)
    assert L.tlc_hks_batch_work_bytes(4, 100, 200, 0, C.byref(need)) == 1
    assert L.tlc_hks_batch_work_bytes(4, 100, 200, _lib.HKS_TMAX + 1, C.byref(need)) == 1
    assert L.tlc_hks_batch_work_bytes(4, 100, 200, 2, C.byref(need)) == 0 and need.value > 0
    small = need.value
    # the workspace does not grow with the number of large graphs beyond one slot per CU
    assert L.tlc_hks_batch_work_bytes(100000, 10 ** 8, 10 ** 8, 2, C.byref(need)) == 0
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert need.value <= 16 * 100000 + 512 + cus * 2 * 256 * 257 * 8 and small < need.value
    node_ptr, edge_ptr, edges, _ = _pack([(3, np.array([(0, 1), (1, 2)]))])
    out = torch.zeros((1, 3), dtype=torch.float64, device="cuda")
    st = torch.zeros(1, dtype=torch.uint8, device="cuda")
    work = torch.empty(small, dtype=torch.uint8, device="cuda")
    t = (C.c_double * 1)(0.1)
    rc = L.tlc_hks_batch(_lib.ptr(node_ptr), _lib.ptr(edge_ptr), _lib.ptr(edges), 1, 3, 2, t, 1, 0x1, _lib.ptr(out), _lib.ptr(st),
                         _lib.ptr(work), 16, _lib.stream_ptr())
    assert rc == 1                                                     # workspace too small
    rc = L.tlc_hks_batch(_lib.ptr(node_ptr), _lib.ptr(edge_ptr), _lib.ptr(edges), 1, 3, 2, t, 1, 0x80, _lib.ptr(out), _lib.ptr(st),
                         _lib.ptr(work), small, _lib.stream_ptr())
    assert rc == 1                                                     # unknown flag


@pytest.mark.parametrize("hop", [1, 2])
def test_vicinity_batches_device_backend_equals_host_backend(hop):
    """On the G5 graph: Vicinities.batch / NodeVicinities.batch with hks_backend='device' return what 'host' returns -- offsets, ids,
    edges, status equal, f a CUDA float64 tensor within 1e-11 -- in both branches (exact offsets; node_cap / edge_cap)."""
    import torch
    from tlc_gnn_amd.Knowledge_Distillation import data_utils_NC as kd_nc, data_utils_LP as kd_lp
    g5 = np.load(os.path.join(G, "e2e.npz"))
    edges = g5["edges"]
    rs = np.random.RandomState(3)
    pairs = edges[rs.choice(len(edges), size=24, replace=False)]
    nodes = rs.choice(np.unique(edges), size=24, replace=False)
    for vic, query in ((kd_lp.Vicinities(edges, None), pairs), (kd_nc.NodeVicinities(edges, None), nodes)):
        sizes = vic.batch(query, hop, filt='degree')
        caps = dict(node_cap=int((sizes["node_ptr"][1:] - sizes["node_ptr"][:-1]).max()) + 1,
                    edge_cap=int((sizes["edge_ptr"][1:] - sizes["edge_ptr"][:-1]).max()) + 1)
        for kw in ({}, caps):
            for t in TIMES:
                host = vic.batch(query, hop, filt='hks', hks_time=t, hks_backend='host', **kw)
                dev = vic.batch(query, hop, filt='hks', hks_time=t, hks_backend='device', **kw)
                assert dev["hks_host_fallback"] == 0 and kd_lp.hks_host_fallback == 0
                for key in ("node_ptr", "edge_ptr", "ids", "edges", "status"):
                    assert torch.equal(host[key], dev[key]), key
                assert dev["f"].is_cuda and dev["f"].dtype == torch.float64 and dev["f"].shape == host["f"].shape
                assert dev["f"].numel() > 0 and float((dev["f"] - host["f"]).abs().max()) <= 1e-11
                # another filtration: the keyword is accepted and has no effect
                a = vic.batch(query, hop, filt='degree', hks_backend='device', **kw)
                assert torch.equal(a["f"], vic.batch(query, hop, filt='degree', **kw)["f"])


def test_gc_batch_device_backend_equals_single_calls():
    from tlc_gnn_amd.Knowledge_Distillation import data_utils_GC as kd_gc
    d = np.load(os.path.join(G, "kd_hks.npz"))
    sel = [gi for gi in range(len(d["kind"])) if int(d["kind"][gi]) == 2 and float(d["time"][gi]) == 10.0]
    graphs = [(int(d["n"][gi]), ragged_slice(d["edges"], d["e_offs"], gi)) for gi in sel]
    outs = kd_gc.compute_persistence_image_batch(graphs, filt='hks', hks_time=10.0, hks_backend='device')
    assert len(outs) == len(sel) >= 12
    for g, o in zip(graphs, outs):
        one = kd_gc.compute_persistence_image(g, filt='hks', hks_time=10.0, mode='PI', hks_backend='device')
        for a, b in zip(o[:4] + o[5:7], one[:4] + one[5:7]):
            assert np.array_equal(np.asarray(a), np.asarray(b))
        fv, ei = kd_gc.compute_persistence_image(g, filt='hks', hks_time=10.0, mode='filtration', hks_backend='device')
        assert fv == o[3]

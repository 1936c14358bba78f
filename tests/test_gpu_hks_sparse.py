"""GPU: the sparse heat-kernel-signature tier (tlc_hks_sparse_batch / _dt, csrc/hks_sparse.hip; hks_sparse='device' of the wrappers)
against the numpy restatement of its operation sequence (tests/hks_sparse_cases.py) bit for bit, against itself (`==`: times, batches,
selections, workspaces, runs), against the other tiers and closed forms, and through routing, autograd and the packed route.

Bounds against other tiers and closed forms: 1e-11 (value) and 2e-11 (derivative) absolute, the bounds of tests/test_gpu_hks_large.py
and tests/test_gpu_hks_dt.py; the method sums non-negative terms only, the restatement stays below 2e-14 of eigh on graphs of 900 nodes
(tests/test_cpu_hks_sparse_host.py)."""
import numpy as np
import pytest

import hks_sparse_cases as hc

pytestmark = pytest.mark.gpu
TIMES = (0.0, 1e-9, 0.1, 10.0, 64.0)
EIGHT = (0.0, 1e-9, 0.1, 0.5, 1.0, 3.0, 10.0, 64.0)
NO_EDGES = np.zeros((0, 2), dtype=np.int64)


def _pack(graphs):
    import torch
    node_ptr = np.concatenate([[0], np.cumsum([n for n, _ in graphs])]).astype(np.int64)
    edge_ptr = np.concatenate([[0], np.cumsum([len(e) for _, e in graphs])]).astype(np.int64)
    edges = np.concatenate([np.asarray(e, dtype=np.int64).reshape(-1, 2) for _, e in graphs] + [NO_EDGES]).astype(np.int32).reshape(-1, 2)
    return torch.from_numpy(node_ptr).cuda(), torch.from_numpy(edge_ptr).cuda(), torch.from_numpy(edges).cuda(), node_ptr


def _sparse(graphs, times, sel=None, normalise=False, packed=None, **kw):
    """engine.hks_sparse_batch with the derivative on a packed list of (n, edges) -> numpy (f, df, status), node offsets"""
    from tlc_gnn_amd import engine
    node_ptr, edge_ptr, edges, nptr = _pack(graphs) if packed is None else packed
    sel = list(range(len(graphs))) if sel is None else sel
    kw.setdefault("sel_nodes", [graphs[k][0] for k in sel])
    kw.setdefault("sel_edges", [len(graphs[k][1]) for k in sel])
    f, df, st = engine.hks_sparse_batch(node_ptr, edge_ptr, edges, sel, kw.pop("sel_nodes"), kw.pop("sel_edges"), list(times), normalise=normalise,
                                        dout=True, **kw)
    return f.cpu().numpy(), df.cpu().numpy(), st.cpu().numpy(), nptr


def _bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def _row_lengths():
    """328 nodes with rows of 0, 1, 63, 64, 65 and 129 neighbours: four stars, an edge and an isolated node"""
    return hc.union(hc.star(63), hc.star(64), hc.star(65), hc.star(129), hc.star(1), isolated=1)


def _hub():
    """4 101 nodes: a hub of 4 100 neighbours (65 chunks: a split row) whose leaves also form a path, so no two columns are alike"""
    n, e = hc.star(4100)
    return n, np.concatenate([e, np.array([(i, i + 1) for i in range(1, 4100)])])


EDGE_GRAPHS = [(n, hc.random_connected(n, 100 + n, extra=n)) for n in (1, 2, 63, 64, 65, 128, 129)] + [_row_lengths()]


def test_bits_against_the_restatement_at_panel_and_row_edges():
    """n = 1, 2, 63, 64, 65, 128, 129 and rows of 0, 1, 63, 64, 65, 129 neighbours, one batch, five times in one call: value and
    derivative, raw and normalised, are the restatement's bits; the call without the derivative writes the same values"""
    from tlc_gnn_amd import engine, _lib
    f, df, st, nptr = _sparse(EDGE_GRAPHS, TIMES)
    fn, dfn, stn, _ = _sparse(EDGE_GRAPHS, TIMES, normalise=True)
    assert (st == _lib.ST_OK).all() and (stn == _lib.ST_OK).all()
    for g, (n, e) in enumerate(EDGE_GRAPHS):
        csr = hc.Csr(n, e)
        for k, t in enumerate(TIMES):
            v, d = hc.restate(n, e, t, csr=csr)
            a, b = nptr[g], nptr[g + 1]
            assert _bits(f[k, a:b], v) and _bits(df[k, a:b], d), (n, t)
            nv, nd = hc.normalise(v, d)
            assert _bits(fn[k, a:b], nv) and _bits(dfn[k, a:b], nd), (n, t)
    node_ptr, edge_ptr, edges, _ = _pack(EDGE_GRAPHS)
    sel = list(range(len(EDGE_GRAPHS)))
    f0, st0 = engine.hks_sparse_batch(node_ptr, edge_ptr, edges, sel, [n for n, _ in EDGE_GRAPHS], [len(e) for _, e in EDGE_GRAPHS], list(TIMES),
                                      normalise=True)
    assert _bits(f0.cpu().numpy(), fn) and (st0.cpu().numpy() == _lib.ST_OK).all()


def test_bits_of_a_hub_of_4100_neighbours():
    """a split row: the hub's column, leaves at the chunk cuts and the last leaf against the restatement; the normalised output is the
    normalisation of the raw one"""
    n, e = _hub()
    times = (0.1, 10.0)
    f, df, st, _ = _sparse([(n, e)], times)
    fn, dfn, _, _ = _sparse([(n, e)], times, normalise=True)
    cols = [0, 1, 63, 64, 65, 2048, 4099, 4100]
    csr = hc.Csr(n, e)
    assert csr.deg[0] == 4100 and st[0] == 0
    for k, t in enumerate(times):
        v, d = hc.restate(n, e, t, cols=cols, csr=csr)
        assert _bits(f[k, cols], v) and _bits(df[k, cols], d), t
        nv, nd = hc.normalise(f[k], df[k])
        assert _bits(fn[k], nv) and _bits(dfn[k], nd), t


def test_bits_of_two_split_rows_at_later_slots():
    """two hubs of 300 and 700 neighbours behind a 40-cycle, their leaves chained: the split rows begin at entries other than 0 (chunk
    slots at an offset), beside a graph that cannot have one; hubs, leaves at the cuts and cycle nodes against the restatement"""
    n, e = hc.union(hc.cycle(40), hc.star(300), hc.star(700))
    e = np.concatenate([e, np.array([(i, i + 1) for i in range(41, 340)] + [(i, i + 1) for i in range(342, 1041)] + [(0, 40), (39, 341)])])
    csr = hc.Csr(n, e)
    assert csr.deg[40] == 301 and csr.deg[341] == 701 and csr.rowptr[40] > 0 and n == 1042
    small = (30, hc.random_connected(30, 5))
    f, df, st, nptr = _sparse([small, (n, e), small], TIMES)
    assert not st.any()
    cols = [0, 39, 40, 41, 104, 105, 340, 341, 342, 405, 406, 1041]
    for k, t in enumerate(TIMES):
        v, d = hc.restate(n, e, t, cols=cols, csr=csr)
        assert _bits(f[k, nptr[1]:nptr[2]][cols], v) and _bits(df[k, nptr[1]:nptr[2]][cols], d), t
    fs, dfs, _, _ = _sparse([small], TIMES)
    assert _bits(f[:, :30], fs) and _bits(f[:, nptr[2]:], fs) and _bits(df[:, :30], dfs)


def test_no_edges_and_no_nodes():
    from tlc_gnn_amd import _lib
    graphs = [(70, NO_EDGES), (0, NO_EDGES), (3, hc.cycle(3)[1]), (0, NO_EDGES)]
    for normalise in (False, True):
        f, df, st, nptr = _sparse(graphs, TIMES, normalise=normalise)
        assert (st == _lib.ST_OK).all()
        want = 1.0 / (1.0 + 1e-10) if normalise else 1.0
        assert (f[:, :70] == want).all() and (df[:, :70] == 0.0).all()
        assert np.isfinite(f[:, 70:]).all() and np.isfinite(df[:, 70:]).all()
    f, df, st, _ = _sparse([(0, NO_EDGES)], [1.0])
    assert f.shape == (1, 0) and st.tolist() == [_lib.ST_OK]


MIXED = [(129, hc.random_connected(129, 11)), (300, hc.random_connected(300, 12, extra=200)),
         hc.union(hc.star(300), hc.cycle(40), isolated=2), (65, hc.random_connected(65, 13)), (1, NO_EDGES)]


@pytest.fixture(scope="module")
def mixed():
    """the mixed batch at eight times, once: (f, df, node offsets), normalised"""
    f, df, st, nptr = _sparse(MIXED, EIGHT, normalise=True)
    assert not st.any()
    f.setflags(write=False)
    df.setflags(write=False)
    return f, df, nptr


def test_eight_times_equal_each_alone(mixed):
    f, df, _ = mixed
    for k, t in enumerate(EIGHT):
        f1, df1, _, _ = _sparse(MIXED, [t], normalise=True)
        assert _bits(f1[0], f[k]) and _bits(df1[0], df[k]), t


def test_alone_in_a_batch_and_in_a_selection(mixed):
    f, df, nptr = mixed
    for g in range(len(MIXED)):
        f1, df1, _, _ = _sparse([MIXED[g]], EIGHT, normalise=True)
        assert _bits(f1, f[:, nptr[g]:nptr[g + 1]]) and _bits(df1, df[:, nptr[g]:nptr[g + 1]]), g
    fs, dfs, st, _ = _sparse(MIXED, EIGHT, sel=[1, 2], normalise=True)
    a, b = nptr[1], nptr[3]
    assert _bits(fs[:, a:b], f[:, a:b]) and _bits(dfs[:, a:b], df[:, a:b])
    assert np.isnan(fs[:, :a]).all() and np.isnan(fs[:, b:]).all() and np.isnan(dfs[:, :a]).all() and np.isnan(dfs[:, b:]).all()


def test_least_workspace_and_run_against_run(mixed):
    from tlc_gnn_amd import engine
    f, df, _ = mixed
    lo, hi = engine.hks_sparse_work_bytes([n for n, _ in MIXED], [len(e) for _, e in MIXED], len(EIGHT))
    assert lo < hi
    for wb in (lo, (lo + hi) // 2 // 256 * 256, hi):
        f1, df1, st, _ = _sparse(MIXED, EIGHT, normalise=True, work_bytes=wb)
        assert _bits(f1, f) and _bits(df1, df) and not st.any(), wb
    f2, df2, _, _ = _sparse(MIXED, EIGHT, normalise=True)
    assert _bits(f2, f) and _bits(df2, df)


def test_against_the_eigensolver_and_the_large_tier():
    import torch
    from tlc_gnn_amd import engine
    graphs = [(20, hc.random_connected(20, 1)), (200, hc.random_connected(200, 2)), (256, hc.random_connected(256, 3)),
              (300, hc.random_connected(300, 4)), (700, hc.random_connected(700, 5))]
    times = [0.1, 10.0]
    node_ptr, edge_ptr, edges, nptr = _pack(graphs)
    f, df, st, _ = _sparse(graphs, times, normalise=True)
    assert not st.any()
    fj, dfj, stj = engine.hks_batch(node_ptr, edge_ptr, edges, times, dt=True)
    fl, dfl, stl = engine.hks_large_batch(node_ptr, edge_ptr, edges, [3, 4], [300, 700], times, dout=True)
    assert stj.cpu().tolist()[:3] == [0, 0, 0] and stl.cpu().tolist()[3:] == [0, 0]
    a = nptr[3]
    ev = max(np.abs(f[:, :a] - fj.cpu().numpy()[:, :a]).max(), np.abs(f[:, a:] - fl.cpu().numpy()[:, a:]).max())
    ed = max(np.abs(df[:, :a] - dfj.cpu().numpy()[:, :a]).max(), np.abs(df[:, a:] - dfl.cpu().numpy()[:, a:]).max())
    print("sparse tier against tlc_hks_batch / tlc_hks_large_batch: value %.2e derivative %.2e" % (ev, ed))
    assert ev <= 1e-11 and ed <= 2e-11
    assert torch.isfinite(fj[:, :a]).all()


@pytest.mark.parametrize("name", ["star K(1,4999)", "cycle C4097", "bipartite K(60,5000)", "union with isolated nodes"])
def test_closed_forms_above_the_old_cap(name):
    times = (0.1, 10.0)
    if name.startswith("star"):
        g, closed = hc.star(4999), lambda t: hc.star_closed(4999, t)
    elif name.startswith("cycle"):
        g, closed = hc.cycle(4097), lambda t: hc.cycle_closed(4097, t)
    elif name.startswith("bipartite"):
        g, closed = hc.bipartite(60, 5000), lambda t: hc.bipartite_closed(60, 5000, t)
    else:
        g = hc.union(hc.cycle(3000), hc.bipartite(20, 1500), isolated=50)
        closed = lambda t: hc.union_closed([hc.cycle_closed(3000, t), hc.bipartite_closed(20, 1500, t)], isolated=50)
    assert g[0] > 4096
    f, df, st, _ = _sparse([g], times)
    assert st.tolist() == [0]
    for k, t in enumerate(times):
        cv, cd = closed(t)
        ev, ed = np.abs(f[k] - cv).max(), np.abs(df[k] - cd).max()
        print("%s t %g: value %.2e derivative %.2e" % (name, t, ev, ed))
        assert ev <= 1e-11 and ed <= 2e-11


def test_refusals_leave_the_neighbours_alone():
    """every TLC_ST_BAD_INPUT of the contract: the refused graph's slices stay NaN, the graphs beside it keep their stand-alone bits"""
    import torch
    from tlc_gnn_amd import _lib
    A, B = (70, hc.random_connected(70, 21)), (300, hc.union(hc.star(280), hc.cycle(19))[1])
    cyc = hc.cycle(20)[1]
    alone = [_sparse([g], [0.1, 10.0], normalise=True) for g in (A, B)]
    bad = {"id out of range": (20, np.concatenate([cyc, [[3, 20]]])), "negative id": (20, np.concatenate([cyc, [[-1, 4]]])),
           "self loop": (20, np.concatenate([cyc, [[7, 7]]])), "repeated edge": (20, np.concatenate([cyc, [[4, 5]]])),
           "repeated edge, reversed": (20, np.concatenate([cyc, [[5, 4]]])), "more edges than pairs": (2, np.array([[0, 1], [0, 1]]))}

    def check(what, f, df, st, nptr, where):
        others = [g for g in range(3) if g != where]
        assert st[where] == _lib.ST_BAD_INPUT and st[others].tolist() == [0, 0], what
        assert np.isnan(f[:, nptr[where]:nptr[where + 1]]).all() and np.isnan(df[:, nptr[where]:nptr[where + 1]]).all(), what
        for g, ref in zip(others, alone):
            assert _bits(f[:, nptr[g]:nptr[g + 1]], ref[0]) and _bits(df[:, nptr[g]:nptr[g + 1]], ref[1]), (what, g)
    for what, X in bad.items():
        check(what, *_sparse([A, X, B], [0.1, 10.0], normalise=True), where=1)
    X = (20, cyc)
    check("declared node count", *_sparse([A, X, B], [0.1, 10.0], normalise=True, sel_nodes=[70, 21, 300]), where=1)
    check("declared edge count", *_sparse([A, X, B], [0.1, 10.0], normalise=True, sel_edges=[len(A[1]), 19, len(B[1])]), where=1)
    # offsets out of order: the last graph's edges end before they begin
    node_ptr, edge_ptr, edges, nptr = _pack([A, B, X])
    edge_ptr = edge_ptr.clone()
    edge_ptr[3] = edge_ptr[2] - 1
    check("offsets out of order", *_sparse([A, B, X], [0.1, 10.0], normalise=True, packed=(node_ptr, edge_ptr, edges, nptr)), where=2)


def test_return_codes_leave_the_outputs_untouched():
    import torch
    from tlc_gnn_amd import engine, _lib
    g = (70, hc.random_connected(70, 21))
    node_ptr, edge_ptr, edges, _ = _pack([g])
    out = torch.full((1, 70), -7.0, dtype=torch.float64, device="cuda")
    dout = torch.full((1, 70), -8.0, dtype=torch.float64, device="cuda")
    status = torch.full((1,), 99, dtype=torch.uint8, device="cuda")
    lo, _ = engine.hks_sparse_work_bytes([70], [len(g[1])])
    for kw in (dict(times=[64.5]), dict(times=[-1.0]), dict(times=[float("nan")]), dict(times=[0.1], work_bytes=lo - 256),
               dict(times=[0.1], sel_edges=[-1]), dict(times=[0.1], sel=[1])):
        args = dict(sel=[0], sel_nodes=[70], sel_edges=[len(g[1])])
        args.update(kw)
        with pytest.raises(_lib.TlcError, match="TLC_ERR_INVALID_ARG"):
            engine.hks_sparse_batch(node_ptr, edge_ptr, edges, args.pop("sel"), args.pop("sel_nodes"), args.pop("sel_edges"), args.pop("times"),
                                    out=out, status=status, dout=dout, **args)
        torch.cuda.synchronize()
        assert bool((out == -7.0).all()) and bool((dout == -8.0).all()) and int(status[0]) == 99, kw


def test_routing(monkeypatch):
    """{20, 257, 5 000} nodes with both tiers on the device: nothing on the host, every slice its own tier's bits; the default still
    calls the host for the 5 000-node graph"""
    import torch
    from tlc_gnn_amd import engine
    from tlc_gnn_amd.Knowledge_Distillation import data_utils_LP as kd_lp
    graphs = [(20, hc.random_connected(20, 1)), (257, hc.random_connected(257, 2)), hc.star(4999)]
    node_ptr, edge_ptr, edges, nptr = _pack(graphs)
    t = 0.1
    out = kd_lp.hks_filtration_device(node_ptr, edge_ptr, edges, t, int(nptr[-1]), hks_large='device', hks_sparse='device')
    assert kd_lp.hks_host_fallback == 0 and kd_lp.hks_large_device == 1 and kd_lp.hks_sparse_device == 1
    small = engine.hks_batch(*_pack([graphs[0]])[:3], [t])[0][0]
    large = engine.hks_large_batch(*_pack([graphs[1]])[:3], [0], [257], [t])[0][0]
    sparse = engine.hks_sparse_batch(*_pack([graphs[2]])[:3], [0], [5000], [4999], [t])[0][0]
    assert torch.equal(out[:20], small) and torch.equal(out[20:277], large) and torch.equal(out[277:], sparse)
    # without the large tier the sparse one takes both
    out2 = kd_lp.hks_filtration_device(node_ptr, edge_ptr, edges, t, int(nptr[-1]), hks_sparse='device')
    assert kd_lp.hks_host_fallback == 0 and kd_lp.hks_large_device == 0 and kd_lp.hks_sparse_device == 2
    assert torch.equal(out2[277:], sparse) and float((out2 - out).abs().max()) <= 1e-11
    # the default: the host, counted (its function replaced by the star's closed form: a dense eigh of 5 000 nodes takes minutes)
    calls = []
    ref = hc.star_closed(4999, t)[0]

    def closed_form(n, e, time):
        calls.append((n, len(e), time))
        return ref.copy() if n == 5000 else np.ones(n)
    monkeypatch.setattr(kd_lp, "hks_signature", closed_form)
    out3 = kd_lp.hks_filtration_device(node_ptr, edge_ptr, edges, t, int(nptr[-1]), hks_large='device')
    assert kd_lp.hks_host_fallback == 1 and kd_lp.hks_sparse_device == 0 and calls == [(5000, 4999, t)]
    assert np.array_equal(out3[277:].cpu().numpy(), ref / (ref.max() + 1e-10)) and torch.equal(out3[:277], out[:277])
    # a time the tier does not take: the host again
    kd_lp.hks_filtration_device(node_ptr, edge_ptr, edges, 100.0, int(nptr[-1]), hks_large='device', hks_sparse='device')
    assert kd_lp.hks_sparse_device == 0 and kd_lp.hks_host_fallback == 2


BIG = (4100, hc.random_connected(4100, 77, extra=4100))


def test_gradcheck_on_4100_nodes():
    import torch
    from tlc_gnn_amd import autograd
    node_ptr, edge_ptr, edges, _ = _pack([BIG])
    times = torch.tensor([1.3], dtype=torch.float64, device="cuda", requires_grad=True)
    with pytest.raises(RuntimeError, match="ST_TOO_LARGE"):
        autograd.hks_signature(times, node_ptr, edge_ptr, edges)                      # 'host', the default: no derivative, it raises
    out = autograd.hks_signature(times, node_ptr, edge_ptr, edges, hks_sparse='device')
    assert out.shape == (1, 4100) and out.requires_grad and bool(torch.isfinite(out).all())
    assert torch.autograd.gradcheck(lambda t: autograd.hks_signature(t, node_ptr, edge_ptr, edges, hks_sparse='device'), (times,))


def test_learning_the_time_on_4100_nodes():
    """target images made at t = 3; from t = 1, Adam steps on the squared image distance through
    topo.images(topo.hks_filtration(t, ..., hks_sparse='device')): the loss falls and t moves towards 3"""
    import torch
    from tlc_gnn_amd import topo
    node_ptr, edge_ptr, edges, _ = _pack([BIG])

    def images(t):
        return topo.images(topo.hks_filtration(t, node_ptr, edge_ptr, edges, hks_sparse='device'), node_ptr, edge_ptr, edges, pd_large='device')
    with torch.no_grad():
        target = images(torch.tensor(3.0, dtype=torch.float64))
    t = torch.tensor(1.0, dtype=torch.float64, device="cuda", requires_grad=True)
    opt = torch.optim.Adam([t], lr=0.1)
    losses = []
    for _ in range(25):
        opt.zero_grad()
        loss = ((images(t) - target) ** 2).sum()
        loss.backward()
        assert t.grad is not None and bool(torch.isfinite(t.grad))
        opt.step()
        losses.append(float(loss.detach()))
    print("learned time: t 1 -> %.4f, loss %.4e -> %.4e" % (float(t.detach()), losses[0], losses[-1]))
    assert losses[-1] < losses[0] and 1.0 < float(t.detach()) and abs(float(t.detach()) - 3.0) < 2.0


def test_ground_truth_packed_on_5000_nodes():
    import torch
    from tlc_gnn_amd.Knowledge_Distillation import data_utils_GC as kd, data_utils_LP as kd_lp
    n = 5000
    packed = kd.pack_dataset([(n, hc.random_connected(n, 5, extra=n))])
    gt = kd.ground_truth_packed(*packed, filt='hks', hks_time=10, hks_sparse='device', pd_large='device')
    assert kd_lp.hks_sparse_device == 1 and kd_lp.hks_host_fallback == 0
    assert gt.ok.cpu().tolist() == [True]
    d0, d1, img, fv = gt.tuples()[0][:4]
    assert len(fv) == n and len(d0) > 0 and len(d1) > 0 and np.isfinite(np.asarray(img)).all() and np.asarray(img).any()
    # normalised: the maximum is mx / (mx + 1e-10), and hks_t(v) >= deg(v) / 2m > 1e-5 here (the eigenvalue 0 alone)
    assert 1.0 - 1e-5 < max(fv) < 1.0 and min(fv) > 0.0

"""GPU: heat-kernel signatures of graphs above TLC_HKS_NMAX nodes on the device (tlc_hks_large_batch, csrc/hks_large.hip;
hks_large='device' of the Knowledge_Distillation drop-ins) against the host route (`data_utils_LP.hks_signature`: scipy's eigh) and
against closed forms.

Bound: 1e-11 absolute, the bound of tests/test_gpu_hks.py for the eigensolver tiers.  The kernel sums non-negative numbers only
(a degree-14 Taylor series of exp(X), ||X|| <= 1/2, then at most 6 squarings): a numpy restatement stays below 3e-13 on these cases.
T = _lib.HKS_LARGE_TILE is HKSL_T (the output-tile side) and Ks = _lib.HKS_LARGE_KSTEP is HKSL_KS (the K-step) of the product kernel."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TIMES = (0.1, 10.0)


def _close_multiset(a, b, tol):
    """two point sets equal as multisets up to `tol` (the helper of test_gpu_hks.py)"""
    a, b = np.asarray(a, dtype=np.float64).reshape(-1, 2), np.asarray(b, dtype=np.float64).reshape(-1, 2)
    if len(a) != len(b):
        return False
    if not len(a):
        return True
    return bool(np.abs(np.sort(a[:, 0]) - np.sort(b[:, 0])).max() <= tol and np.abs(np.sort(a[:, 1]) - np.sort(b[:, 1])).max() <= tol
                and np.abs(a.sum(0) - b.sum(0)).max() <= tol * len(a))


def _random_connected(n, seed, extra=None):
    """a random tree plus about 2n extra edges: simple, connected, each edge once (lower id first)"""
    rs = np.random.RandomState(seed)
    es = {(int(rs.randint(i)), i) for i in range(1, n)}
    for _ in range((2 * n if extra is None else extra) if n > 1 else 0):
        a, b = (int(x) for x in rs.randint(n, size=2))
        if a != b:
            es.add((min(a, b), max(a, b)))
    return np.array(sorted(es), dtype=np.int64).reshape(-1, 2)


def _pack(graphs):
    import torch
    node_ptr = np.concatenate([[0], np.cumsum([n for n, _ in graphs])]).astype(np.int64)
    edge_ptr = np.concatenate([[0], np.cumsum([len(e) for _, e in graphs])]).astype(np.int64)
    edges = np.concatenate([np.asarray(e, dtype=np.int64).reshape(-1, 2) for _, e in graphs]).astype(np.int32).reshape(-1, 2)
    return torch.from_numpy(node_ptr).cuda(), torch.from_numpy(edge_ptr).cuda(), torch.from_numpy(edges).cuda(), node_ptr


_HOST = {}


def _host(name, n, e, t):
    """the host route, normalised; computed once per (case, time) and shared by the tests"""
    from tlc_gnn_amd.Knowledge_Distillation.data_utils_LP import hks_signature
    if (name, t) not in _HOST:
        v = hks_signature(n, e, t)
        v = v / (max(v) + 1e-10)
        v.setflags(write=False)
        _HOST[(name, t)] = v
    return _HOST[(name, t)]


def _large(graphs, times, sel=None, sel_nodes=None, **kw):
    """engine.hks_large_batch on a packed list of (n, edges); sel: every graph unless given"""
    from tlc_gnn_amd import engine
    node_ptr, edge_ptr, edges, nptr = _pack(graphs)
    sel = list(range(len(graphs))) if sel is None else sel
    sel_nodes = [graphs[k][0] for k in sel] if sel_nodes is None else sel_nodes
    f, st = engine.hks_large_batch(node_ptr, edge_ptr, edges, sel, sel_nodes, times, **kw)
    return f, st, nptr


def _star(leaves):
    return leaves + 1, np.array([(0, i) for i in range(1, leaves + 1)])


def _cycle(n):
    return n, np.array([(i, i + 1) for i in range(n - 1)] + [(0, n - 1)])


def _complete(n):
    return n, np.array([(i, j) for i in range(n) for j in range(i + 1, n)])


def _bipartite(a, b):
    return a + b, np.array([(i, a + j) for i in range(a) for j in range(b)])


def _grid(k):
    return k * k, np.array([(i * k + j, i * k + j + 1) for i in range(k) for j in range(k - 1)] +
                           [(i * k + j, i * k + j + k) for i in range(k - 1) for j in range(k)])


def _two_components_and_isolated():
    """585 nodes: components 0 .. 299 and 300 .. 579, nodes 580 .. 584 isolated -- padding and degree 0 meet in the last tile"""
    return 585, np.concatenate([_random_connected(300, 51), _random_connected(280, 52) + 300])


_CASES = []


def _cases():
    from tlc_gnn_amd import _lib
    if _CASES:
        return _CASES
    T, Ks = _lib.HKS_LARGE_TILE, _lib.HKS_LARGE_KSTEP
    sizes = {257, 300, 513, 1, 2, 3, 33, 200}
    for unit in (16, T, Ks):
        b = (_lib.HKS_NMAX // unit + 1) * unit                   # the first multiple above 256
        sizes |= {b - 1, b, b + 1}
    cases = [("random%d" % n, n, _random_connected(n, 2000 + n)) for n in sorted(sizes)]
    cases.append(("star K(1,600)",) + _star(600))
    cases.append(("cycle C400",) + _cycle(400))
    cases.append(("complete K320",) + _complete(320))
    cases.append(("bipartite K(150,170)",) + _bipartite(150, 170))
    cases.append(("grid 18x18",) + _grid(18))
    cases.append(("two components + 5 isolated",) + _two_components_and_isolated())
    order = np.random.RandomState(11).permutation(len(cases))
    _CASES.extend(cases[i] for i in order)
    return _CASES


_BATCH = {}


def _batch():
    """the batch of the size test, normalised, both times: computed once"""
    if not _BATCH:
        cases = _cases()
        f, st, nptr = _large([(n, e) for _, n, e in cases], TIMES)
        _BATCH.update(f=f, st=st, nptr=nptr)
    return _BATCH["f"], _BATCH["st"], _BATCH["nptr"]


def test_sizes_tile_boundaries_and_spectra_in_one_batch_against_host():
    """Random connected graphs at 257, 300, 513, at b - 1, b, b + 1 for the first multiple b above 256 of 16, T and Ks, and at 1, 2, 3,
    33, 200; a 600-leaf star, C400, K320, K(150,170), an 18 x 18 grid, two components plus isolated nodes: ONE shuffled batch, times
    0.1 and 10, every status OK and 1e-11 of the host route."""
    from tlc_gnn_amd import _lib
    cases = _cases()
    assert {n for _, n, _ in cases} >= {257, 271, 272, 273, 319, 320, 321, 300, 513, 585, 601, 400, 324, 1, 2, 3, 33, 200}
    assert _lib.HKS_LARGE_TILE == 64 and _lib.HKS_LARGE_KSTEP == 16
    f, st, nptr = _batch()
    f, st = f.cpu().numpy(), st.cpu().numpy()
    assert f.shape == (2, nptr[-1])
    assert np.array_equal(st, np.zeros(len(cases), dtype=np.uint8)), st
    worst = 0.0
    for k, (name, n, e) in enumerate(cases):
        for ti, t in enumerate(TIMES):
            diff = np.abs(f[ti, nptr[k]:nptr[k + 1]] - _host(name, n, e, t)).max()
            print("%-28s n %4d t %4.1f  |device - host| %.2e" % (name, n, t, diff))
            worst = max(worst, diff)
            assert diff <= 1e-11, (name, t, diff)
    print("worst |device - host| %.2e" % worst)


def test_closed_forms_raw_values_up_to_the_cap():
    """Raw values against closed forms (no host eigh), 1e-11, times 0.1, 10, 64 and 0 (every value 1): the star K(1, 4095) at
    n = TLC_HKS_LARGE_NMAX, K320, C400, K(150,170)."""
    from tlc_gnn_amd import _lib
    assert _lib.HKS_LARGE_NMAX == 4096 and _lib.HKS_LARGE_TIME_MAX == 64.0
    times = (0.1, 10.0, 64.0, 0.0)
    m = 4095

    def star(t):
        v = np.full(m + 1, 1 / (2 * m) + np.exp(-2 * t) / (2 * m) + (1 - 1 / m) * np.exp(-t))
        v[0] = 0.5 + np.exp(-2 * t) / 2
        return v

    def bip(t, a=150, b=170):
        side = lambda c: 1 / (2 * c) + np.exp(-2 * t) / (2 * c) + (1 - 1 / c) * np.exp(-t)
        return np.concatenate([np.full(a, side(a)), np.full(b, side(b))])
    forms = [("star K(1,4095)", _star(m), star),
             ("complete K320", _complete(320), lambda t: np.full(320, 1 / 320 + (1 - 1 / 320) * np.exp(-t * 320 / 319))),
             ("cycle C400", _cycle(400), lambda t: np.full(400, np.exp(-t * (1 - np.cos(2 * np.pi * np.arange(400) / 400))).sum() / 400)),
             ("bipartite K(150,170)", _bipartite(150, 170), bip)]
    f, st, nptr = _large([g for _, g, _ in forms], times, normalise=False)
    f = f.cpu().numpy()
    assert st.cpu().tolist() == [0] * len(forms)
    worst = 0.0
    for k, (name, (n, e), form) in enumerate(forms):
        for ti, t in enumerate(times):
            got = f[ti, nptr[k]:nptr[k + 1]]
            diff = np.abs(got - form(t)).max()
            print("%-22s n %4d t %5.1f  |device - closed form| %.2e" % (name, n, t, diff))
            worst = max(worst, diff)
            assert diff <= 1e-11, (name, t, diff)
            if t == 0.0:
                assert np.array_equal(got, np.ones(n)), name
    print("worst |device - closed form| %.2e" % worst)


def _pubmed_like_1205():
    """a hub with 800 leaves, a random connected remainder of 404 nodes joined to the hub, random extra edges over everything"""
    rs = np.random.RandomState(1205)
    es = {(0, i) for i in range(1, 801)}
    es |= {(int(a) + 801, int(b) + 801) for a, b in _random_connected(404, 77)}
    es.add((0, 801))
    for _ in range(1500):
        a, b = (int(x) for x in rs.randint(1205, size=2))
        if a != b:
            es.add((min(a, b), max(a, b)))
    return 1205, np.array(sorted(es), dtype=np.int64)


def test_largest_pubmed_shaped_vicinity_against_host():
    n, e = _pubmed_like_1205()
    f, st, _ = _large([(n, e)], TIMES)
    assert st.cpu().tolist() == [0]
    f = f.cpu().numpy()
    for ti, t in enumerate(TIMES):
        diff = np.abs(f[ti] - _host("pubmed1205", n, e, t)).max()
        print("hub + 800 leaves + remainder, n 1205 t %4.1f  |device - host| %.2e" % (t, diff))
        assert diff <= 1e-11, (t, diff)


def test_more_work_items_than_the_grid():
    """72 random graphs of 257 .. 320 nodes (15 tiles each: more work items than the product kernel's grid of four workgroups per
    CU): each within 1e-11 of the host route, and its bits those of its stand-alone call."""
    import torch
    rs = np.random.RandomState(5)
    graphs = [(int(n), _random_connected(int(n), 3000 + i)) for i, n in enumerate(rs.randint(257, 321, size=72))]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert 15 * len(graphs) > 4 * cus or cus > 256
    f, st, nptr = _large(graphs, TIMES)
    assert int(st.sum()) == 0
    fh = f.cpu().numpy()
    worst = 0.0
    for k, (n, e) in enumerate(graphs):
        for ti, t in enumerate(TIMES):
            worst = max(worst, np.abs(fh[ti, nptr[k]:nptr[k + 1]] - _host("many%d" % k, n, e, t)).max())
        alone, st1, _ = _large([(n, e)], TIMES)
        assert int(st1.sum()) == 0 and torch.equal(alone, f[:, nptr[k]:nptr[k + 1]]), k
    print("72 graphs: worst |device - host| %.2e" % worst)
    assert worst <= 1e-11


def test_deterministic_and_independent_of_batch_group_and_workspace():
    """The batch of the size test twice: same bits.  Each graph alone: the bits of its slice.  work_bytes = min_bytes (one group after
    the other) against all_bytes.  Two times in one call against two single-time calls.  Raw / (max + 1e-10) in torch fp64: the bits
    of the normalised output.  Every second large graph selected: the other slices stay NaN, the other status bytes as given."""
    import torch
    from tlc_gnn_amd import engine
    cases = _cases()
    graphs = [(n, e) for _, n, e in cases]
    f1, st1, nptr = _batch()
    f2, st2, _ = _large(graphs, TIMES)
    assert int(st1.sum()) == 0 and torch.equal(f1, f2) and torch.equal(st1, st2)
    for k, (name, n, e) in enumerate(cases):
        alone, st, _ = _large([(n, e)], TIMES)
        assert int(st.sum()) == 0 and torch.equal(alone, f1[:, nptr[k]:nptr[k + 1]]), name
    lo, hi = engine.hks_large_work_bytes([n for n, _ in graphs], len(TIMES))
    assert lo < hi
    for wb in (lo, hi, (lo + hi) // 2 // 16 * 16):
        f3, st3, _ = _large(graphs, TIMES, work_bytes=wb)
        assert int(st3.sum()) == 0 and torch.equal(f1, f3), wb
    for ti, t in enumerate(TIMES):
        single, _, _ = _large(graphs, [t])
        assert torch.equal(single[0], f1[ti]), t
    raw, _, _ = _large(graphs, TIMES, normalise=False)
    for k in range(len(cases)):
        sl = raw[:, nptr[k]:nptr[k + 1]]
        assert torch.equal(sl / (sl.max(dim=1, keepdim=True).values + 1e-10), f1[:, nptr[k]:nptr[k + 1]]), cases[k][0]
    large = [k for k, (n, _) in enumerate(graphs) if n > 256]
    sel = large[::2]
    node_ptr, edge_ptr, edges, _ = _pack(graphs)
    out = torch.full((2, int(nptr[-1])), float("nan"), dtype=torch.float64, device="cuda")
    status = torch.full((len(graphs),), 9, dtype=torch.uint8, device="cuda")
    engine.hks_large_batch(node_ptr, edge_ptr, edges, sel, [graphs[k][0] for k in sel], TIMES, out=out, status=status)
    for k in range(len(graphs)):
        sl = out[:, nptr[k]:nptr[k + 1]]
        if k in sel:
            assert int(status[k]) == 0 and torch.equal(sl, f1[:, nptr[k]:nptr[k + 1]]), k
        else:
            assert int(status[k]) == 9 and bool(torch.isnan(sl).all()), k


def test_refusals_are_a_status_or_a_return_code():
    """A 4 097-node path: TLC_ST_TOO_LARGE, slice still NaN, the neighbours bit-equal to their stand-alone values.  An id of n, an id of
    -1, a self loop, (a,b)(a,b), (a,b)(b,a), a declared node count that is not the device's: TLC_ST_BAD_INPUT for that graph alone.
    A time of 64.5, -0.1 or nan, a descending or out-of-range h_sel, work_bytes = min_bytes - 16: an error, the output untouched."""
    import torch
    from tlc_gnn_amd import engine, _lib
    bad, big = _lib.ST_BAD_INPUT, _lib.HKS_LARGE_NMAX + 1
    good = (260, _random_connected(260, 4))
    base = _random_connected(270, 6)
    path = (big, np.array([(i, i + 1) for i in range(big - 1)]))
    graphs = [good, path, (270, np.concatenate([base, [(5, 270)]])), good, (270, np.concatenate([base, [(-1, 7)]])),
              (270, np.concatenate([base, [(9, 9)]])), (270, np.concatenate([base, base[100:101]])),
              (270, np.concatenate([base, base[200:201, ::-1]])), good, (270, base)]
    f, st, nptr = _large(graphs, TIMES)
    assert st.cpu().tolist() == [0, _lib.ST_TOO_LARGE, bad, 0, bad, bad, bad, bad, 0, 0]
    alone, _, _ = _large([good], TIMES)
    for k in (0, 3, 8):
        assert torch.equal(f[:, nptr[k]:nptr[k + 1]], alone), k
    alone, _, _ = _large([graphs[9]], TIMES)
    assert torch.equal(f[:, nptr[9]:nptr[10]], alone)
    assert bool(torch.isnan(f[:, nptr[1]:nptr[3]]).all()) and bool(torch.isnan(f[:, nptr[4]:nptr[8]]).all())
    # a declared count that is not node_ptr[g + 1] - node_ptr[g]
    for wrong in (259, 261, 0, 320):
        f2, st2, nptr2 = _large([good, good], [0.1], sel_nodes=[260, wrong])
        assert st2.cpu().tolist() == [0, bad], wrong
        assert torch.equal(f2[:, :260], f[:1, :260]) and bool(torch.isnan(f2[:, 260:]).all()), wrong
    # return codes: nothing launched, nothing written
    node_ptr, edge_ptr, edges, _ = _pack([good, good])
    lo, _ = engine.hks_large_work_bytes([260, 260], 1)

    def call(sel=(0, 1), times=(0.1,), work_bytes=None):
        out = torch.full((len(times), 520), 7.0, dtype=torch.float64, device="cuda")
        status = torch.full((2,), 9, dtype=torch.uint8, device="cuda")
        with pytest.raises(_lib.TlcError):
            engine.hks_large_batch(node_ptr, edge_ptr, edges, list(sel), [260] * len(sel), list(times), out=out, status=status,
                                   work_bytes=work_bytes)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()) and status.cpu().tolist() == [9, 9]
    call(times=(64.5,))
    call(times=(-0.1,))
    call(times=(0.1, float("nan")))
    call(times=(float("inf"),))
    call(sel=(1, 0))
    call(sel=(0, 0))
    call(sel=(0, 2))
    call(sel=(-1, 0))
    call(work_bytes=lo - 16)
    out, st3 = engine.hks_large_batch(node_ptr, edge_ptr, edges, [0, 1], [260, 260], [0.1], work_bytes=lo)
    assert st3.cpu().tolist() == [0, 0] and torch.equal(out[:, :260], out[:, 260:])


def _hub_graph():
    """a hub of degree 300 whose leaves carry a few edges of their own (cycles through the hub) and two pendant paths of length 2:
    the hop-1 vicinity of the hub has 301 nodes"""
    es = [(0, i) for i in range(1, 301)] + [(i, i + 1) for i in range(1, 120, 2)] + [(i, i + 7) for i in range(130, 200, 9)]
    es += [(300, 301), (301, 302), (299, 303), (303, 304)]
    return 305, np.array(es, dtype=np.int64)


def test_wrappers_route_large_graphs_to_the_large_tier(monkeypatch):
    """hks_filtration_device with hks_large='device': nothing on the host, the small slices as engine.hks_batch alone, the large one
    1e-11 of the host; the default is today's behaviour; a time above the cap or a graph above the size cap takes the host and is
    counted."""
    import torch
    from tlc_gnn_amd import engine, _lib
    from tlc_gnn_amd.Knowledge_Distillation import data_utils_LP as kd_lp
    graphs = [(20, _random_connected(20, 1)), (257, _random_connected(257, 2)), (45, _random_connected(45, 3))]
    node_ptr, edge_ptr, edges, nptr = _pack(graphs)
    small = [engine.hks_batch(*_pack([graphs[k]])[:3], [0.1])[0][0] for k in (0, 2)]
    host = _host("wrap257", 257, graphs[1][1], 0.1)
    out = kd_lp.hks_filtration_device(node_ptr, edge_ptr, edges, 0.1, int(nptr[-1]), hks_large='device')
    assert kd_lp.hks_host_fallback == 0 and kd_lp.hks_large_device == 1
    assert torch.equal(out[:20], small[0]) and torch.equal(out[nptr[2]:], small[1])
    diff = np.abs(out[nptr[1]:nptr[2]].cpu().numpy() - host).max()
    print("hks_filtration_device, n 257: |large tier - host| %.2e" % diff)
    assert diff <= 1e-11
    out = kd_lp.hks_filtration_device(node_ptr, edge_ptr, edges, 0.1, int(nptr[-1]))
    assert kd_lp.hks_host_fallback == 1 and kd_lp.hks_large_device == 0
    assert np.array_equal(out[nptr[1]:nptr[2]].cpu().numpy(), host)
    assert torch.equal(out[:20], small[0]) and torch.equal(out[nptr[2]:], small[1])
    # a time above TLC_HKS_LARGE_TIME_MAX: the host, counted
    out = kd_lp.hks_filtration_device(node_ptr, edge_ptr, edges, 100.0, int(nptr[-1]), hks_large='device')
    assert kd_lp.hks_host_fallback == 1 and kd_lp.hks_large_device == 0
    assert np.array_equal(out[nptr[1]:nptr[2]].cpu().numpy(), _host("wrap257", 257, graphs[1][1], 100.0))
    # a graph above TLC_HKS_LARGE_NMAX: the host, counted.  The routing is what is tested: the host function is replaced by the
    # star's closed form for this call (a dense eigh of 4 097 nodes takes the better part of a minute)
    big = _lib.HKS_LARGE_NMAX + 1
    g2 = [graphs[1], _star(big - 1)]
    node_ptr, edge_ptr, edges, nptr = _pack(g2)
    m, t, calls = big - 1, 0.1, []
    ref = np.full(big, 1 / (2 * m) + np.exp(-2 * t) / (2 * m) + (1 - 1 / m) * np.exp(-t))
    ref[0] = 0.5 + np.exp(-2 * t) / 2

    def closed_form(n, e, time):
        calls.append((n, len(e), time))
        return ref.copy()
    monkeypatch.setattr(kd_lp, "hks_signature", closed_form)
    out = kd_lp.hks_filtration_device(node_ptr, edge_ptr, edges, t, int(nptr[-1]), hks_large='device')
    assert kd_lp.hks_host_fallback == 1 and kd_lp.hks_large_device == 1 and calls == [(big, m, t)]
    assert np.abs(out[:257].cpu().numpy() - host).max() <= 1e-11
    assert np.array_equal(out[257:].cpu().numpy(), ref / (ref.max() + 1e-10))


def test_drop_ins_large_tier_against_host_fallback():
    """compute_persistence_image_batch (graph classification) and NodeVicinities.batch / compute_persistence_image (node
    classification) at hop 1 around a hub of degree 300 -- a 301-node vicinity -- with hks_large='device' against 'host': values 1e-11,
    diagram sizes equal, diagrams as multisets 1e-9, images 1e-7 * max(1, |ref|)."""
    import torch
    from tlc_gnn_amd.Knowledge_Distillation import data_utils_NC as kd_nc, data_utils_LP as kd_lp, data_utils_GC as kd_gc
    n, e = _hub_graph()

    def same(dev, host):
        o0, e1, img, fv, ei, pi0, pi1 = dev[:7]
        r0, r1, rimg, rfv, rei, rpi0, rpi1 = host[:7]
        diff = np.abs(np.array(fv) - np.array(rfv)).max()
        print("n %d: |large tier - host| %.2e" % (len(fv), diff))
        assert diff <= 1e-11
        assert torch.equal(ei, rei) and len(o0) == len(r0) and len(e1) == len(r1) and len(e1) > 0
        assert _close_multiset(o0, r0, 1e-9) and _close_multiset(e1, r1, 1e-9)
        for got, ref in ((img, rimg), (pi0, rpi0), (pi1, rpi1)):
            assert np.abs(np.asarray(got) - ref).max() <= 1e-7 * max(1.0, np.abs(ref).max())
    for t in TIMES:
        kw = dict(filt='hks', hks_time=t, hks_backend='device')
        small = (30, _random_connected(30, 8))
        dev = kd_gc.compute_persistence_image_batch([small, (n, e)], hks_large='device', **kw)
        assert kd_lp.hks_host_fallback == 0 and kd_lp.hks_large_device == 1
        host = kd_gc.compute_persistence_image_batch([small, (n, e)], **kw)
        assert kd_lp.hks_host_fallback == 1 and kd_lp.hks_large_device == 0
        assert len(host[1][3]) == 305
        same(dev[1], host[1])
        assert dev[0][3] == host[0][3]
        vic = kd_nc.NodeVicinities(e, None)
        bd = vic.batch([0, 302], 1, hks_large='device', **kw)
        assert bd["hks_host_fallback"] == 0 and bd["hks_large_device"] == 1
        bh = vic.batch([0, 302], 1, **kw)
        assert bh["hks_host_fallback"] == 1 and bh["hks_large_device"] == 0
        for key in ("node_ptr", "edge_ptr", "ids", "edges", "status"):
            assert torch.equal(bd[key], bh[key]), key
        assert int(bd["node_ptr"][1]) == 301 and float((bd["f"] - bh["f"]).abs().max()) <= 1e-11
        assert torch.equal(bd["f"][301:], bh["f"][301:])
        same(kd_nc.compute_persistence_image(e, 0, hop=1, mode='PI', hks_large='device', **kw),
             kd_nc.compute_persistence_image(e, 0, hop=1, mode='PI', **kw))
        assert kd_lp.hks_host_fallback == 1                      # (the second call: the host route)
        # the keyword has no effect on another filtration or on the host backend
        a = vic.batch([0], 1, filt='degree', hks_large='device')
        assert torch.equal(a["f"], vic.batch([0], 1, filt='degree')["f"]) and "hks_large_device" not in a
        assert torch.equal(vic.batch([0], 1, filt='hks', hks_time=t, hks_large='device')["f"], vic.batch([0], 1, filt='hks', hks_time=t)["f"])

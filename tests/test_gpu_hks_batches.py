"""GPU: tlc_hks_batch (csrc/hks.hip) where tests/test_gpu_hks.py does not reach.

  a  full batches: more graphs per tier than the tier's grid has units, so every ticket loop runs on and every LDS / workspace slot is
     re-initialised after a graph of another size; hks_bin_kernel over many full wavefronts with mixed tiers, n = 0 and refused graphs;
  b  closed forms (tests/helpers.py) that no eigensolver enters, at the tier edges and with TLC_HKS_TMAX times in one call;
  c  graphs that are not connected, nodes of degree 0, m = 0, n = 0, B = 0;
  d  refusals: TLC_ST_BAD_INPUT for ids equal to n, negative ids, repeated edges, offsets out of order or beyond the totals;
  e  the wrapper's branches for TLC_ST_NOT_CONVERGED (host values) and TLC_ST_BAD_INPUT (RuntimeError).

Bounds: 1e-11 on values against the host route (the project's bound, test_gpu_hks.py) and 1e-11 * max(1, t / 10) against the closed
forms (helpers.hks_bound: the same bound with the linear-in-t error model); LAPACK's own distance from the closed forms is 1.0e-12 at
worst (tests/test_cpu_hks_host.py pins it).  Bit equality wherever the header promises it: a graph's values do not depend on the batch."""
import ctypes as C
import functools

import numpy as np
import pytest

from helpers import (HKS_CLOSED_FORM_SIZES, HKS_CLOSED_FORM_TIMES, hks_bound, hks_closed_form_cases, hks_stationary, random_connected)

pytestmark = pytest.mark.gpu
TIMES = (0.1, 10.0)
MULTI = np.array([(0, 1), (1, 2), (2, 3), (1, 3)])
NO_EDGES = np.zeros((0, 2), dtype=np.int64)


def _pack(graphs):
    import torch
    node_ptr = np.concatenate([[0], np.cumsum([n for n, _ in graphs])]).astype(np.int64)
    edge_ptr = np.concatenate([[0], np.cumsum([len(e) for _, e in graphs])]).astype(np.int64)
    edges = np.concatenate([np.zeros((0, 2), dtype=np.int64)] + [np.asarray(e, dtype=np.int64).reshape(-1, 2) for _, e in graphs]).astype(np.int32)
    return torch.from_numpy(node_ptr).cuda(), torch.from_numpy(edge_ptr).cuda(), torch.from_numpy(edges).cuda(), node_ptr


def _host(n, e, t):
    from tlc_gnn_amd.Knowledge_Distillation.data_utils_LP import hks_signature
    v = hks_signature(n, e, t)
    return v / (max(v) + 1e-10)


def _alone(graph, times=TIMES, normalise=True):
    """the graph in a batch of its own -> (f[T, n], status byte)"""
    from tlc_gnn_amd import engine
    a = _pack([graph])
    f, st = engine.hks_batch(a[0], a[1], a[2], times, normalise=normalise)
    return f, int(st[0])


def _same_bits(a, b):
    """torch.equal on the bit patterns: NaN slices (refused graphs) compare equal to NaN"""
    import torch
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


# ---- a. full batches ------------------------------------------------------------------------------------------------------------------
POOL_SIZES = ((1, 2, 3, 5, 16, 17, 31, 32), (33, 34, 47, 63, 64), (65, 66, 81, 95, 96), (97, 98, 111, 128))    # WAVE, WG64, WG96, GLOBAL


def _tier_of(n):
    return 0 if n <= 32 else 1 if n <= 64 else 2 if n <= 96 else 3


def _pool():
    """40 distinct graphs: a random connected one per size of POOL_SIZES, and complete graphs, stars, cycles, complete bipartite graphs
    in every tier"""
    pool = [("random%d" % n, n, random_connected(n, 2000 + n)) for sizes in POOL_SIZES for n in sizes]
    structured = {c[0]: c for c in hks_closed_form_cases((5, 16, 17, 31, 32, 33, 47, 63, 64, 65, 81, 95, 96, 97, 98, 111, 128))}
    for name in ("cycle5", "complete5", "star17", "cycle31", "complete32", "bipartite16",
                 "star33", "cycle47", "complete64", "bipartite63",
                 "complete65", "star81", "cycle96", "bipartite95",
                 "star97", "cycle111", "complete128", "bipartite98"):
        pool.append(structured[name][:3])
    assert len(pool) == 40 and len({(n, e.tobytes()) for _, n, e in pool}) == 40
    return pool


def _full_batch(cus, pool, seed):
    """Shuffled copies of the pool: 1.25 x 8 cus WAVE graphs (a wavefront each, four per workgroup, 2 cus workgroups), 1.5 x 2 cus WG64,
    2 x cus WG96 and 2 x cus GLOBAL graphs, so that units of every tier draw a second ticket; nine graphs without nodes, two above the
    cap and three with bad edges in between.  Returns [(pool index or None, (n, edges), expected status)]."""
    from tlc_gnn_amd import _lib
    rs = np.random.RandomState(seed)
    want = (10 * cus, 3 * cus, 2 * cus, 2 * cus)
    items = []
    for tier in range(4):
        members = [k for k, (_, n, _) in enumerate(pool) if _tier_of(n) == tier]
        for c in range(want[tier]):
            k = members[c % len(members)]
            items.append((k, (pool[k][1], pool[k][2]), _lib.ST_OK))
    items += [(None, (0, NO_EDGES), _lib.ST_OK)] * 9
    for big in (_lib.HKS_NMAX + 1, _lib.HKS_NMAX + 44):
        items.append((None, (big, random_connected(big, big)), _lib.ST_TOO_LARGE))
    for bad in ((4, np.array([(0, 1), (1, 7)])), (3, np.array([(1, 1)])), (4, np.concatenate([MULTI, MULTI[2:3]]))):
        items.append((None, bad, _lib.ST_BAD_INPUT))
    while len(items) % 64 == 0:
        items.append((None, (0, NO_EDGES), _lib.ST_OK))
    return [items[i] for i in rs.permutation(len(items))]


def _check_batch(items, alone, label):
    """one call on `items`: statuses position by position, every slice the bits of its pool graph alone, refused slices NaN; -> f"""
    import torch
    from tlc_gnn_amd import engine
    node_ptr, edge_ptr, edges, nptr = _pack([g for _, g, _ in items])
    f, st = engine.hks_batch(node_ptr, edge_ptr, edges, TIMES)
    want_st = np.array([s for _, _, s in items], dtype=np.uint8)
    got_st = st.cpu().numpy()
    wrong = np.nonzero(got_st != want_st)[0]
    assert len(wrong) == 0, (label, "status", [(int(i), items[i][1][0], int(got_st[i]), int(want_st[i])) for i in wrong[:10]], len(wrong))
    want = torch.full((len(TIMES), int(nptr[-1])), float("nan"), dtype=torch.float64)
    for i, (k, _, _) in enumerate(items):
        if k is not None:
            want[:, nptr[i]:nptr[i + 1]] = alone[k]
    if not _same_bits(f, want.cuda()):
        fh, wh = f.cpu().numpy().view(np.int64), want.numpy().view(np.int64)
        bad = [(i, items[i][1][0], items[i][0]) for i in range(len(items)) if not np.array_equal(fh[:, nptr[i]:nptr[i + 1]], wh[:, nptr[i]:nptr[i + 1]])]
        raise AssertionError((label, "slices that differ from the graph alone (position, n, pool index)", bad[:10], len(bad)))
    for i, (k, (n, _), s) in enumerate(items):
        if k is None and n:
            assert bool(torch.isnan(f[:, nptr[i]:nptr[i + 1]]).all()), (label, i)
    return f


def test_full_batches_every_tier_draws_second_tickets():
    """About 4 400 graphs in one call (B not a multiple of 64): more per tier than the tier's grid has wavefronts / workgroups, sizes
    mixed so that a unit takes a smaller graph after a larger one, an odd n after an even one, and a workspace slot again.  Statuses
    exact; every copy bit-equal to its pool graph computed alone; the pool within 1e-11 of the host route; refused slices NaN; a
    second run and the reversed batch (tickets land elsewhere) give the same bits."""
    import torch
    from tlc_gnn_amd import _lib
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    pool = _pool()
    alone, worst = [], 0.0
    for name, n, e in pool:
        f, st = _alone((n, e))
        assert st == _lib.ST_OK, name
        fh = f.cpu().numpy()
        for ti, t in enumerate(TIMES):
            d = np.abs(fh[ti] - _host(n, e, t)).max()
            worst = max(worst, d)
            assert d <= 1e-11, (name, t, d)
        alone.append(f.cpu())
    print("pool of %d graphs: worst |device - host| %.2e" % (len(pool), worst))
    items = _full_batch(cus, pool, seed=11)
    B = len(items)
    per_tier = [sum(1 for k, _, _ in items if k is not None and _tier_of(pool[k][1]) == t) for t in range(4)]
    print("B = %d on %d CUs, graphs per tier %s" % (B, cus, per_tier))
    assert B % 64 != 0 and per_tier[0] > 8 * cus and per_tier[1] > 2 * cus and per_tier[2] > cus and per_tier[3] > cus
    f1 = _check_batch(items, alone, "shuffled")
    f2 = _check_batch(items, alone, "shuffled, second run")
    assert _same_bits(f1, f2)
    _check_batch(items[::-1], alone, "reversed")


# ---- b. closed forms ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _closed_form_run():
    """the closed-form graphs and the random graphs of the t = 1000 limit, ONE batch, all eight times in one call -> cases, offsets,
    statuses, raw and normalised values (host arrays) and the packed tensors"""
    from tlc_gnn_amd import engine
    cases = [(name, n, e, f) for name, n, e, f in hks_closed_form_cases()]
    cases += [("random%d" % n, n, random_connected(n, 1000 + n), None) for n in HKS_CLOSED_FORM_SIZES]
    packed = _pack([(n, e) for _, n, e, _ in cases])
    raw, st = engine.hks_batch(packed[0], packed[1], packed[2], HKS_CLOSED_FORM_TIMES, normalise=False)
    nrm, st2 = engine.hks_batch(packed[0], packed[1], packed[2], HKS_CLOSED_FORM_TIMES, normalise=True)
    return cases, packed[3], st.cpu().numpy(), st2.cpu().numpy(), raw, nrm, packed


def test_closed_form_batch_converges_and_v_is_orthonormal():
    """Spectra with eigenvalues of multiplicity up to 255 (K256): every status TLC_ST_OK -- the sweeps stay inside TLC_HKS_MAX_SWEEPS --
    and the un-normalised values at t = 0, sum_k phi_k(x)^2, are 1."""
    from tlc_gnn_amd import _lib
    cases, nptr, st, st2, raw, _, _ = _closed_form_run()
    assert len(HKS_CLOSED_FORM_TIMES) == _lib.HKS_TMAX and HKS_CLOSED_FORM_TIMES[0] == 0.0
    bad = [(cases[k][0], int(st[k])) for k in range(len(cases)) if st[k] != _lib.ST_OK or st2[k] != _lib.ST_OK]
    assert not bad, bad
    d = np.abs(raw[0].cpu().numpy() - 1.0).max()
    print("worst |hks(t = 0) - 1| %.2e" % d)
    assert d <= hks_bound(0.0)


@pytest.mark.parametrize("family", ["complete", "star", "cycle", "bipartite"])
def test_closed_forms(family):
    """Un-normalised values against the closed form, normalised values against the closed form / (its max + 1e-10), at
    n = 2 .. 256 around every tier edge and t = 0 .. 1000: 1e-11 * max(1, t / 10)."""
    cases, nptr, st, _, raw, nrm, _ = _closed_form_run()
    raw, nrm = raw.cpu().numpy(), nrm.cpu().numpy()
    worst, seen = {t: 0.0 for t in HKS_CLOSED_FORM_TIMES}, 0
    fails = []
    for k, (name, n, e, f) in enumerate(cases):
        if not name.startswith(family):
            continue
        seen += 1
        for ti, t in enumerate(HKS_CLOSED_FORM_TIMES):
            ref = f(t)
            d = max(np.abs(raw[ti, nptr[k]:nptr[k + 1]] - ref).max(), np.abs(nrm[ti, nptr[k]:nptr[k + 1]] - ref / (ref.max() + 1e-10)).max())
            worst[t] = max(worst[t], d)
            if not d <= hks_bound(t):
                fails.append((name, t, d))
    print("%s, %d graphs: worst |device - closed form| per t: %s" % (family, seen, ", ".join("t=%g %.2e" % kv for kv in worst.items())))
    assert seen == len(HKS_CLOSED_FORM_SIZES) - (family == "cycle")
    assert not fails, fails


def test_long_time_limit_on_random_graphs():
    """t = 1000 on random connected graphs: deg(x) / (2m) within 1e-11 * 100 (un-normalised), and normalised accordingly."""
    cases, nptr, st, _, raw, nrm, _ = _closed_form_run()
    ti = HKS_CLOSED_FORM_TIMES.index(1000.0)
    raw, nrm = raw[ti].cpu().numpy(), nrm[ti].cpu().numpy()
    worst, seen = 0.0, 0
    for k, (name, n, e, f) in enumerate(cases):
        if f is None:
            ref = hks_stationary(n, e)
            d = max(np.abs(raw[nptr[k]:nptr[k + 1]] - ref).max(), np.abs(nrm[nptr[k]:nptr[k + 1]] - ref / (ref.max() + 1e-10)).max())
            worst, seen = max(worst, d), seen + 1
            assert d <= hks_bound(1000.0), (name, d)
    print("worst |device(t = 1000) - deg / 2m| %.2e over %d graphs" % (worst, seen))
    assert seen == len(HKS_CLOSED_FORM_SIZES)


def test_eight_times_in_one_call_equal_eight_calls():
    """n_times = TLC_HKS_TMAX: each row of the eight-time call has the bits of a single-time call, normalised or not."""
    from tlc_gnn_amd import engine
    _, _, _, _, raw, nrm, packed = _closed_form_run()
    for ti, t in enumerate(HKS_CLOSED_FORM_TIMES):
        for full, normalise in ((raw, False), (nrm, True)):
            single, _ = engine.hks_batch(packed[0], packed[1], packed[2], [t], normalise=normalise)
            assert _same_bits(single[0], full[ti]), (t, normalise)


# ---- c. graphs that are not connected -------------------------------------------------------------------------------------------------
def _components(sizes, seed):
    """disjoint union of random connected graphs of the given sizes (a size of 1 is an isolated node)"""
    es, off = [NO_EDGES], 0
    for i, s in enumerate(sizes):
        es.append(random_connected(s, seed + i) + off)
        off += s
    return off, np.concatenate(es)


def test_disconnected_graphs_and_isolated_nodes_against_host():
    """Components of sizes that put the union into every tier, isolated nodes between edges, and an isolated node as the LAST index
    of an odd n (next to the idle index of the Jacobi schedule): one batch, 1e-11 of the host route."""
    from tlc_gnn_amd import engine, _lib
    graphs = [(5, np.array([(0, 1), (3, 4)])), (3, np.array([(0, 1)])), (7, np.array([(0, 5), (1, 5), (2, 3)]))]
    graphs += [_components(s, 10 * k) for k, s in enumerate(((10, 10), (20, 30), (45, 45), (60, 61), (64, 64)))]
    graphs += [_components(s, 100 * k) for k, s in enumerate(((3, 5, 7, 9, 7), (12, 13, 13, 13, 13), (19, 19, 19, 19, 19), (25, 26, 25, 26, 26)))]
    graphs += [_components((s, 1), 50 + s) for s in (2, 32, 64, 96, 128)]                       # odd n, the last node isolated
    graphs += [_components((1, s, 1, 1), 60 + s) for s in (29, 62, 94)]
    node_ptr, edge_ptr, edges, nptr = _pack(graphs)
    f, st = engine.hks_batch(node_ptr, edge_ptr, edges, TIMES)
    assert st.cpu().tolist() == [_lib.ST_OK] * len(graphs)
    f, worst = f.cpu().numpy(), 0.0
    for k, (n, e) in enumerate(graphs):
        for ti, t in enumerate(TIMES):
            d = np.abs(f[ti, nptr[k]:nptr[k + 1]] - _host(n, e, t)).max()
            worst = max(worst, d)
            assert d <= 1e-11, (k, n, t, d)
    print("worst |device - host| %.2e over %d graphs, n = %s" % (worst, len(graphs), [n for n, _ in graphs]))
    assert np.abs(f[1, :5] - np.array([.5, .5, 1, .5, .5])).max() <= 2e-9                       # exp(-20) / 2 = 1.0e-9


def test_graphs_without_edges_without_nodes_and_the_empty_batch():
    """m = 0: un-normalised values exactly 1.0, normalised exactly 1 / (1 + 1e-10).  n = 0 as the only and as the last graph:
    TLC_ST_OK, nothing written.  B = 0: empty outputs."""
    import torch
    from tlc_gnn_amd import engine, _lib
    graphs = [(n, NO_EDGES) for n in (1, 2, 7, 33)] + [(6, random_connected(6, 1)), (0, NO_EDGES)]
    node_ptr, edge_ptr, edges, nptr = _pack(graphs)
    raw, st = engine.hks_batch(node_ptr, edge_ptr, edges, (0.0, 0.1, 10.0), normalise=False)
    nrm, st2 = engine.hks_batch(node_ptr, edge_ptr, edges, (0.0, 0.1, 10.0), normalise=True)
    assert st.cpu().tolist() == st2.cpu().tolist() == [_lib.ST_OK] * 6
    assert torch.equal(raw[:, :43], torch.ones((3, 43), dtype=torch.float64, device="cuda"))
    assert torch.equal(nrm[:, :43], torch.full((3, 43), 1.0 / (1.0 + 1e-10), dtype=torch.float64, device="cuda"))
    assert _same_bits(nrm[:, 43:], _alone(graphs[4], (0.0, 0.1, 10.0))[0])
    a = _pack([(0, NO_EDGES)])
    f, st = engine.hks_batch(a[0], a[1], a[2], TIMES)
    assert f.shape == (2, 0) and st.cpu().tolist() == [_lib.ST_OK]
    zero = torch.zeros(1, dtype=torch.int64, device="cuda")
    f, st = engine.hks_batch(zero, zero, torch.zeros((0, 2), dtype=torch.int32, device="cuda"), TIMES)
    assert f.shape == (2, 0) and st.shape == (0,)


# ---- d. refusals ----------------------------------------------------------------------------------------------------------------------
def _with_repeat(n, seed, flip):
    e = random_connected(n, seed)
    again = e[len(e) // 2:len(e) // 2 + 1]
    return n, np.concatenate([e, again[:, ::-1] if flip else again])


def test_bad_ids_and_repeated_edges_are_a_status():
    """An id equal to n on an odd graph (the idle index of the schedule) and on an even one, a negative id, and a repeated unordered
    pair in either orientation at sizes of every tier -- also the whole edge list in both directions, as PyG stores it: TLC_ST_BAD_INPUT,
    slice NaN; the neighbours bit-equal to their stand-alone values."""
    import torch
    from tlc_gnn_amd import engine, _lib
    good = [(9, random_connected(9, 5)), (40, random_connected(40, 6)), (70, random_connected(70, 7)), (100, random_connected(100, 8))]
    bad = [(5, np.array([(0, 1), (1, 5)])), (4, np.array([(0, 1), (1, 4)])), (33, np.concatenate([random_connected(33, 9), [(33, 2)]])),
           (6, np.array([(0, 1), (-1, 2)])), (4, np.concatenate([MULTI, MULTI[:1]])), (4, np.concatenate([MULTI, MULTI[:, ::-1]])),
           _with_repeat(20, 1, False), _with_repeat(31, 2, True), _with_repeat(50, 3, True), _with_repeat(64, 4, False),
           _with_repeat(90, 5, True), _with_repeat(120, 6, False), _with_repeat(255, 7, True), (2, np.array([(0, 1), (1, 0)]))]
    graphs, which = [], []                                             # which: index into `good`, None for a bad graph
    for k, b in enumerate(bad):
        graphs += [good[k % 4], b]
        which += [k % 4, None]
    graphs.append(good[0])
    which.append(0)
    is_bad = [w is None for w in which]
    node_ptr, edge_ptr, edges, nptr = _pack(graphs)
    f, st = engine.hks_batch(node_ptr, edge_ptr, edges, TIMES)
    assert st.cpu().tolist() == [_lib.ST_BAD_INPUT if b else _lib.ST_OK for b in is_bad]
    alone = [_alone(g)[0] for g in good]
    for k, g in enumerate(graphs):
        sl = f[:, nptr[k]:nptr[k + 1]]
        if is_bad[k]:
            assert bool(torch.isnan(sl).all()), k
        else:
            assert torch.equal(sl, alone[which[k]]), k


def test_offsets_out_of_order_or_beyond_the_totals_are_a_status():
    """edge_ptr [0, 5, 3, 8]: the middle graph's offsets run backwards (its neighbours' ranges overlap, every entry stays inside the
    buffers).  node_ptr[-1] above the total_nodes handed to the C ABI: the last graph lies beyond the totals.  TLC_ST_BAD_INPUT for
    that graph alone, the others bit-equal to their stand-alone values."""
    import torch
    from tlc_gnn_amd import engine, _lib
    e = np.array([(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (0, 1), (1, 2), (2, 3)], dtype=np.int32)
    node_ptr = torch.tensor([0, 6, 10, 16], dtype=torch.int64, device="cuda")
    edge_ptr = torch.tensor([0, 5, 3, 8], dtype=torch.int64, device="cuda")
    f, st = engine.hks_batch(node_ptr, edge_ptr, torch.from_numpy(e).cuda(), TIMES)
    assert st.cpu().tolist() == [_lib.ST_OK, _lib.ST_BAD_INPUT, _lib.ST_OK]
    assert torch.equal(f[:, :6], _alone((6, e[:5]))[0]) and torch.equal(f[:, 10:], _alone((6, e[3:8]))[0])
    assert bool(torch.isnan(f[:, 6:10]).all())
    # node_ptr [0, 3, 7], total_nodes = 3: the output has room for all 7 nodes per row all the same
    L = _lib.lib()
    node_ptr, edge_ptr, edges, _ = _pack([(3, np.array([(0, 1), (1, 2)])), (4, MULTI)])
    need = C.c_int64(0)
    assert L.tlc_hks_batch_work_bytes(2, 3, 6, 1, C.byref(need)) == 0
    out = torch.full((1, 7), float("nan"), dtype=torch.float64, device="cuda")
    st = torch.zeros(2, dtype=torch.uint8, device="cuda")
    work = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    rc = L.tlc_hks_batch(_lib.ptr(node_ptr), _lib.ptr(edge_ptr), _lib.ptr(edges), 2, 3, 6, (C.c_double * 1)(0.1), 1, _lib.HKS_NORMALISE,
                         _lib.ptr(out), _lib.ptr(st), _lib.ptr(work), need.value, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and st.cpu().tolist() == [_lib.ST_OK, _lib.ST_BAD_INPUT]
    assert torch.equal(out[:, :3], _alone((3, np.array([(0, 1), (1, 2)])), [0.1])[0]) and bool(torch.isnan(out[:, 3:]).all())


# ---- e. wrapper branches --------------------------------------------------------------------------------------------------------------
def test_wrapper_not_converged_takes_the_host_route_and_bad_input_raises(monkeypatch):
    """`engine.hks_batch` doctored to report one graph TLC_ST_NOT_CONVERGED with a NaN slice: `hks_filtration_device` returns the
    host values for it bit for bit, the others as they were, hks_host_fallback == 1.  TLC_ST_BAD_INPUT instead: RuntimeError."""
    import torch
    from tlc_gnn_amd import engine, _lib
    from tlc_gnn_amd.Knowledge_Distillation import data_utils_LP as kd_lp
    graphs = [(12, random_connected(12, 1)), (40, random_connected(40, 2)), (7, random_connected(7, 3))]
    node_ptr, edge_ptr, edges, nptr = _pack(graphs)
    real = engine.hks_batch
    true_f = kd_lp.hks_filtration_device(node_ptr, edge_ptr, edges, 10.0, int(nptr[-1])).clone()
    assert kd_lp.hks_host_fallback == 0

    def doctored(code):
        def fake(*args, **kwargs):
            f, st = real(*args, **kwargs)
            f[:, nptr[1]:nptr[2]] = float("nan")
            st[1] = code
            return f, st
        return fake
    assert kd_lp.engine is engine
    monkeypatch.setattr(kd_lp.engine, "hks_batch", doctored(_lib.ST_NOT_CONVERGED))
    out = kd_lp.hks_filtration_device(node_ptr, edge_ptr, edges, 10.0, int(nptr[-1]))
    assert kd_lp.hks_host_fallback == 1
    assert np.array_equal(out[nptr[1]:nptr[2]].cpu().numpy(), _host(40, graphs[1][1], 10.0))
    assert torch.equal(out[:nptr[1]], true_f[:nptr[1]]) and torch.equal(out[nptr[2]:], true_f[nptr[2]:])
    monkeypatch.setattr(kd_lp.engine, "hks_batch", doctored(_lib.ST_BAD_INPUT))
    with pytest.raises(RuntimeError, match="repeated"):
        kd_lp.hks_filtration_device(node_ptr, edge_ptr, edges, 10.0, int(nptr[-1]))
    monkeypatch.setattr(kd_lp.engine, "hks_batch", real)
    kd_lp.hks_filtration_device(node_ptr, edge_ptr, edges, 10.0, int(nptr[-1]))
    assert kd_lp.hks_host_fallback == 0


def test_gc_drop_ins_refuse_repeated_edges_on_the_device_route():
    """A caller's (n, edges) tuple with every edge in both directions, or with one edge twice: hks_backend='device' raises (it never
    returns values that differ from the host route's); 'host' keeps scipy's multigraph semantics -- both directions is the simple
    graph -- and the simple graph agrees between the two backends."""
    from tlc_gnn_amd.Knowledge_Distillation import data_utils_GC as kd_gc
    both, once_more = np.concatenate([MULTI, MULTI[:, ::-1]]), np.concatenate([MULTI, MULTI[:1]])
    for t in TIMES:
        for e in (both, once_more):
            with pytest.raises(RuntimeError, match="repeated"):
                kd_gc.compute_persistence_image((4, e), filt='hks', hks_time=t, mode='filtration', hks_backend='device')
            with pytest.raises(RuntimeError, match="repeated"):
                kd_gc.compute_persistence_image((4, e), filt='hks', hks_time=t, mode='PI', hks_backend='device')
            with pytest.raises(RuntimeError, match="repeated"):
                kd_gc.compute_persistence_image_batch([(4, MULTI), (4, e)], filt='hks', hks_time=t, hks_backend='device')
        dev = kd_gc.compute_persistence_image((4, MULTI), filt='hks', hks_time=t, mode='filtration', hks_backend='device')[0]
        host = kd_gc.compute_persistence_image((4, MULTI), filt='hks', hks_time=t, mode='filtration', hks_backend='host')[0]
        host_both = kd_gc.compute_persistence_image((4, both), filt='hks', hks_time=t, mode='filtration', hks_backend='host')[0]
        host_more = kd_gc.compute_persistence_image((4, once_more), filt='hks', hks_time=t, mode='filtration', hks_backend='host')[0]
        assert np.abs(np.array(dev) - np.array(host)).max() <= 1e-11
        assert np.abs(np.array(host_both) - np.array(host)).max() <= 1e-12
        assert np.abs(np.array(host_more) - np.array(host)).max() > 1e-4

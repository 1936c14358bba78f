"""GPU: vicinity images differentiable in the graph's edge weights (csrc/vic_grad.hip, topo.VicinityImages, pipelines.train_curvature)
against the numpy restatements of tests/vic_grad_cases.py, the vicinity pipeline itself and torch's autograd.  Integer outputs and
fp64 sums are compared bit for bit; every other bound is stated where it is used."""
import ctypes as C
import functools

import numpy as np
import pytest

import dist_filt_cases as dc
import vic_grad_cases as vc

pytestmark = pytest.mark.gpu


def _cuda(*arrays):
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def _hk():
    """The 300-node Holme-Kim graph of the LP tests with a generic curvature in (-0.5, 0.9): (n, edges int32[900, 2], kappa)"""
    from tlc_gnn_amd import synth
    n = 300
    ge = synth.holme_kim_edges(n, 900, triad_p=0.5, seed=5).astype(np.int32)
    kappa = np.random.default_rng(17).uniform(-0.5, 0.9, len(ge))
    return n, ge, kappa


def _device_graph(n, ge, kappa):
    from tlc_gnn_amd import engine, synth
    return engine.DeviceGraph(*synth.edges_to_csr(n, ge, kappa))


def _packed(g, pairs, hop, flags):
    """The packed batch of the pairs with exact offsets -> dict of CUDA tensors (ids int32), f and status included"""
    from tlc_gnn_amd import engine
    n0, m0 = g.vicinity_sizes(pairs, hop, flags=flags)
    node_ptr, edge_ptr, totals = engine.pack_offsets(n0, m0)
    _, _, tot_n, tot_m = totals.tolist()
    _, ids, f, _, st, _, edges, _ = g.vicinity_filtration(pairs, hop, flags=flags, zero=False, offsets=(node_ptr, edge_ptr, tot_n, tot_m))
    return dict(node_ptr=node_ptr, edge_ptr=edge_ptr, ids=ids[:tot_n], f=f[:tot_n], edges=edges[:tot_m], status=st)


def _mixed_pairs(n, ge, count, seed):
    """edges of the graph, random pairs that are mostly no edges, a pair (u, u), and a pair as far apart as the graph has"""
    rs = np.random.RandomState(seed)
    import collections
    adj = collections.defaultdict(list)
    for a, b in ge:
        adj[int(a)].append(int(b))
        adj[int(b)].append(int(a))
    dist = {0: 0}
    queue = collections.deque([0])
    while queue:
        x = queue.popleft()
        for y in adj[x]:
            if y not in dist:
                dist[y] = dist[x] + 1
                queue.append(y)
    far = max(dist, key=dist.get)
    assert dist[far] >= 3
    k = count * 3 // 4
    pairs = np.concatenate([ge[rs.permutation(len(ge))[:k]], rs.randint(0, n, size=(count - k - 2, 2)), [[7, 7]], [[0, far]]])
    return pairs.astype(np.int32)


# ---- lookup ------------------------------------------------------------------------------------------------------------------------------
def test_lookup_equals_the_restatement_on_hop2_vicinities():
    import torch
    from tlc_gnn_amd import engine
    from tlc_gnn_amd.Knowledge_Distillation import data_utils_LP as kd_lp
    n, ge, kappa = _hk()
    g = _device_graph(n, ge, kappa)
    pairs = ge[np.random.RandomState(3).permutation(len(ge))[:256]]
    ge_d, pairs_d = _cuda(ge, pairs)
    b = _packed(g, pairs_d, 2, kd_lp.KD_LP_FLAGS)
    host = [b[k].cpu().numpy() for k in ("node_ptr", "edge_ptr", "ids", "edges")]
    assert not b["status"].any() and int(host[1][-1]) > 256
    want = vc.lookup(ge, *host, pairs)
    assert not want[2].any()
    for ids in (b["ids"], b["ids"].to(torch.int64)):                           # both id widths the packers return
        eid, roots, st = engine.packed_edge_lookup(ge_d, b["node_ptr"], b["edge_ptr"], ids, b["edges"], pairs=pairs_d)
        assert np.array_equal(eid.cpu().numpy(), want[0]) and np.array_equal(roots.cpu().numpy(), want[1]) and not st.any()
    eid, roots, st = engine.packed_edge_lookup(ge_d, b["node_ptr"], b["edge_ptr"], b["ids"], b["edges"])       # no pair list: no roots
    assert roots is None and np.array_equal(eid.cpu().numpy(), want[0]) and not st.any()
    # u == v with the one-root flag: the node vicinities of the PDGNN fork
    nodes = np.random.RandomState(4).choice(n, 64, replace=False).astype(np.int32)
    uu = np.stack([nodes, nodes], 1)
    uu_d, = _cuda(uu)
    b1 = _packed(g, uu_d, 2, kd_lp.KD_LP_FLAGS | 0xC0)
    host1 = [b1[k].cpu().numpy() for k in ("node_ptr", "edge_ptr", "ids", "edges")]
    eid, roots, st = engine.packed_edge_lookup(ge_d, b1["node_ptr"], b1["edge_ptr"], b1["ids"], b1["edges"], pairs=uu_d, one_root=True)
    want1 = vc.lookup(ge, *host1, uu, one_root=True)
    assert np.array_equal(eid.cpu().numpy(), want1[0]) and np.array_equal(roots.cpu().numpy(), want1[1]) and not st.any()
    assert (roots[:, 1] == -1).all() and (roots[:, 0] >= 0).all()
    g.close()


def test_lookup_edge_cases_by_hand():
    """M = 1; the first and the last edge of the list; a vicinity with an edge that is not in the list between two good ones; B = 0"""
    import torch
    from tlc_gnn_amd import engine
    one = np.array([[0, 1]], np.int32)
    eid, roots, st = engine.packed_edge_lookup(*_cuda(one, np.array([0, 2]), np.array([0, 1]), np.array([0, 1], np.int32), one, one))
    assert eid.tolist() == [0] and roots.tolist() == [[0, 1]] and st.tolist() == [0]
    n, ge, _ = _hk()
    present = set(map(tuple, ge.tolist()))
    a, b = next((a, b) for a in range(n) for b in range(a + 1, n) if (a, b) not in present)
    ids = np.array([ge[0, 0], ge[0, 1], a, b, ge[-1, 0], ge[-1, 1]], np.int64)
    node_ptr, edge_ptr = np.array([0, 2, 4, 6]), np.array([0, 1, 2, 3])
    edges = np.array([[0, 1]] * 3, np.int32)
    pairs = np.array([ge[0][::-1], [a, b], ge[-1]], np.int32)                  # (the first pair the other way round: roots follow the pair)
    eid, roots, st = engine.packed_edge_lookup(*_cuda(ge, node_ptr, edge_ptr, ids, edges, pairs))
    assert eid.tolist() == [0, -1, len(ge) - 1] and roots.tolist() == [[1, 0], [-1, -1], [0, 1]] and st.tolist() == [0, vc.ST_BAD_INPUT, 0]
    want = vc.lookup(ge, node_ptr, edge_ptr, ids, edges, pairs)
    assert np.array_equal(eid.cpu().numpy(), want[0]) and np.array_equal(roots.cpu().numpy(), want[1]) and np.array_equal(st.cpu().numpy(), want[2])
    # a root that is not in its vicinity refuses it too, and a local id outside the vicinity
    pairs2 = pairs.copy()
    pairs2[2, 1] = a
    edges2 = edges.copy()
    edges2[0, 1] = 2
    eid, roots, st = engine.packed_edge_lookup(*_cuda(ge, node_ptr, edge_ptr, ids, edges2, pairs2))
    assert eid.tolist() == [-1, -1, -1] and (roots == -1).all() and st.tolist() == [vc.ST_BAD_INPUT] * 3
    # B = 0
    z = torch.zeros(1, dtype=torch.int64, device="cuda")
    eid, roots, st = engine.packed_edge_lookup(_cuda(ge)[0], z, z, torch.zeros(0, dtype=torch.int64, device="cuda"),
                                               torch.zeros((0, 2), dtype=torch.int32, device="cuda"),
                                               pairs=torch.zeros((0, 2), dtype=torch.int32, device="cuda"))
    assert eid.numel() == 0 and roots.shape == (0, 2) and st.numel() == 0


def test_refusals_on_the_device():
    import torch
    from tlc_gnn_amd import _lib
    L = _lib.lib()
    t = torch.zeros(1024, dtype=torch.int64, device="cuda")
    p, s = C.c_void_p(t.data_ptr()), _lib.stream_ptr()
    assert L.tlc_packed_edge_lookup(1, None, 1, p, p, p, 1, p, 2, 1, None, 0, p, None, p, s) == 1
    assert L.tlc_packed_edge_lookup(1, p, 1, p, p, p, 1, p, 2, 1, p, 0, p, None, p, s) == 1
    assert L.tlc_packed_edge_lookup(1, p, -1, p, p, p, 1, p, 2, 1, None, 0, p, None, p, s) == 1
    assert L.tlc_segment_index(4, p, 4, p, p, p, 8, s) == 1 and L.tlc_segment_index(4, p, 4, None, p, p, 1 << 20, s) == 1
    assert L.tlc_segment_sum_f64(4, p, p, 4, p, p, p, 8, s) == 1 and L.tlc_segment_sum_f64(4, p, p, 4, None, p, p, 1 << 20, s) == 1
    assert L.tlc_segment_sum_f64(4, p, p, 4, p, p, C.c_void_p(t.data_ptr() + 8), 1 << 12, s) == 1
    assert L.tlc_lp_decode_bwd_pi_f32(1, p, p, p, 4, 8, p, 25, p, p, p, p, p, p, s) == 4
    assert L.tlc_lp_decode_bwd_pi_f32(1, p, p, p, 4, 16, p, 25, p, p, p, p, p, None, s) == 1
    torch.cuda.synchronize()


# ---- segment index and sum -----------------------------------------------------------------------------------------------------------------
def _values(rng, n):
    """normal values with ties (a few distinct magnitudes), -0.0 and cancelling pairs"""
    v = rng.normal(size=n) * 10.0 ** rng.integers(-2, 3, size=n)
    v[rng.random(n) < 0.05] = -0.0
    tie = rng.random(n) < 0.1
    v[tie] = np.round(v[tie])
    half = n // 20
    where = rng.permutation(n)[:2 * half]
    v[where[half:]] = -v[where[:half]]
    return v


def _keys_for(lengths, rng, skipped):
    """item keys with lengths[k] items of key k and `skipped` negative ones, in random order"""
    key = np.concatenate([np.repeat(np.arange(len(lengths)), lengths), -1 - rng.integers(0, 3, size=skipped)]).astype(np.int32)
    return key[rng.permutation(len(key))]


def _check_index_and_sum(lengths, seed, skipped=100):
    import torch
    from tlc_gnn_amd import engine
    rng = np.random.default_rng(seed)
    key = _keys_for(np.asarray(lengths), rng, skipped)
    M = len(lengths)
    val = _values(rng, len(key))
    key_d, val_d = _cuda(key, val)
    seg_ptr, seg_pos = engine.segment_index(key_d, M)
    want_ptr, want_pos = vc.segment_index(key, M)
    assert np.array_equal(seg_ptr.cpu().numpy(), want_ptr) and np.array_equal(seg_pos.cpu().numpy(), want_pos)
    assert np.array_equal(np.diff(want_ptr), lengths)
    again = engine.segment_index(key_d, M)
    assert torch.equal(again[0], seg_ptr) and torch.equal(again[1], seg_pos)
    want = vc.segment_sum(val, want_ptr, want_pos)
    least = torch.empty(engine.segment_sum_work_bytes(M) + 255, dtype=torch.uint8, device="cuda")
    roomy = torch.full((3 * engine.segment_sum_work_bytes(M) + 4096 + 77,), 0x5A, dtype=torch.uint8, device="cuda")[77:]
    outs = [engine.segment_sum(val_d, seg_ptr, seg_pos, work=w).cpu().numpy() for w in (least, roomy, None, least)]
    for o in outs:
        assert np.array_equal(_bits(o), _bits(want))
    return want, np.diff(want_ptr)


def test_segment_sum_at_the_cuts_and_one_long_key_among_short_ones():
    """Lengths 0, 1 and each cut - 1, at, + 1; one key with 70 000 items among 5 000 short segments (two radix digits: M < 2^16);
    -0.0, ties and cancelling pairs among the values; negative keys skipped; the least workspace, a roomy one, run against run."""
    rng = np.random.default_rng(5)
    short = rng.integers(0, 6, size=5000)
    cuts = [0, 1, vc.LANE_MAX - 1, vc.LANE_MAX, vc.LANE_MAX + 1, vc.WAVE_MAX - 1, vc.WAVE_MAX, vc.WAVE_MAX + 1]
    lengths = np.concatenate([short[:2500], [70000], short[2500:], cuts, [0]])
    want, L = _check_index_and_sum(lengths, 6)
    empty = L == 0
    assert empty.any() and (_bits(want[empty]) == 0).all()                    # an empty segment is +0.0
    # all -0.0 and a cancelling pair end as +0.0 in every class
    import torch
    from tlc_gnn_amd import engine
    for Lz in (1, 16, 17, 2048, 2049):
        key = torch.zeros(Lz, dtype=torch.int32, device="cuda")
        ptr, pos = engine.segment_index(key, 1)
        out = engine.segment_sum(torch.full((Lz,), -0.0, dtype=torch.float64, device="cuda"), ptr, pos)
        assert _bits(out.cpu().numpy())[0] == 0, Lz


def test_segment_sum_with_more_segments_than_any_grid():
    """1.1 million keys (four radix digits; more than the 4 096 x 256 threads of the first kernel), of which 33 000 are of the wavefront
    class (more than its 8 192 x 4 wavefronts) and 2 060 of the workgroup class (more than its 2 048 workgroups): every grid-stride
    loop goes round"""
    rng = np.random.default_rng(8)
    M = 1_100_000
    lengths = rng.integers(0, 3, size=M)
    where = rng.permutation(M)
    lengths[where[:33000]] = rng.integers(vc.LANE_MAX + 1, 41, size=33000)
    lengths[where[33000:35060]] = rng.integers(vc.WAVE_MAX + 1, 2101, size=2060)
    _check_index_and_sum(lengths, 9, skipped=1000)


def test_segment_sum_error_against_fsum_on_the_device():
    """the device's sums (not only the restatement's) within L * 2^-53 * sum |v| of the exact sum"""
    import math
    from tlc_gnn_amd import engine
    rng = np.random.default_rng(12)
    lengths = np.array([3, 16, 17, 500, 2048, 2049, 9000])
    key = _keys_for(lengths, rng, 10)
    val = _values(rng, len(key))
    key_d, val_d = _cuda(key, val)
    ptr, pos = engine.segment_index(key_d, len(lengths))
    out = engine.segment_sum(val_d, ptr, pos).cpu().numpy()
    for k, L in enumerate(lengths):
        v = val[key == k]
        assert abs(out[k] - math.fsum(v)) <= L * 2.0 ** -53 * np.abs(v).sum(), k


# ---- the decoder's d PI ------------------------------------------------------------------------------------------------------------------
def _decode_ref(emb, pairs, pi, w1, b1, w2, b2):
    """TLCGNN.py:48-61 after the renorm, with autograd (the restatement of tests/test_gpu_lp_train.py)"""
    import torch
    import torch.nn.functional as F
    a, b = emb[pairs[:, 0].long()], emb[pairs[:, 1].long()]
    h = F.leaky_relu(F.linear(torch.cat(((a - b).pow(2), pi.to(emb.dtype)), dim=1), w1, b1), 0.2)
    d = torch.clamp(torch.abs(F.linear(h, w2, b2)).reshape(-1), min=0, max=40)
    return 1.0 / (torch.exp((d - 2.0) / 1.0) + 1.0)


def _close(got, want, rtol=1e-4, atol_frac=2e-5):
    """the bound of test_decode_backward_matches_autograd_f64 for d emb: the same f32 chain"""
    import torch
    atol = atol_frac * float(want.abs().max())
    err = float((got.to(want.dtype) - want).abs().max())
    return torch.allclose(got.to(want.dtype), want, rtol=rtol, atol=atol), err, atol


def test_decoder_d_pi_matches_autograd_f64():
    import torch
    from tlc_gnn_amd import autograd, engine, ops
    t = {k: v for k, v in zip(vc.decode_data(), _cuda(*vc.decode_data().values()))}
    post = ops.renorm_rows_(t["emb"].clone())
    args = (t["pairs"], t["emb"], post, t["pi"], t["w1"], t["b1"], t["w2"], t["b2"], t["g"])
    got = engine.lp_decode_bwd_pi(*args)
    assert got.shape == (700, 25) and got.dtype == torch.float32 and torch.equal(got, engine.lp_decode_bwd_pi(*args))
    r = {k: t[k].double() for k in ("w1", "b1", "w2", "b2")}
    pi64 = t["pi"].double().requires_grad_(True)
    prob = _decode_ref(post.double(), t["pairs"], pi64, r["w1"], r["b1"], r["w2"], r["b2"])
    with torch.no_grad():                                                       # the cases the data is built to hold
        a, b = post.double()[t["pairs"][:, 0].long()], post.double()[t["pairs"][:, 1].long()]
        h = torch.cat(((a - b).pow(2), pi64), 1) @ r["w1"].t() + r["b1"]
        d = (torch.nn.functional.leaky_relu(h, 0.2) @ r["w2"].t() + r["b2"]).reshape(-1)
        assert bool((h < 0).any()) and bool((h > 0).any()) and bool((d.abs() > 40.01).any()) and int((d == 0).sum()) >= 10
        assert bool((t["pairs"][:50] == t["pairs"][50:100]).all()) and bool((t["pairs"][100:130, 0] == t["pairs"][100:130, 1]).all())
    prob.backward(t["g"].double())
    ok, err, atol = _close(got, pi64.grad)
    print("d PI: max |err| %.3e, atol %.3e, max |want| %.3e" % (err, atol, float(pi64.grad.abs().max())))
    assert ok, (err, atol)
    assert bool((got[(d.abs() > 40.01) | (d == 0)] == 0).all())                 # beyond the clamp, and at d == 0: no gradient
    # the f32 restatement of the formula: the same chain in another summation order
    want32 = vc.decode_dpi(vc.decode_gz(post.cpu().numpy(), *(t[k].cpu().numpy() for k in ("pairs", "pi", "w1", "b1", "w2", "b2", "g"))),
                           t["w1"].cpu().numpy())
    assert _close(got, torch.from_numpy(want32).cuda().double())[0]
    # LpDecode: the other five gradients do not depend on whether pi wants one
    grads = []
    for need in (False, True):
        leaves = [t[k].clone().requires_grad_(True) for k in ("emb", "w1", "b1", "w2", "b2")]
        pi = t["pi"].clone().requires_grad_(need)
        autograd.lp_decode(leaves[0], t["pairs"], pi, *leaves[1:]).backward(t["g"])
        grads.append([x.grad for x in leaves] + [pi.grad])
    assert all(torch.equal(a, b) for a, b in zip(grads[0][:5], grads[1][:5]))
    assert grads[0][5] is None and torch.equal(grads[1][5], got)
    pi64in = t["pi"].double().requires_grad_(True)                              # a float64 table gets a float64 gradient
    autograd.lp_decode(t["emb"], t["pairs"], pi64in, t["w1"], t["b1"], t["w2"], t["b2"]).backward(t["g"])
    assert pi64in.grad.dtype == torch.float64 and torch.equal(pi64in.grad, got.double())


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["plain", "kd_lp"])
def test_module_equals_the_vicinity_pipeline(which):
    """200 pairs at hop 2 -- edges, pairs that are no edges, (u, u), a far pair: the module's filtration == tlc_vicinity_filtration's f,
    its images within 1e-12 of tlc_pd_pi_batch's rows (the bound of tests/test_gpu_extract.py between two routes to one image: the
    points arrive in another order under equal keys), its status bytes == that batch's.

    Two of the 'kd_lp' rows are vicinities that are not connected, which only TLC_UNREACHABLE_100 lets through: one component that
    holds every edge (11 nodes, 13 edges, three cycles; 6 nodes, 6 edges, one cycle) beside three / one isolated nodes, so m == n - 1
    without the vicinity being a tree.  The batch kernels took every such vicinity for a tree and left its Ext1 points out (6.3e-05 and
    1.2e-05 of image); pd_all_stages now keeps that shortcut to batches without TLC_UNREACHABLE_100
    (test_batch_equals_the_oracle_on_vicinities_with_isolated_nodes)."""
    import torch
    from tlc_gnn_amd import _lib, topo
    from tlc_gnn_amd.Knowledge_Distillation import data_utils_LP as kd_lp
    flags = 0 if which == "plain" else kd_lp.KD_LP_FLAGS
    n, ge, kappa = _hk()
    pairs = _mixed_pairs(n, ge, 200, 21)
    mod = topo.VicinityImages(n, ge, pairs, 2, flags=flags)
    S = mod.structure
    kap, pairs_d = _cuda(kappa, pairs)
    g = _device_graph(n, ge, kappa)
    want_img, want_st = g.pd_pi_batch(pairs_d, 2, flags=flags)
    img, st = mod(kap)
    b = _packed(g, pairs_d[S.rows].contiguous(), 2, flags)
    f = topo.vicinity_filtration_of(kap, S)
    row_err = (img - want_img).abs().max(1).values
    worst = int(row_err.argmax())
    print("%s: %d of 200 rows computed, status counts %s / %s, max |image diff| %.3e at pair %d %s, filtration equal: %s"
          % (which, S.rows.numel(), torch.bincount(st.long(), minlength=8).tolist(), torch.bincount(want_st.long(), minlength=8).tolist(),
             float(row_err.max()), worst, pairs[worst].tolist(), bool(torch.equal(f, b["f"]))))
    assert torch.equal(st, want_st)
    assert float(row_err.max()) <= 1e-12 and S.rows.numel() >= 100
    off = torch.ones(200, dtype=torch.bool, device="cuda")
    off[S.rows] = False
    assert bool((img[off] == 0).all()) and bool((want_img[off] == 0).all()) and bool((st[S.rows] == _lib.ST_OK).all())
    assert bool((img[S.rows].abs().sum(1) > 0).all())
    assert torch.equal(b["node_ptr"], S.node_ptr) and torch.equal(b["edges"], S.edges)
    assert torch.equal(f, b["f"])
    g.close()


def test_module_equals_the_oracle_under_kd_flags():
    """The same 200 pairs under KD_LP_FLAGS against the CPU oracle's pd_pi_batch: status bytes equal, every image within 1e-12 --
    the vicinities that are not connected included (measured: 1.1e-15)."""
    import torch
    from oracle import oracle
    from tlc_gnn_amd import synth, topo
    from tlc_gnn_amd.Knowledge_Distillation import data_utils_LP as kd_lp
    n, ge, kappa = _hk()
    pairs = _mixed_pairs(n, ge, 200, 21)
    mod = topo.VicinityImages(n, ge, pairs, 2, flags=kd_lp.KD_LP_FLAGS)
    img, st = mod(_cuda(kappa)[0])
    ref, rst, _ = oracle.pd_pi_batch(*synth.edges_to_csr(n, ge, kappa), pairs, 2, flags=kd_lp.KD_LP_FLAGS, n_threads=0)
    err = float(np.abs(img.cpu().numpy() - ref).max())
    print("module against the oracle under KD_LP_FLAGS: max |image diff| %.3e" % err)
    assert np.array_equal(st.cpu().numpy(), rst) and err <= 1e-12


def test_batch_equals_the_oracle_on_vicinities_with_isolated_nodes():
    """tlc_pd_pi_batch under KD_LP_FLAGS on the same 200 pairs against the CPU oracle, the bound of the batch's other oracle tests
    (status bytes and zero pattern equal, 1e-8 relative): two of the vicinities have n - 1 edges and are no trees -- a component with
    cycles beside isolated nodes -- and their Ext1 points used to be left out (6e-3 relative)."""
    from oracle import oracle
    from tlc_gnn_amd import synth
    from tlc_gnn_amd.Knowledge_Distillation import data_utils_LP as kd_lp
    n, ge, kappa = _hk()
    pairs = _mixed_pairs(n, ge, 200, 21)
    g = _device_graph(n, ge, kappa)
    b = _packed(g, _cuda(pairs)[0], 2, kd_lp.KD_LP_FLAGS)
    nn, mm = (b[k][1:] - b[k][:-1] for k in ("node_ptr", "edge_ptr"))
    assert int(((mm == nn - 1) & (nn >= 2)).sum()) >= 2
    out, st = g.pd_pi_batch(_cuda(pairs)[0], 2, flags=kd_lp.KD_LP_FLAGS)
    g.close()
    ref, rst, _ = oracle.pd_pi_batch(*synth.edges_to_csr(n, ge, kappa), pairs, 2, flags=kd_lp.KD_LP_FLAGS, n_threads=0)
    out = out.cpu().numpy()
    assert np.array_equal(st.cpu().numpy(), rst) and np.array_equal(out == 0, ref == 0)
    nz = ref != 0
    assert (np.abs(out[nz] - ref[nz]) / np.abs(ref[nz])).max() < 1e-8


@functools.lru_cache(maxsize=None)
def _small():
    """16 nodes, 24 edges, generic weights, 6 pairs (five edges and one pair two steps apart)"""
    rng = np.random.default_rng(31)
    n = 16
    ge = np.unique(np.sort(dc.random_connected(rng, n, 24), 1), axis=0).astype(np.int32)
    kappa = dc.generic_weights(rng, len(ge)) - 1.0
    present = set(map(tuple, ge.tolist()))
    two = next((a, c) for a, b in ge.tolist() for b2, c in ge.tolist() if b == b2 and a < c and (a, c) not in present)
    pairs = np.concatenate([ge[[0, 5, 9, 14, 20]], [two]]).astype(np.int32)
    return n, ge, kappa, pairs


def test_gradcheck_through_the_whole_module():
    """torch.autograd.gradcheck at its fp64 defaults, grad='full', a pimg imager.  The data is generic: inside every vicinity the path
    lengths to each root and the filtration values off the roots are pairwise distinct (asserted below with a margin far above the
    finite-difference step), so the trees and the critical vertices stay put under the perturbation."""
    import torch
    from tlc_gnn_amd import topo
    from tlc_gnn_amd.Knowledge_Distillation import pimg
    n, ge, kappa, pairs = _small()
    im = pimg.PersistenceImager(resolution=6, kernel_params={"sigma": 0.05})
    mod = topo.VicinityImages(n, ge, pairs, 2, flags=0, imager=im, grad="full")
    S = mod.structure
    assert S.rows.numel() == 6 and S.columns == 36
    kap, = _cuda(kappa)
    f = topo.vicinity_filtration_of(kap, S).cpu().numpy()
    w = (kap + 1.0)[S.eid.long()]
    one = torch.full_like(S.roots[:, 0], -1)
    D = [topo.distance_filtration(w, S.node_ptr, S.edge_ptr, S.edges, roots=torch.stack([S.roots[:, r], one], 1).contiguous(),
                                  norm="none").cpu().numpy() for r in (0, 1)]
    no, roots = S.node_ptr.cpu().numpy(), S.roots.cpu().numpy()
    for k in range(6):
        sl = slice(no[k], no[k + 1])
        inner = np.delete(f[sl], roots[k])                                      # (both roots sit at 0: constants, no derivative)
        assert len(inner) >= 2 and np.diff(np.sort(inner)).min() > 1e-4 and inner.min() > 1e-4, k
        assert np.diff(np.sort(D[0][sl])).min() > 1e-4 and np.diff(np.sort(D[1][sl])).min() > 1e-4, k
    x = kap.clone().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda z: mod(z)[0], (x,))
    img, _ = mod(x)
    assert float(img.abs().sum()) > 0


def test_weight_gradient_equals_the_composition_with_a_sequential_scatter():
    """grad='weight' on the 300-node graph: kappa.grad through the module == the same composition cut at the packed weights, whose
    gradient is then summed per graph edge by the numpy restatement in the header's order.  Bit for bit."""
    import torch
    from tlc_gnn_amd import topo
    n, ge, kappa = _hk()
    pairs = _mixed_pairs(n, ge, 200, 22)
    mod = topo.VicinityImages(n, ge, pairs, 2, flags=0, grad="weight")
    S = mod.structure
    kap, = _cuda(kappa)
    G = torch.from_numpy(np.random.default_rng(2).normal(size=(200, 25))).cuda()
    x = kap.clone().requires_grad_(True)
    (mod(x)[0] * G).sum().backward()
    w = (kap + 1.0)[S.eid.long()].clone().requires_grad_(True)
    f = topo.distance_filtration(w, S.node_ptr, S.edge_ptr, S.edges, roots=S.roots, **S.opts)
    img = topo.images(f, S.node_ptr, S.edge_ptr, S.edges, which=S.which, res=5, grad="weight")
    (img * G[S.rows]).sum().backward()
    want = vc.segment_sum(w.grad.cpu().numpy(), S.seg_ptr.cpu().numpy(), S.seg_pos.cpu().numpy())
    assert np.abs(want).max() > 0 and np.array_equal(_bits(x.grad.cpu().numpy()), _bits(want))
    # against index_add_ (floating-point atomics): within L * 2^-52 * sum |g| per edge
    ref = torch.zeros_like(kap).index_add_(0, S.eid.long(), w.grad)
    bound = torch.zeros_like(kap).index_add_(0, S.eid.long(), w.grad.abs()) * float(np.diff(S.seg_ptr.cpu().numpy()).max()) * 2.0 ** -52
    assert bool(((x.grad - ref).abs() <= bound).all())


class _Tap:
    """`images` for train_curvature that keeps the table of the last call (and its gradient)"""

    def __init__(self, images):
        self.images, self.structure, self.kappa, self.table = images, images.structure, images.kappa, None

    def __call__(self):
        self.table, st = self.images()
        self.table.retain_grad()
        return self.table, st


def _lp_setup(torch, tp=60, tn=80, seed=3):
    """the 300-node graph as a link-prediction problem whose image table is learned: tp positives (edges) and tn negatives"""
    from tlc_gnn_amd import pipelines, synth, topo
    from tlc_gnn_amd.baselines import TLCGNN
    from tlc_gnn_amd.data import Data
    n, ge, kappa = _hk()
    rs = np.random.RandomState(seed)
    pos = ge[rs.permutation(len(ge))[:tp]]
    neg = rs.randint(0, n, size=(tn, 2))
    pairs = np.concatenate([pos, neg]).astype(np.int64)
    y = torch.from_numpy(np.concatenate([np.ones(tp, np.int64), np.zeros(tn, np.int64)]))
    ei = torch.from_numpy(np.concatenate([ge, ge[:, ::-1]]).T.copy()).long()
    data = Data(x=torch.from_numpy(synth.synthetic_features(n, 48, seed=5)), edge_index=ei, y=torch.zeros(n), total_edges=pairs, total_edges_y=y,
                train_pos=tp, train_neg=tn, val_pos=0, val_neg=0, test_pos=0, test_neg=0)
    pipelines.setup_seed(seed)
    model = TLCGNN.Net(data, 48, 2, PI=np.zeros((tp + tn, 25)))
    model.apply(pipelines.weights_init)
    model, data = model.cuda(), data.to("cuda")
    images = topo.VicinityImages(n, ge, pairs, 2, flags=0)
    with torch.no_grad():
        images.kappa.copy_(torch.from_numpy(kappa))
    return model, data, images


def test_train_curvature_step_is_reproducible_and_agrees_with_autograd():
    """One full step twice from the same state and seeds: kappa.grad bit-equal.  Against the same step with torch's autograd for the
    decoder (f64, on the step's own embedding and table): d loss / d table within the decoder's bound; the scatter's agreement with
    index_add_ within L_max * 2^-52 * sum |g| per edge is test_weight_gradient_equals_the_composition_with_a_sequential_scatter."""
    import torch
    import torch.nn.functional as F
    from tlc_gnn_amd import pipelines
    model, data, images = _lp_setup(torch)
    opt = torch.optim.SGD(list(model.parameters()) + [images.kappa], lr=0.0)
    tap = _Tap(images)
    runs = []
    for _ in range(2):
        pipelines.setup_seed(9)
        x = pipelines.train_curvature(model, data, opt, tap)
        runs.append((x.detach().clone(), images.kappa.grad.clone(), tap.table.grad.clone(), tap.table.detach().clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and np.array_equal(_bits(runs[0][1].cpu().numpy()), _bits(runs[1][1].cpu().numpy()))
    assert bool(torch.isfinite(runs[0][1]).all()) and float(runs[0][1].abs().max()) > 0
    # the decoder's part against autograd: the same draws give the same embedding and the same pairs
    pipelines.setup_seed(9)
    model.train()
    emb = model._encode_train(data).detach()
    tp, tn = data.train_pos, data.train_neg
    idx = torch.cat((torch.arange(tp), tp + torch.from_numpy(np.random.randint(0, tn, tp)))).cuda()
    table = runs[0][3].clone().requires_grad_(True)
    pairs = model._tables(data, emb.device)[1][idx]
    p = {k: v.detach().double() for k, v in model.named_parameters()}
    post = emb.renorm(2, 0, 1)
    prob = _decode_ref(post.double(), pairs, table[idx].float().double(), p["linear_1.weight"], p["linear_1.bias"], p["linear.weight"], p["linear.bias"])
    assert float((prob.detach().float() - runs[0][0]).abs().max()) < 1e-5
    F.binary_cross_entropy(prob, data.total_edges_y.cuda()[idx].double()).backward()
    ok, err, atol = _close(runs[0][2], table.grad)
    print("d loss / d table: max |err| %.3e, atol %.3e" % (err, atol))
    assert ok, (err, atol)


def test_training_smoke_recovers_images_of_a_hidden_curvature():
    """128 pairs of the 300-node graph; the target is the images at a hidden curvature; from kappa = 0, 200 Adam steps through
    VicinityImages.  The MSE ends below half of its start (a sanity condition; the ratio reached is in DESIGN.md 6.11)."""
    import torch
    from tlc_gnn_amd import topo
    n, ge, _ = _hk()
    hidden = torch.from_numpy(np.random.default_rng(41).uniform(-0.4, 0.6, len(ge))).cuda()
    pairs = ge[np.random.RandomState(6).permutation(len(ge))[:128]]
    mod = topo.VicinityImages(n, ge, pairs, 2, flags=0)
    with torch.no_grad():
        target, st = mod(hidden)
    assert not st.any()
    opt = torch.optim.Adam(mod.parameters(), lr=0.02)
    losses = []
    for _ in range(200):
        opt.zero_grad()
        loss = ((mod()[0] - target) ** 2).mean()
        loss.backward()
        assert bool(torch.isfinite(mod.kappa.grad).all())
        opt.step()
        with torch.no_grad():
            mod.kappa.clamp_(min=-0.9)                                         # weights stay positive
        losses.append(float(loss))
    print("training smoke: MSE %.4e -> %.4e (ratio %.4f)" % (losses[0], losses[-1], losses[-1] / losses[0]))
    assert losses[-1] < 0.5 * losses[0]


def test_five_train_curvature_steps():
    """Five steps of the link predictor with a learned table: the predictions stay finite, kappa.grad is non-zero on edges that lie in
    some vicinity and exactly +0.0 on the edges that lie in none."""
    import torch
    from tlc_gnn_amd import pipelines
    model, data, images = _lp_setup(torch, tp=24, tn=24, seed=4)
    opt = torch.optim.Adam([{"params": model.parameters()}, {"params": [images.kappa], "lr": 1e-3}], lr=0.01)
    before = images.kappa.detach().clone()
    for _ in range(5):
        x = pipelines.train_curvature(model, data, opt, images)
        assert bool(torch.isfinite(x).all()) and bool(((x > 0) & (x < 1)).all())
    inside = (images.structure.seg_ptr[1:] > images.structure.seg_ptr[:-1]).cpu().numpy()
    g = images.kappa.grad.cpu().numpy()
    assert inside.any() and (~inside).any()
    assert (g[inside] != 0).any() and (_bits(g[~inside]) == 0).all()
    assert bool((images.kappa.detach() != before).any())

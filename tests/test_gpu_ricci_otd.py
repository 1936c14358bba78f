"""Ollivier-Ricci curvature with the EXACT transport distance on the GPU (tlc_ollivier_ricci_otd, method "OTD") against the closed
forms and the LP reference of tests/ricci_otd_cases.py.  Everything is compared exactly: W and D with == on int64, kappa with
np.array_equal against 1.0 - W / D computed in Python (int / int true division is correctly rounded, and so is the kernel's one
fp64 division of two exactly representable integers).  Nothing is compared at a tolerance, because there is nothing to tolerate --
except against Sinkhorn, whose own tested agreement bound (1e-7, tests/test_gpu_ricci.py) is used there."""
import ctypes as C
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

import ricci_otd_cases as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pytestmark = pytest.mark.gpu


def _csr(g):
    from tlc_gnn_amd import synth
    rowptr, col, _ = synth.edges_to_csr(g[0], g[1])
    return rowptr, col


def _run(g, pairs, alpha=0.5, **kw):
    from tlc_gnn_amd import engine
    rowptr, col = _csr(g)
    k, w, d = engine.ollivier_ricci_otd(rowptr, col, pairs, alpha=alpha, want_cost=True, **kw)
    assert k.dtype == np.float64 and w.dtype == np.int64 and d.dtype == np.int64 and len(k) == len(w) == len(d) == len(pairs)
    return k, w, d


def _same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def _check_exact(g, pairs, num=1, den=2):
    """the device's (kappa, W, D) of the pairs == the LP reference's, both orientations"""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    ref = oc.exact_kappa(g[0], g[1], pairs, num, den)
    got = _run(g, pairs, Fraction(num, den))
    assert np.array_equal(got[1], ref[1]), np.flatnonzero(got[1] != ref[1])[:8]
    assert np.array_equal(got[2], ref[2])
    assert np.array_equal(got[0], ref[0])
    assert _same(_run(g, pairs[:, ::-1], Fraction(num, den)), got)
    return got


def _check_closed(g, pairs, kappas):
    """closed forms at alpha = 1/2: D = 2 deg(s) deg(t), W = (1 - kappa) D (an integer), kappa = 1.0 - W / D"""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    deg = np.bincount(g[1].ravel(), minlength=g[0])
    D = [2 * int(deg[s]) * int(deg[t]) for s, t in pairs.tolist()]
    W = [(1 - k) * d for k, d in zip(kappas, D)]
    assert all(w.denominator == 1 for w in W)
    W = [int(w) for w in W]
    for p in (pairs, pairs[:, ::-1]):
        k, w, d = _run(g, p)
        assert w.tolist() == W and d.tolist() == D, (w.tolist(), W)
        assert np.array_equal(k, np.array([1.0 - a / b for a, b in zip(W, D)]))
    return k


# ---- 1. closed forms ---------------------------------------------------------------------------------------------------------
def test_closed_forms_at_alpha_one_half():
    for n in (3, 4, 5, 8):
        g = oc.complete(n)
        _check_closed(g, g[1], [oc.kappa_complete(n)] * len(g[1]))
    for n in (3, 4, 5, 6, 7):
        g = oc.cycle(n)
        _check_closed(g, g[1], [oc.kappa_cycle(n)] * n)
    for d in (1, 2, 5, 9):
        g = oc.star(d)
        k = _check_closed(g, g[1], [oc.kappa_star(d)] * d)
        if d == 1:
            assert k[0] == 1.0                                       # K_2: exactly 1, where the entropic plan leaks e^-10
    for p, q in ((2, 3), (4, 4), (3, 7)):
        g = oc.bipartite(p, q)
        _check_closed(g, g[1], [oc.kappa_bipartite(p, q)] * (p * q))
    g = oc.path(6)
    _check_closed(g, g[1], [oc.kappa_path(6, k) for k in range(5)])


# ---- 2. random graphs, every edge ------------------------------------------------------------------------------------------------
def _clustered():
    from tlc_gnn_amd import synth
    return 300, synth.holme_kim_edges(300, 900, triad_p=0.6, seed=4)


@pytest.mark.parametrize("kind", ["clustered", "tree", "dense"])
def test_every_edge_of_random_graphs_against_the_lp(kind):
    g = {"clustered": _clustered, "tree": lambda: oc.random_tree(200, 3), "dense": lambda: oc.gnp(24, 0.4, 5)}[kind]()
    assert len(g[1]) == {"clustered": 900, "tree": 199}.get(kind, len(g[1]))
    k, _, _ = _check_exact(g, g[1])
    assert (k <= 1.0).all() and (k >= -2.0).all()


# ---- 3. tier edges -----------------------------------------------------------------------------------------------------------
def _tier_graph(na, nb, seed=0):
    """the two-hub family with supports of na and nb entries on its hub edge (0, 1), and extras so that all four hop codes occur"""
    ds, dt = na - 1, nb - 1
    c = (min(ds, dt) - 1) // 3
    lo = min(ds, dt) - 1 - c
    return oc.two_hubs(ds, dt, c, m=lo // 3, cross=lo // 2, outside=5, seed=seed)


def _tier_of(na, nb, den=2):
    from tlc_gnn_amd import _lib
    wave = na * nb <= _lib.OTD_WAVE_PRODUCT and na + nb <= _lib.OTD_WAVE_SUPPORT and den * (na - 1) * (nb - 1) <= _lib.OTD_WAVE_DENOM
    return "wave" if wave else "group"


@pytest.mark.parametrize("shape,tier", [((64, 128), "wave"), ((91, 91), "group"), ((250, 6), "wave"), ((251, 6), "group"), ((2, 2), "wave"),
                                        ((2, 3), "wave"), ((2, 300), "group"), ((300, 2), "group"), ((128, 64), "wave"), ((401, 401), "group")])
def test_tier_edges_against_the_lp(shape, tier):
    na, nb = shape
    assert _tier_of(na, nb) == tier                                   # the shapes sit where the exported limits say
    g = _tier_graph(na, nb, seed=na + nb)
    deg = np.bincount(g[1].ravel(), minlength=g[0])
    assert deg[0] + 1 == na and deg[1] + 1 == nb
    _check_exact(g, [[0, 1]])


def test_wave_tier_limits_come_from_the_exported_constants():
    """one shape on either side of each of the three limits of the wavefront kernel, named from the constants"""
    from tlc_gnn_amd import _lib
    P, S = _lib.OTD_WAVE_PRODUCT, _lib.OTD_WAVE_SUPPORT
    a = int(np.sqrt(P))
    shapes = [(a, P // a), (a + 1, P // a + 1), (S - 6, 6), (S - 5, 6)]
    assert [_tier_of(*s) for s in shapes] == ["wave", "group", "wave", "group"]
    for na, nb in shapes:
        _check_exact(_tier_graph(na, nb, seed=na), [[0, 1]])
    # the denominator limit (u16 cells) binds at larger alpha denominators only: q = 64 on a square support, either side of it
    den = 64
    na = max(k for k in range(2, 90) if den * (k - 1) ** 2 <= _lib.OTD_WAVE_DENOM)
    assert _tier_of(na, na, den) == "wave" and _tier_of(na + 1, na + 1, den) == "group" and _tier_of(na + 1, na + 1) == "wave"
    for k in (na, na + 1):
        _check_exact(_tier_graph(k, k, seed=k), [[0, 1]], 3, den)


def test_cell_width_boundary_of_the_group_tier():
    """max_support below 4 094: u32 flow cells; from there on u64 (1024 * (max_support / 2)^2 could pass 2^32): a leaf against a hub
    on either side, against the LP, and with alpha = 1023/1024 on the wider side"""
    for d in (4090, 4091):                                            # supports (d + 1, 2): max_support d + 3
        g = oc.star(d)
        _check_exact(g, [[0, d]])
        _check_closed(g, [[0, 1]], [oc.kappa_star(d)])
    g = oc.star(4091)
    _check_exact(g, [[0, 7]], 1023, 1024)


def test_lds_and_slot_codes_and_the_800_square_hub_edge():
    """The group tier keeps the 2-bit codes in LDS while they fit beside the per-node state (engine.otd_lds_codes) and in the
    workspace slot beyond: the largest square support on the LDS side, the next one, and 800 x 800, against the closed form of the
    two-hub family -- after the same family has gone through the LP."""
    from tlc_gnn_amd import engine
    for d, c, m in ((6, 2, 1), (12, 0, 5), (10, 4, 0)):
        g = oc.two_hubs(d, d, c, m)
        got = _check_exact(g, [[0, 1]])
        assert Fraction(int(got[1][0]), int(got[2][0])) == 1 - oc.kappa_two_hubs(d, c, m)
    n_in = max(n for n in range(600, 900) if n * n <= engine.otd_lds_codes(2 * n))
    assert (n_in + 1) ** 2 > engine.otd_lds_codes(2 * n_in + 2) and n_in < 800
    for n, c, m in ((n_in, 90, 250), (n_in + 1, 0, 0), (800, 100, 300)):
        d = n - 1
        g = oc.two_hubs(d, d, c, m)
        _check_closed(g, [[0, 1]], [oc.kappa_two_hubs(d, c, m)])


# ---- 4. other alphas ---------------------------------------------------------------------------------------------------------
def test_other_alphas():
    g = oc.gnp(24, 0.4, 5)
    k, w, d = _run(g, g[1], alpha=1)
    assert np.array_equal(w, d) and np.array_equal(k, np.zeros(len(k))) and not np.signbit(k).any()
    _check_exact(g, g[1], 0, 1)
    _check_exact(g, g[1], 1, 4)
    assert _same(_run(g, g[1], alpha=0.25), _run(g, g[1], alpha=Fraction(1, 4)))
    k3, w3, d3 = _check_exact(g, g[1][:20], 1, 3)                     # not a binary fraction: only a Fraction can say it
    deg = np.bincount(g[1].ravel(), minlength=24)
    assert d3.tolist() == [3 * int(deg[s]) * int(deg[t]) for s, t in g[1][:20].tolist()]


# ---- 5. batch independence and determinism -------------------------------------------------------------------------------------------
def test_batch_independence_and_determinism():
    g = _clustered()
    e = g[1]
    whole = _run(g, e)
    assert _same(_run(g, e), whole)                                   # twice the same call
    rev = _run(g, e[::-1])
    assert _same([x[::-1] for x in rev], whole)
    parts = [_run(g, e[a:b]) for a, b in ((0, 1), (1, 450), (450, 900))]
    assert _same([np.concatenate([p[i] for p in parts]) for i in range(3)], whole)


def test_mixed_batches_equal_per_edge_calls():
    from test_gpu_ricci import _graph                                 # the Sinkhorn tests' own generator: the same hub graph, not a copy of it
    from tlc_gnn_amd import _lib
    rs = np.random.RandomState(3)
    n, edges = _graph("hub", rs)                                      # the hub of degree 220 of the Sinkhorn tests
    assert np.bincount(edges.ravel()).max() == 220
    pick = edges[np.concatenate([np.arange(0, 12), rs.choice(len(edges), 12, replace=False)])]
    batch = _run((n, edges), pick)
    singles = [_run((n, edges), pick[k:k + 1]) for k in range(len(pick))]
    assert _same([np.concatenate([s[i] for s in singles]) for i in range(3)], batch)
    ref = oc.exact_kappa(n, edges, pick[:4])
    assert _same([b[:4] for b in batch], ref)
    # a graph whose edges fall into both tiers: the hub edge and a few spokes beyond the wavefront limits, the leaf edges within
    g = oc.two_hubs(130, 140, 20, m=30, cross=40, outside=5, seed=2)
    deg = np.bincount(g[1].ravel(), minlength=g[0])
    na, nb = deg[g[1][:, 0]] + 1, deg[g[1][:, 1]] + 1
    big = (na * nb > _lib.OTD_WAVE_PRODUCT) | (na + nb > _lib.OTD_WAVE_SUPPORT)
    assert big.any() and (~big).any() and big[0]
    pick = np.concatenate([g[1][:3], g[1][~big][:9], g[1][-3:]])
    batch = _run(g, pick)
    singles = [_run(g, pick[k:k + 1]) for k in range(len(pick))]
    assert _same([np.concatenate([s[i] for s in singles]) for i in range(3)], batch)
    assert _same(batch, oc.exact_kappa(g[0], g[1], pick))


# ---- 6. relation to Sinkhorn -------------------------------------------------------------------------------------------------
def test_exact_cost_is_not_above_the_entropic_plans():
    """The Sinkhorn plan is feasible, so its cost cannot beat the optimum: kappa_otd >= kappa_sinkhorn, up to the Sinkhorn kernel's
    own tested agreement bound (1e-7, tests/test_gpu_ricci.py) -- and the two differ, so the new method is not the old one relabelled."""
    from tlc_gnn_amd import engine
    g = _clustered()
    rowptr, col = _csr(g)
    otd = engine.ollivier_ricci_otd(rowptr, col, g[1])
    sk = engine.ollivier_ricci_sinkhorn(rowptr, col, g[1])
    print("min(otd - sinkhorn) = %.3e, max = %.3e" % ((otd - sk).min(), (otd - sk).max()))
    assert (otd >= sk - 1e-7).all(), (otd - sk).min()
    assert np.abs(otd - sk).max() > 1e-6


# ---- 7. refusals and degenerate input ------------------------------------------------------------------------------------------
def test_refusals_and_degenerate_input():
    from tlc_gnn_amd import engine, synth
    rowptr, col, _ = synth.edges_to_csr(5, np.array([[0, 1], [1, 2], [3, 4]]))
    with pytest.raises(ValueError):
        engine.ollivier_ricci_otd(rowptr, col, np.array([[0, 2]]))            # two hops apart: not an edge
    with pytest.raises(ValueError):
        engine.ollivier_ricci_otd(rowptr, col, np.array([[0, 7]]))
    with pytest.raises(ValueError):
        engine.ollivier_ricci_otd(rowptr, col, np.array([[0, 1]]), alpha=0.3)
    k, w, d = engine.ollivier_ricci_otd(rowptr, col, np.array([[2, 2], [3, 4], [4, 4]]), want_cost=True)
    assert k.tolist() == [0.0, 1.0, 0.0] and w.tolist() == [0, 0, 0] and d.tolist() == [0, 2, 0]
    assert engine.ollivier_ricci_otd(rowptr, col, np.zeros((0, 2), dtype=np.int32)).shape == (0,)
    k, w, d = engine.ollivier_ricci_otd(rowptr, col, np.zeros((0, 2), dtype=np.int32), want_cost=True)
    assert k.shape == w.shape == d.shape == (0,) and w.dtype == np.int64


def test_c_abi_refusals():
    import torch
    from tlc_gnn_amd import _lib, synth
    L = _lib.lib()
    rowptr, col, _ = synth.edges_to_csr(3, np.array([[0, 1], [1, 2]]))
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()
    d_rowptr, d_col, d_edges = t(rowptr, np.int32), t(col, np.int32), t([[0, 1], [1, 2]], np.int32)
    kappa = torch.full((2,), 7.0, dtype=torch.float64, device="cuda")
    cost = torch.full((2,), 7, dtype=torch.int64, device="cuda")
    need = C.c_int64(0)
    assert L.tlc_ollivier_ricci_otd_work_bytes(2, 8, 16, C.byref(need)) == 0
    work = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    P = _lib.ptr

    def call(num=1, den=2, k=P(kappa), w=P(work), wb=need.value, ms=8, mp=16, E=2, rp=P(d_rowptr)):
        rc = L.tlc_ollivier_ricci_otd(3, rp, P(d_col), E, P(d_edges), num, den, k, P(cost), None, w, wb, ms, mp, _lib.stream_ptr())
        return rc, L.tlc_last_error().decode()

    for kw, word in ((dict(den=0), "alpha_den"), (dict(den=1025), "alpha_den"), (dict(num=3), "alpha_num"), (dict(num=-1), "alpha_num"),
                     (dict(k=None), "null"), (dict(rp=None), "null"), (dict(w=None), "workspace"), (dict(ms=1), "max_support"),
                     (dict(ms=_lib.OTD_MAX_SUPPORT + 1), "max_support"), (dict(mp=0), "max_product"), (dict(E=-1), "negative"),
                     (dict(w=C.c_void_p(work.data_ptr() + 8)), "aligned")):
        rc, msg = call(**kw)
        assert rc == 1 and word in msg, (kw, rc, msg)
    one = C.c_int64(0)
    assert L.tlc_ollivier_ricci_otd_work_bytes(2, 8, 16, C.byref(one)) == 0
    least = 16 + 16 + (one.value - 32) // 2                           # the counter, the list of two edges, ONE slot
    rc, msg = call(wb=least - 1)
    assert rc == 1 and "workspace" in msg
    torch.cuda.synchronize()
    assert kappa.tolist() == [7.0, 7.0]                               # nothing was launched by a refused call
    assert call(wb=least)[0] == 0 and call()[0] == 0 and call(E=0, k=None)[0] == 0
    torch.cuda.synchronize()
    assert kappa.tolist() == [0.5, 0.5] and cost.tolist() == [2, 2]   # the path on three nodes: both edges end edges


def test_small_max_product_gives_nan_for_that_edge_only():
    g = oc.two_hubs(130, 140, 20, m=30, cross=40, outside=5, seed=2)
    pick = np.concatenate([g[1][5:9], g[1][:1], g[1][-4:]])           # the hub edge (131 x 141 support pairs) in the middle
    full = _run(g, pick)
    cut = _run(g, pick, max_product=131 * 141 - 1)
    assert np.isnan(cut[0][4]) and cut[1][4] == -1 and cut[2][4] == 2 * 130 * 140
    keep = np.arange(len(pick)) != 4
    assert not np.isnan(full[0]).any() and _same([c[keep] for c in cut], [f[keep] for f in full])
    assert _same(_run(g, pick, max_product=131 * 141), full)


# ---- 8. drop-ins -------------------------------------------------------------------------------------------------------------
def _dropin_data(n=200, m=520, seed=9):
    import torch
    from tlc_gnn_amd import synth
    from tlc_gnn_amd.data import Data
    edges = synth.holme_kim_edges(n, m, triad_p=0.5, seed=seed)
    ei = torch.from_numpy(np.concatenate([edges, edges[:, ::-1]]).T.copy()).long()
    return edges, Data(x=torch.from_numpy(synth.synthetic_features(n, 24, seed=2)), edge_index=ei, y=torch.zeros(n, dtype=torch.long))


def test_loaddatas_dropin_both_methods():
    from tlc_gnn_amd import engine, loaddatas, synth
    n, m = 200, 520
    edges, data = _dropin_data(n, m)
    lst = loaddatas.compute_ricci_curvature(data, method="OTD")
    assert len(lst) == 2 * m and lst == sorted(lst)
    d = {(a, b): k for a, b, k in lst}
    und = np.unique(np.sort(edges, axis=1), axis=0)
    ref, _, _ = oc.exact_kappa(n, und, und)
    for (a, b), k in zip(und.tolist(), ref.tolist()):
        assert d[(a, b)] == k == d[(b, a)]
    # the default is Sinkhorn, bit for bit what the function returned before it had a method argument
    lst_s = loaddatas.compute_ricci_curvature(data)
    assert lst_s == loaddatas.compute_ricci_curvature(data, method="Sinkhorn") and lst_s != lst
    ei = data.edge_index.numpy().astype(np.int64)
    rowptr, col, _ = synth.edges_to_csr(n, und)
    flat = ei.T.reshape(-1)
    first = np.full(n, np.iinfo(np.int64).max, dtype=np.int64)
    np.minimum.at(first, flat, np.arange(len(flat)))
    swap = first[und[:, 0]] > first[und[:, 1]]
    oriented = np.where(swap[:, None], und[:, ::-1], und)
    kappa = engine.ollivier_ricci_sinkhorn(rowptr, col, oriented, alpha=0.5)
    old = sorted([[a, b, k] for (a, b), k in zip(oriented.tolist(), kappa.tolist())] + [[b, a, k] for (a, b), k in zip(oriented.tolist(), kappa.tolist())])
    assert lst_s == old


def test_kd_cache_keeps_the_two_methods_apart(tmp_path):
    from tlc_gnn_amd.Knowledge_Distillation import data_utils_LP
    _, data = _dropin_data(80, 200, seed=1)
    sk = data_utils_LP.compute_ricci_curvature(data, "toy", cache_dir=str(tmp_path))                  # the Sinkhorn cache first
    assert os.path.exists(str(tmp_path / "graph_toy_removevaltest.edge_list"))
    a = data_utils_LP.compute_ricci_curvature(data, "toy", cache_dir=str(tmp_path), method="OTD")
    assert os.path.exists(str(tmp_path / "graph_toy_removevaltest_otd.edge_list"))
    b = data_utils_LP.compute_ricci_curvature(data, "toy", cache_dir=str(tmp_path), method="OTD")     # second call: from the file
    assert a == b and len(a) == 400 and a != sk
    assert [r[:2] for r in a] == [r[:2] for r in sk]
    assert data_utils_LP.compute_ricci_curvature(data, "toy", cache_dir=str(tmp_path)) == sk


def test_convcurv_gin_takes_the_method():
    import torch
    from tlc_gnn_amd import synth
    from tlc_gnn_amd.data import Data
    from tlc_gnn_amd.Knowledge_Distillation import ConvCurv_GIN
    from tlc_gnn_amd.Knowledge_Distillation.Teacher_model import Teacher_Model
    n, edges = synth.shaped_graph("Cora", scale=0.05)[:2]
    und = torch.from_numpy(edges.T.copy())
    ei = torch.cat([und, und.flip(0)], dim=1)
    torch.manual_seed(3)
    teacher = Teacher_Model(hidden_dim=32, type='GAT', num_models=1, dropout=0, new_node_feat=True, use_edge_attn=True).eval()
    nets = {}
    for method in ("Sinkhorn", "OTD"):
        data = Data(x=torch.randn(n, 4), edge_index=ei.clone(), y=torch.zeros(n, dtype=torch.long))
        nets[method], data = ConvCurv_GIN.call(data, "Cora", 4, 3, teacher=teacher, ricci_method=method)
        assert nets[method].ricci_method == method and bool(torch.isfinite(nets[method].w_mul).all())
    cs, co = nets["Sinkhorn"]._vic._g2p.ricci_curv, nets["OTD"]._vic._g2p.ricci_curv
    assert cs.keys() == co.keys() and cs != co
    und_np = np.unique(np.sort(edges, axis=1), axis=0)
    ref, _, _ = oc.exact_kappa(n, und_np, und_np[:50])
    assert [co[(a, b)] for a, b in und_np[:50].tolist()] == ref.tolist()
    with pytest.raises(ValueError):
        ConvCurv_GIN.Net(data, "Cora", 4, 3, w_mul=nets["OTD"].w_mul, ricci_method="nonsense")
    w = nets["OTD"].w_mul
    assert ConvCurv_GIN.Net(data, "Cora", 4, 3, ricci_method="OTD", w_mul=w).w_mul is w

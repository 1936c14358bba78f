"""GPU: the distance filtration of packed batches (tlc_dist_filtration, csrc/dist_filt.hip) and its VJP in the edge weights, against the
reference's recorded values, the numpy restatement of tests/dist_filt_cases.py (itself pinned to the reference on the CPU), the
vicinity pipeline's own filtration and the oracle.  Every comparison is np.array_equal unless it says otherwise."""
import functools
import os

import numpy as np
import pytest

import dist_filt_cases as dc

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OPTS = {0: "sum", dc.DESC_MIN: "min", dc.DESC_MAX: "max"}


def _kw(flags):
    return dict(descriptor=OPTS[flags & dc.DESC_ROOT1], norm="none" if flags & dc.NO_NORM else ("max_eps" if flags & dc.NORM_EPS else "max"),
                unreachable_100=bool(flags & dc.UNREACHABLE_100), include_roots=bool(flags & dc.INCLUDE_ROOTS))


def _cuda(packed):
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in packed)


def _fwd(packed, flags=0, work=None, dev=None):
    """-> f, status, parent as numpy; never raises on a status"""
    from tlc_gnn_amd import engine
    no, eo, E, W, R = dev if dev is not None else _cuda(packed)
    f, st, P = engine.dist_filtration(no, eo, E, W, R, work=work, check=False, **_kw(flags))
    return f.cpu().numpy(), st.cpu().numpy(), P.cpu().numpy()


def _vjp(packed, flags, parent, g, dev=None):
    import torch
    from tlc_gnn_amd import engine
    no, eo, E, W, R = dev if dev is not None else _cuda(packed)
    gw, st = engine.dist_filtration_vjp(no, eo, E, W, R, torch.from_numpy(np.ascontiguousarray(parent)).cuda(), torch.from_numpy(g).cuda(),
                                        check=False, **_kw(flags))
    return gw.cpu().numpy(), st.cpu().numpy()


def test_cuts_are_the_header_constants():
    from tlc_gnn_amd import _lib
    assert (_lib.DIST_WAVE_NMAX, _lib.DIST_WG_NMAX, _lib.DIST_WG_MMAX) == (64, 2048, 4096)


def test_golden_through_the_c_abi():
    """The reference's values for 55 graphs of 2 .. 200 nodes: one root (data_utils_NC build_fv, / (max + 1e-10)) and two roots
    (riccidist2dgm build_fv: sum / min / max); the graph that is its two roots is ST_ZERO_RANGE with its slice untouched."""
    z = np.load(os.path.join(G, "dist_filt_ref.npz"))
    packed = (z["node_offs"], z["edge_offs"], z["edges"], z["w"], z["roots"])
    one = (packed[0], packed[1], packed[2], packed[3], np.stack([z["roots"][:, 0], np.full(len(z["roots"]), -1)], 1).astype(np.int32))
    f, st, _ = _fwd(one, dc.NORM_EPS)
    assert not st.any() and np.array_equal(f, z["f_one"])
    for name, flag in (("f_sum", 0), ("f_min", dc.DESC_MIN), ("f_max", dc.DESC_MAX)):
        f, st, _ = _fwd(packed, flag)
        assert np.array_equal(st, z["st_two"]), name
        assert np.array_equal(f, z[name], equal_nan=True), name             # (NaN: the untouched slice of the refused graph)


# ---- the cuts ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cut_cases():
    """[(name, n, edges, w, r0, r1, flags, f, status, parent)] with the restatement's outputs, computed once."""
    rng = np.random.default_rng(77)
    raw = []
    for n in (1, 2, 63, 64, 65):
        for kind in ("generic", "ties"):
            m = 0 if n == 1 else min(n * (n - 1) // 2, n + n // 2)
            e = dc.random_connected(rng, n, m) if n > 1 else np.zeros((0, 2), np.int32)
            w = dc.generic_weights(rng, len(e)) if kind == "generic" else dc.tie_weights(rng, len(e))
            r0, r1 = (0, -1) if n == 1 else (int(v) for v in rng.choice(n, 2, replace=False))
            raw.append(("%s%d" % (kind, n), n, e, w, r0, r1, dc.NORM_EPS))
            if n > 2:
                raw.append(("%s%d one root" % (kind, n), n, e, w, r0, -1, 0))
    raw.append(("one node, norm max", 1, np.zeros((0, 2), np.int32), np.zeros(0), 0, -1, 0))          # ST_ZERO_RANGE
    raw.append(("two roots and nothing else", 2, dc.path(2), np.array([0.7]), 1, 0, 0))                 # ST_ZERO_RANGE
    raw.append(("star300", 300, dc.star(300), dc.generic_weights(rng, 299), 5, 17, 0))
    raw.append(("cycle64 antipode", 64, dc.cycle(64), np.ones(64), 0, -1, 0))
    raw.append(("cycle66 antipode", 66, dc.cycle(66), np.ones(66), 0, 33, dc.DESC_MAX))
    raw.append(("grid8x8 unit", 64, dc.grid(8, 8), np.ones(len(dc.grid(8, 8))), 0, 63, 0))
    raw.append(("grid9x11 unit", 99, dc.grid(9, 11), np.ones(len(dc.grid(9, 11))), 4, 90, dc.DESC_MIN))
    e = dc.random_connected(rng, 40, 60)
    raw.append(("equal roots", 40, e, dc.tie_weights(rng, 60), 7, 7, 0))
    two = np.concatenate([dc.random_connected(rng, 30, 40), dc.random_connected(rng, 20, 25) + 30]).astype(np.int32)
    raw.append(("two components", 50, two, dc.generic_weights(rng, 65), 3, 35, dc.UNREACHABLE_100))
    raw.append(("two components, 70", 70, np.concatenate([two, dc.path(20) + 50]).astype(np.int32), dc.tie_weights(rng, 84), 3, 12, dc.UNREACHABLE_100 | dc.NORM_EPS))
    e = dc.random_connected(rng, 2049, 4097)
    raw.append(("random 2049 / 4097", 2049, e, dc.generic_weights(rng, 4097), 11, 1500, 0))
    small = dc.random_connected(rng, 14, 20)
    wsm = dc.tie_weights(rng, 20)
    for desc in (0, dc.DESC_MIN, dc.DESC_MAX):
        for nf in (0, dc.NORM_EPS, dc.NO_NORM):
            for extra in (0, dc.INCLUDE_ROOTS | dc.UNREACHABLE_100):
                raw.append(("flags %#x" % (desc | nf | extra), 14, small, wsm, 2, 9, desc | nf | extra))
    out = []
    for name, n, e, w, r0, r1, fl in raw:
        f, st, P = dc.forward(n, e, w, r0, r1, fl)
        out.append((name, n, e, w, r0, r1, fl, f, st, P))
    return out


def _path_case(n):
    """A path rooted at its last node: D_x = w[x] + w[x + 1] + ... left to right, by sequential cumulative sums"""
    rng = np.random.default_rng(n)
    w = dc.generic_weights(rng, n - 1)
    S = np.zeros(n)
    for k in range(n - 1):
        S[:k + 1] += w[k]
    return w, S / S.max(), np.stack([np.r_[np.arange(1, n), -1], np.full(n, -1)]).astype(np.int32)


def test_restatement_parity_at_the_cuts():
    """n = 1, 2, 63, 64, 65, a star, even cycles, unit grids (every source falls back), graphs that are not connected, equal roots, a
    2 049-node graph with 4 097 edges, every flag combination -- each flag word as one batch: f, status, parent and grad_w"""
    cases = _cut_cases()
    rng = np.random.default_rng(3)
    for fl in sorted({c[6] for c in cases}):
        sel = [c for c in cases if c[6] == fl]
        packed = dc.pack([(c[1], c[2], c[3], c[4], c[5]) for c in sel])
        dev = _cuda(packed)
        f, st, P = _fwd(packed, fl, dev=dev)
        g = rng.normal(size=int(packed[0][-1]))
        gw, st2 = _vjp(packed, fl, P, g, dev=dev)
        for k, c in enumerate(sel):
            a, b, ea, eb = packed[0][k], packed[0][k + 1], packed[1][k], packed[1][k + 1]
            assert st[k] == c[8] == st2[k], (c[0], st[k], c[8], st2[k])
            assert np.array_equal(P[:, a:b], c[9]), c[0]
            if c[8] != dc.ST_OK:
                assert np.isnan(f[a:b]).all() and np.isnan(gw[ea:eb]).all(), c[0]
                continue
            assert np.array_equal(f[a:b], c[7]), c[0]
            want, _ = dc.vjp(c[1], c[2], c[3], c[4], c[5], fl, c[9], g[a:b])
            assert np.array_equal(gw[ea:eb], want), c[0]
    assert any(c[8] == dc.ST_ZERO_RANGE for c in cases)                       # n = 1 under norm='max'


@pytest.mark.parametrize("n", [2048, 2049])
def test_paths_at_the_workgroup_cut(n):
    w, f_want, P_want = _path_case(n)
    packed = dc.pack([(n, dc.path(n), w, n - 1, -1)])
    f, st, P = _fwd(packed, 0)
    assert not st.any() and np.array_equal(f, f_want) and np.array_equal(P, P_want)
    g = np.random.default_rng(1).normal(size=n)
    gw, st = _vjp(packed, 0, P, g)
    want, _ = dc.vjp(n, dc.path(n), w, n - 1, -1, 0, P_want, g)
    assert not st.any() and np.array_equal(gw, want)


def test_big_unit_grid_every_source_falls_back_in_the_device_class():
    """46 x 46 unit grid (2 116 nodes: the whole-device class): distances are Manhattan distances, exact in fp64; every source with two
    shortest paths takes the per-source search, in groups that the workspace sizes -- the least workspace gives the same bits"""
    import torch
    from tlc_gnn_amd import _lib, engine
    a = 46
    e = dc.grid(a, a)
    yy, xx = np.divmod(np.arange(a * a), a)
    r0, r1 = 5 * a + 7, 40 * a + 30
    d0 = (np.abs(yy - 5) + np.abs(xx - 7)).astype(np.float64)
    d1 = (np.abs(yy - 40) + np.abs(xx - 30)).astype(np.float64)
    q = d0 + d1
    q[[r0, r1]] = 0.0
    packed = dc.pack([(a * a, e, np.ones(len(e)), r0, r1)])
    need = engine.dist_filtration_work_bytes(1, a * a, len(e))
    work = torch.empty(need + 255, dtype=torch.uint8, device="cuda")
    f, st, P = _fwd(packed, 0, work=work)
    assert not st.any() and np.array_equal(f, q / q.max())
    assert np.array_equal(P[0], dc.tree(a * a, e, np.ones(len(e)), d0)) and np.array_equal(P[1], dc.tree(a * a, e, np.ones(len(e)), d1))
    off = (-work.data_ptr()) % 256
    fallbacks = int(work[off + _lib.DIST_WORK_FALLBACKS_OFF:off + _lib.DIST_WORK_FALLBACKS_OFF + 8].cpu().numpy().view(np.uint64)[0])
    assert fallbacks >= (a - 1) * (a - 1)                                     # every node off the roots' rows and columns at least
    f2, _, P2 = _fwd(packed, 0)                                              # the engine's own workspace
    f3, _, P3 = _fwd(packed, 0, work=torch.empty(need + 255 + 64 * 8 * 2304, dtype=torch.uint8, device="cuda"))
    assert np.array_equal(f, f2) and np.array_equal(f, f3) and np.array_equal(P, P2) and np.array_equal(P, P3)


# ---- against the vicinity pipeline and the oracle ---------------------------------------------------------------------------------------
def test_pubmed_shaped_vicinities_equal_the_vicinity_pipeline_and_the_oracle():
    """256 pairs at hop 2 (`Vicinities.batch`, KD_LP_FLAGS) and 256 node vicinities (`NodeVicinities.batch`, KD_NC_FLAGS) of the
    PubMed-shaped graph: the packed filtration with the same flags == f of tlc_vicinity_filtration == the oracle's vicinity_filtration"""
    import torch
    from oracle import oracle
    from tlc_gnn_amd import engine, synth
    from tlc_gnn_amd.Knowledge_Distillation import data_utils_LP as kd_lp, data_utils_NC as kd_nc
    n, edges, kappa, hop, _ = synth.shaped_graph("PubMed")
    curv = np.concatenate([np.concatenate([edges, edges[:, ::-1]]).astype(np.float64), np.concatenate([kappa, kappa])[:, None]], axis=1)
    rowptr, col, wcsr = synth.edges_to_csr(n, edges, kappa)
    key = edges.min(1).astype(np.int64) * n + edges.max(1)
    order = np.argsort(key)
    rs = np.random.RandomState(9)
    pairs = edges[rs.choice(len(edges), 256, replace=False)]
    nodes = rs.choice(n, 256, replace=False)
    for vic, query, qpairs, flags in ((kd_lp.Vicinities(edges, curv), pairs, pairs, kd_lp.KD_LP_FLAGS),
                                      (kd_nc.NodeVicinities(edges, curv), nodes, np.stack([nodes, nodes], 1), kd_nc.KD_NC_FLAGS)):
        b = vic.batch(query, 2)
        no, eo, ids, E = (b[k].cpu().numpy() for k in ("node_ptr", "edge_ptr", "ids", "edges"))
        assert not b["status"].any() and (no[1:] > no[:-1]).all()
        owner = np.repeat(np.arange(256), eo[1:] - eo[:-1])
        ga, gb = ids[no[owner] + E[:, 0]], ids[no[owner] + E[:, 1]]
        w = (kappa[order[np.searchsorted(key[order], np.minimum(ga, gb) * n + np.maximum(ga, gb))]] + 1.0)
        single = bool(flags & 0xC0 == 0xC0)
        roots = np.array([[np.searchsorted(ids[no[k]:no[k + 1]], qpairs[k, 0]), -1 if single else np.searchsorted(ids[no[k]:no[k + 1]], qpairs[k, 1])]
                          for k in range(256)], np.int32)
        f, st, _ = engine.dist_filtration(b["node_ptr"], b["edge_ptr"], b["edges"], torch.from_numpy(w).cuda(), torch.from_numpy(roots).cuda(),
                                          descriptor="sum", norm="max_eps", include_roots=True, unreachable_100=True)
        assert torch.equal(f, b["f"])
        if single:
            continue                                                          # (the oracle has no single-root descriptor)
        cap = int((no[1:] - no[:-1]).max())
        offs, oids, of, on, om, ost = oracle.vicinity_filtration(rowptr, col, wcsr, qpairs, 2, flags=flags, cap=cap)
        f = f.cpu().numpy()
        for k in range(256):
            assert ost[k] == 0 and on[k] == no[k + 1] - no[k] and np.array_equal(f[no[k]:no[k + 1]], of[offs[k]:offs[k] + on[k]]), k


# ---- the batch, the workspace, the run --------------------------------------------------------------------------------------------------
def test_twenty_thousand_tiny_graphs_and_one_of_each_class_against_every_graph_alone():
    import torch
    from tlc_gnn_amd import engine
    rng = np.random.default_rng(11)
    graphs = []
    for _ in range(20000):
        n = int(rng.integers(2, 7))
        e = dc.random_connected(rng, n, int(rng.integers(n - 1, n * (n - 1) // 2 + 1)))
        graphs.append((n, e, dc.tie_weights(rng, len(e)), 0, n - 1))
    graphs.insert(5000, (60, dc.random_connected(rng, 60, 100), dc.tie_weights(rng, 100), 1, 2))
    graphs.insert(10000, (500, dc.random_connected(rng, 500, 900), dc.tie_weights(rng, 900), 1, 2))
    graphs.insert(15000, (2100, dc.random_connected(rng, 2100, 4200), dc.tie_weights(rng, 4200), 1, 2))
    packed = dc.pack(graphs)
    dev = _cuda(packed)
    need = engine.dist_filtration_work_bytes(len(graphs), int(packed[0][-1]), int(packed[1][-1]))
    least = torch.empty(need + 255, dtype=torch.uint8, device="cuda")
    f, st, P = _fwd(packed, dc.NORM_EPS, dev=dev, work=least)
    assert not st.any()
    f2, _, P2 = _fwd(packed, dc.NORM_EPS, dev=dev)                            # the full workspace; run against run
    f3, _, P3 = _fwd(packed, dc.NORM_EPS, dev=dev)
    assert np.array_equal(f, f2) and np.array_equal(f2, f3) and np.array_equal(P, P2) and np.array_equal(P2, P3)
    g = rng.normal(size=len(f))
    gw, st = _vjp(packed, dc.NORM_EPS, P, g, dev=dev)
    gw2, _ = _vjp(packed, dc.NORM_EPS, P, g, dev=dev)
    assert not st.any() and np.array_equal(gw, gw2)
    # every graph alone: results stay on the device until the end
    no, eo, E, W, R = dev
    gd, Pd = torch.from_numpy(g).cuda(), torch.from_numpy(P).cuda()
    work = torch.empty(engine.dist_filtration_work_bytes(1, 2100, 4200, vjp=True) + 255, dtype=torch.uint8, device="cuda")
    fs, gs = [], []
    no_all = torch.stack([torch.zeros_like(no[1:]), no[1:] - no[:-1]], 1).contiguous()
    eo_all = torch.stack([torch.zeros_like(eo[1:]), eo[1:] - eo[:-1]], 1).contiguous()
    for k, (n, e, _, _, _) in enumerate(graphs):
        a, ea = int(packed[0][k]), int(packed[1][k])
        zero2, eo1 = no_all[k], eo_all[k]
        fk, _, Pk = engine.dist_filtration(zero2, eo1, E[ea:ea + len(e)], W[ea:ea + len(e)], R[k:k + 1], norm="max_eps", work=work, total_nodes=n,
                                           check=False)
        if k % 50 == 0 or n > 6:                                              # the VJP alone on a sample and on the three large ones
            gk, _ = engine.dist_filtration_vjp(zero2, eo1, E[ea:ea + len(e)], W[ea:ea + len(e)], R[k:k + 1], Pk, gd[a:a + n], norm="max_eps",
                                               work=work, total_nodes=n, check=False)
            gs.append((ea, gk))
        fs.append(fk)
    assert np.array_equal(torch.cat(fs).cpu().numpy(), f)
    for ea, gk in gs:
        assert np.array_equal(gk.cpu().numpy(), gw[ea:ea + len(gk)])


# ---- derivatives --------------------------------------------------------------------------------------------------------------------------
def test_exact_finite_differences_on_twelve_nodes():
    """Distinct random weights: central differences of the DEVICE forward (h = 1e-6) against the device VJP, both roots, every descriptor,
    normalised and not.  Truncation h^2 |f'''| < 1e-10 and rounding 2^-52 |f| / h ~ 1e-9 stay a factor of fifty under the bound 1e-7."""
    rng = np.random.default_rng(5)
    n, r0, r1 = 12, 3, 7
    e = dc.random_connected(rng, n, 22)
    w, g = dc.generic_weights(rng, len(e)), rng.normal(size=n)
    m = len(e)
    for desc in (0, dc.DESC_MIN, dc.DESC_MAX):
        for nf in (0, dc.NORM_EPS, dc.NO_NORM):
            fl = desc | nf
            base = dc.pack([(n, e, w, r0, r1)])
            f, st, P = _fwd(base, fl)
            gw, _ = _vjp(base, fl, P, g)
            graphs = []
            for k in range(m):
                for s in (1e-6, -1e-6):
                    wk = w.copy()
                    wk[k] += s
                    graphs.append((n, e, wk, r0, r1))
            fp, st, _ = _fwd(dc.pack(graphs), fl)
            assert not st.any()
            vals = fp.reshape(m, 2, n) @ g
            num = (vals[:, 0] - vals[:, 1]) / 2e-6
            assert np.abs(num - gw).max() < 1e-7, (hex(fl), np.abs(num - gw).max())


def test_gradcheck_of_the_autograd_function():
    import torch
    from tlc_gnn_amd import autograd
    rng = np.random.default_rng(8)
    graphs = [(n, dc.random_connected(rng, n, n + 4), None, 0, n - 1) for n in (6, 9)]
    graphs = [(n, e, dc.generic_weights(rng, len(e)), a, b) for n, e, _, a, b in graphs]
    no, eo, E, W, R = _cuda(dc.pack(graphs))
    for kw in (dict(descriptor="sum", norm="max"), dict(descriptor="min", norm="max_eps"), dict(descriptor="max", norm="none")):
        w = W.clone().requires_grad_(True)
        assert torch.autograd.gradcheck(lambda x: autograd.distance_filtration(x, no, eo, E, R, **kw), (w,))     # torch's fp64 defaults


def test_training_smoke_through_the_images():
    """Weights started at 1 on 64 small graphs, trained through topo.images(topo.distance_filtration(w, ...), grad='full', imager=...)
    toward images made from hidden weights: the loss after 200 Adam steps is below a tenth of the start."""
    import torch
    from tlc_gnn_amd import topo
    from tlc_gnn_amd.Knowledge_Distillation import pimg
    rng = np.random.default_rng(21)
    graphs = []
    for _ in range(64):
        n = int(rng.integers(8, 20))
        e = dc.random_connected(rng, n, n + int(rng.integers(2, 6)))
        graphs.append((n, e, dc.generic_weights(rng, len(e)), 0, -1))
    no, eo, E, W, _ = _cuda(dc.pack(graphs))
    im = pimg.PersistenceImager(resolution=8, kernel_params={"sigma": 0.05})
    with torch.no_grad():
        target = topo.images(topo.distance_filtration(W, no, eo, E), no, eo, E, imager=im, grad="full")
    w = torch.ones_like(W, requires_grad=True)
    opt = torch.optim.Adam([w], lr=0.02)
    losses = []
    for _ in range(200):
        opt.zero_grad()
        loss = ((topo.images(topo.distance_filtration(w, no, eo, E), no, eo, E, imager=im, grad="full") - target) ** 2).sum()
        loss.backward()
        assert bool(torch.isfinite(w.grad).all())
        opt.step()
        with torch.no_grad():
            w.clamp_(min=0.05)
        losses.append(float(loss.detach()))
    print("distance filtration training: loss %.4e -> %.4e (ratio %.4f)" % (losses[0], losses[-1], losses[-1] / losses[0]))
    assert losses[-1] < 0.1 * losses[0]


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_other_graphs_alone():
    import torch
    from tlc_gnn_amd import _lib, engine
    rng = np.random.default_rng(2)
    good = [(n, dc.random_connected(rng, n, n + 5), None, 0, 1) for n in (10, 70, 30)]
    good = [(n, e, dc.tie_weights(rng, len(e)), a, b) for n, e, _, a, b in good]
    want_f, want_st, want_P = _fwd(dc.pack(good), 0)
    assert not want_st.any()
    victim = (20, dc.random_connected(rng, 20, 30), dc.generic_weights(rng, 30), 0, 5)

    def spoil(kind):
        n, e, w, r0, r1 = victim[0], victim[1].copy(), victim[2].copy(), victim[3], victim[4]
        if kind == "zero weight":
            w[3] = 0.0
        elif kind == "negative weight":
            w[3] = -1.0
        elif kind == "nan weight":
            w[3] = np.nan
        elif kind == "inf weight":
            w[3] = np.inf
        elif kind == "loop":
            e[4] = (6, 6)
        elif kind == "repeated edge":
            e[5] = e[9][::-1]
        elif kind == "id out of range":
            e[2, 1] = 20
        elif kind == "root out of range":
            r1 = 20
        elif kind == "negative root":
            r0 = -1
        return n, e, w, r0, r1

    for kind in ("zero weight", "negative weight", "nan weight", "inf weight", "loop", "repeated edge", "id out of range", "root out of range",
                 "negative root"):
        packed = dc.pack([good[0], good[1], spoil(kind), good[2]])
        f, st, P = _fwd(packed, 0)
        assert st.tolist() == [0, 0, dc.ST_BAD_INPUT, 0], (kind, st)
        keep = np.r_[0:80, 100:130]
        assert np.array_equal(f[keep], want_f) and np.isnan(f[80:100]).all() and np.array_equal(P[:, keep], want_P), kind
        gw, st = _vjp(packed, 0, P, np.ones(130))
        assert st.tolist() == [0, 0, dc.ST_BAD_INPUT, 0] and np.isnan(gw[packed[1][2]:packed[1][3]]).all(), kind
        with pytest.raises(RuntimeError, match=r"\[2\]"):
            engine.dist_filtration(*_cuda(packed))
    # decreasing offsets: graph 1 runs backwards
    no, eo, E, W, R = dc.pack(good)
    bad_no = no.copy()
    bad_no[2] = no[1] - 3
    f, st, _ = _fwd((bad_no, eo, E, W, R), 0)
    assert st[0] == 0 and st[1] == dc.ST_BAD_INPUT and np.array_equal(f[:10], want_f[:10])
    # a graph that is not connected, without unreachable_100
    two = np.concatenate([dc.path(5), dc.path(4) + 5]).astype(np.int32)
    f, st, _ = _fwd(dc.pack([good[0], (9, two, np.ones(7), 0, -1)]), 0)
    assert st.tolist() == [0, _lib.ST_DISCONNECTED] and np.array_equal(f[:10], want_f[:10]) and np.isnan(f[10:]).all()
    # a workspace below the minimum: TLC_ERR_INVALID_ARG, nothing launched
    dev = _cuda(dc.pack(good))
    need = engine.dist_filtration_work_bytes(3, 110, int(eo[-1]))
    with pytest.raises(_lib.TlcError, match="TLC_ERR_INVALID_ARG"):
        engine.dist_filtration(*dev, work=torch.empty(need + 255 - 256, dtype=torch.uint8, device="cuda"))
    with pytest.raises(_lib.TlcError, match="TLC_ERR_INVALID_ARG"):
        engine.dist_filtration_vjp(*dev, torch.from_numpy(want_P).cuda(), torch.ones(110, dtype=torch.float64, device="cuda"),
                                   work=torch.empty(1024, dtype=torch.uint8, device="cuda"))


def test_parent_is_optional_through_the_c_abi():
    """d_parent NULL: the same f and status, in all three classes"""
    import ctypes as C
    import torch
    from tlc_gnn_amd import _lib, engine
    rng = np.random.default_rng(14)
    graphs = [(n, dc.random_connected(rng, n, 2 * n), None, 0, 1) for n in (20, 70, 2100)]
    graphs = [(n, e, dc.tie_weights(rng, len(e)), a, b) for n, e, _, a, b in graphs]
    no, eo, E, W, R = _cuda(dc.pack(graphs))
    want, st, _ = engine.dist_filtration(no, eo, E, W, R)
    tot_n, tot_m = int(no[-1]), int(E.shape[0])
    need = engine.dist_filtration_work_bytes(3, tot_n, tot_m)
    work = torch.empty(need + 255, dtype=torch.uint8, device="cuda")
    work = work[(-work.data_ptr()) % 256:]
    f = torch.full((tot_n,), float("nan"), dtype=torch.float64, device="cuda")
    st2 = torch.full((3,), 9, dtype=torch.uint8, device="cuda")
    rc = _lib.lib().tlc_dist_filtration(C.c_int64(3), _lib.ptr(no), _lib.ptr(eo), _lib.ptr(E), _lib.ptr(W), _lib.ptr(R), C.c_int64(tot_n),
                                        C.c_int64(tot_m), C.c_uint32(0), _lib.ptr(f), _lib.ptr(st2), None, _lib.ptr(work), C.c_int64(work.numel()),
                                        _lib.stream_ptr())
    assert rc == 0 and torch.equal(f, want) and torch.equal(st2, st) and not st.any()
    # an unknown flag and a misaligned workspace are refused before anything is launched
    for flags, wk in ((0x200, work), (0, work[8:])):
        rc = _lib.lib().tlc_dist_filtration(C.c_int64(3), _lib.ptr(no), _lib.ptr(eo), _lib.ptr(E), _lib.ptr(W), _lib.ptr(R), C.c_int64(tot_n),
                                            C.c_int64(tot_m), C.c_uint32(flags), _lib.ptr(f), _lib.ptr(st2), None, _lib.ptr(wk),
                                            C.c_int64(work.numel()), _lib.stream_ptr())
        assert rc == 1, flags


def test_no_graphs():
    import torch
    from tlc_gnn_amd import engine, topo
    no = torch.zeros(1, dtype=torch.int64, device="cuda")
    E = torch.zeros((0, 2), dtype=torch.int32, device="cuda")
    W = torch.zeros(0, dtype=torch.float64, device="cuda")
    R = torch.zeros((0, 2), dtype=torch.int32, device="cuda")
    f, st, P = engine.dist_filtration(no, no, E, W, R)
    assert f.numel() == 0 and st.numel() == 0 and tuple(P.shape) == (2, 0)
    gw, st = engine.dist_filtration_vjp(no, no, E, W, R, P, f)
    assert gw.numel() == 0 and st.numel() == 0
    assert topo.distance_filtration(W, no, no, E).numel() == 0

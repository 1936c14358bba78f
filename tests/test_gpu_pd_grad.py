"""GPU: d diagram / d filtration of the exact extended persistence (csrc/pd_grad.hip; autograd.ExtendedPersistence; topo).

The reference for the ids and the gradients is the numpy restatement of the rule (lowest id v with f[v] == c) and of the fixed
summation order in tests/pd_grad_cases.py; ids and gradient bits are compared with ==.  That the ids are the true critical vertices
is shown by exact finite differences (test_ids_are_the_critical_vertices) and by torch.autograd.gradcheck."""
import ctypes as C

import numpy as np
import pytest

import pd_grad_cases as cases
from pd_grad_cases import KEYS, SENTINEL, ST_BAD_INPUT, ST_OK, ST_TOO_LARGE

pytestmark = pytest.mark.gpu
KEEP0 = 0x1
FILL = 777.0                     # what grad_f holds before a call: slices the entry must not write keep it


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _dev(torch, a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


class Batch:
    """a packed batch on the host and on the device, its diagrams, ids (device arrays pre-filled with SENTINEL) and the restatement"""

    def __init__(self, torch, graphs, fs, flags=KEEP0, pd_large="host", forward=True):
        from tlc_gnn_amd import engine
        self.graphs = graphs
        self.no, self.eo, self.E, self.f = cases.pack(graphs, fs)
        self.B = len(graphs)
        self.d_no, self.d_eo = _dev(torch, self.no, torch.int64), _dev(torch, self.eo, torch.int64)
        self.d_E = _dev(torch, self.E if len(self.E) else np.zeros((1, 2)), torch.int32).reshape(-1, 2)
        self.d_f = _dev(torch, self.f if len(self.f) else np.zeros(1), torch.float64)
        if forward:
            self.d_pd = engine.pd_from_filtration(self.d_no, self.d_eo, self.d_E, self.d_f, flags=flags, want_rank=False, pd_large=pd_large)
            self.pull()

    def pull(self):
        self.pd = {k: self.d_pd[k].cpu().numpy() for k in KEYS + ("counts",)}

    def vertices(self, torch, work=None):
        """tlc_pd_point_vertices into arrays filled with SENTINEL -> (dict of device id arrays + status, rc)"""
        from tlc_gnn_amd import _lib, engine
        ids = {k: torch.full(tuple(self.d_pd[k].shape), SENTINEL, dtype=torch.int32, device="cuda") for k in ("up", "down", "one")}
        ids["ext0"] = torch.full((max(self.B, 1), 2), SENTINEL, dtype=torch.int32, device="cuda")
        ids["status"] = torch.full((max(self.B, 1),), 99, dtype=torch.uint8, device="cuda")
        work, nbytes = engine._pd_grad_work(torch, self.d_no, self.d_eo, work)
        p = _lib.ptr
        rc = _lib.lib().tlc_pd_point_vertices(C.c_int64(self.B), p(self.d_no), p(self.d_eo), p(self.d_f), p(self.d_pd["up"]),
                                              p(self.d_pd["down"]), p(self.d_pd["one"]), p(self.d_pd["ext0"].contiguous()),
                                              p(self.d_pd["counts"].contiguous()), p(ids["up"]), p(ids["down"]), p(ids["one"]), p(ids["ext0"]),
                                              p(ids["status"]), p(work), C.c_int64(nbytes), _lib.stream_ptr())
        _lib.check(rc, "tlc_pd_point_vertices")
        ids["ext0"], ids["status"] = ids["ext0"][:self.B], ids["status"][:self.B]
        return ids

    def grad(self, torch, ids, grads, work=None):
        """tlc_pd_filtration_grad into a slice array filled with FILL -> numpy"""
        from tlc_gnn_amd import engine
        out = torch.full((max(len(self.f), 1),), FILL, dtype=torch.float64, device="cuda")
        g = engine.pd_filtration_grad(self.d_no, self.d_eo, self.d_pd["counts"], ids, *[grads[k] for k in KEYS], work=work, out=out)
        return g.cpu().numpy()[:len(self.f)]

    def random_grads(self, torch, seed):
        rs = np.random.RandomState(seed)
        self.g = {k: rs.standard_normal(self.pd[k].shape) for k in KEYS}           # every row, the ones behind the points too
        self.d_g = {k: _dev(torch, self.g[k], torch.float64) for k in KEYS}

    def single(self, torch, g):
        """graph g alone, with its slices of the diagrams (and of the gradients, if any)"""
        one = Batch(torch, [self.graphs[g]], [self.f[self.no[g]:self.no[g + 1]]], forward=False)
        rows = {"up": slice(self.no[g], self.no[g + 1]), "down": slice(self.no[g], self.no[g + 1]), "one": slice(self.eo[g], self.eo[g + 1]),
                "ext0": slice(g, g + 1), "counts": slice(g, g + 1)}
        pad = lambda a: a if len(a) else np.zeros((1,) + a.shape[1:], dtype=a.dtype)
        one.pd = {k: pad(self.pd[k][rows[k]]) for k in rows}
        one.d_pd = {k: _dev(torch, one.pd[k], torch.int32 if k == "counts" else torch.float64) for k in rows}
        if hasattr(self, "g"):
            one.g = {k: pad(self.g[k][rows[k]]) for k in KEYS}
            one.d_g = {k: _dev(torch, one.g[k], torch.float64) for k in KEYS}
        return one


def same_ids(ids, ref, ref_status):
    for k in KEYS:
        got = ids[k].cpu().numpy()
        want = ref[k][:len(got)]
        assert np.array_equal(got, want), (k, np.flatnonzero((got != want).any(1))[:8])
    assert np.array_equal(ids["status"].cpu().numpy(), ref_status)


@pytest.fixture(scope="module")
def world(torch_cuda):
    """the batch that mixes every class, once with distinct values (points of zero persistence dropped) and once with ties (kept);
    ids, the restatement and random point gradients of both -- computed once and left unchanged"""
    torch = torch_cuda
    graphs, named = cases.mixed_batch(seed=0)
    rs = np.random.RandomState(1)
    w = {"named": named}
    for label, flags in (("distinct", 0), ("ties", KEEP0)):
        if label == "distinct":
            fs = [cases.distinct_values(rs, n) for n, _ in graphs]
            fs[named["star64"]][0] = 0.999                     # the hub enters last: it is the death of every Ord0 point
        else:
            fs = [cases.tied_values(rs, n, g % 3) for g, (n, _) in enumerate(graphs)]
            for key in ("triangle", "n65", "n2047"):
                fs[named[key]] = cases.tied_values(rs, graphs[named[key]][0], 3)             # -0.0 and +0.0
            fs[named["n64"]] = cases.tied_values(rs, 64, 0)
            fs[named["n2048"]] = cases.tied_values(rs, 2048, 2)
        b = Batch(torch, graphs, fs, flags)
        b.ids = b.vertices(torch)
        b.ref, b.ref_status = cases.ref_vertices(b.no, b.eo, b.f, b.pd)
        b.random_grads(torch, 7)
        b.h_ids = {k: b.ids[k].cpu().numpy() for k in KEYS}
        b.ref_grad = cases.ref_grad(b.no, b.eo, b.pd["counts"], b.ref, b.ref_status, b.g)
        w[label] = b
    return w


# ---- 1. ids against the restatement -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", ["distinct", "ties"])
def test_ids_equal_the_restatement(torch_cuda, world, label):
    b, named = world[label], world["named"]
    assert b.B > 4 * 2048, "more graphs than the wave tier's grid has wavefronts"
    c = b.pd["counts"]
    assert (c >= 0).all() and c[named["apart"], 3] == 3 and c[named["triangle"], 2] == 1 and c[named["empty"], :3].tolist() == [0, 0, 0]
    assert (b.ref_status == ST_OK).all()
    same_ids(b.ids, b.ref, b.ref_status)
    h = b.h_ids
    g = named["one"]                                                      # one node, no edge: no points, ext0 = [f, f], ids (0, 0)
    assert c[g, :3].tolist() == [0, 0, 0] and h["ext0"][g].tolist() == [0, 0] and (h["up"][b.no[g]] == -1).all()
    # rows behind the points hold -1, the rows of points an id (the restatement says the same; this is the direct statement)
    for key, offs, col in (("up", b.no, 0), ("down", b.no, 1), ("one", b.eo, 2)):
        row = np.arange(int(offs[-1])) - np.repeat(offs[:-1], np.diff(offs))
        is_point = row < np.repeat(c[:, col], np.diff(offs))
        ids = h[key][:int(offs[-1])]
        assert (ids[is_point] >= 0).all() and (ids[~is_point] == -1).all(), key
    if label == "ties":
        g = named["n64"]                                                  # all values equal: every id is 0
        assert (h["up"][b.no[g]:b.no[g] + c[g, 0]] == 0).all() and (h["one"][b.eo[g]:b.eo[g] + c[g, 2]] == 0).all()
        g = named["n65"]                                                  # a zero of either sign belongs to vertex 0 (-0.0)
        pts, ids = b.pd["up"][b.no[g]:b.no[g] + c[g, 0]], h["up"][b.no[g]:b.no[g] + c[g, 0]]
        assert np.signbit(b.f[b.no[g]]) and (pts == 0).any() and (ids[pts == 0] == 0).all()


# ---- 2. the large class -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def large(torch_cuda):
    torch = torch_cuda
    rs = np.random.RandomState(3)
    graphs = [(2049, cases.chord_graph(rs, 2049, 2049 + 700, "cycle")), (5000, cases.chord_graph(rs, 5000, 7500, "cycle"))]
    b = Batch(torch, graphs, [cases.distinct_values(rs, n) for n, _ in graphs], KEEP0, pd_large="device")
    b.ids = b.vertices(torch)
    b.ref, b.ref_status = cases.ref_vertices(b.no, b.eo, b.f, b.pd)
    b.random_grads(torch, 11)
    b.ref_grad = cases.ref_grad(b.no, b.eo, b.pd["counts"], b.ref, b.ref_status, b.g)
    return b


def test_large_class(torch_cuda, large):
    from tlc_gnn_amd import engine
    torch, b = torch_cuda, large
    assert (b.pd["counts"][:, 0] > 0).all() and (b.pd["counts"][:, 2] > 0).all()
    same_ids(b.ids, b.ref, b.ref_status)
    got = b.grad(torch, b.ids, b.d_g)
    assert np.array_equal(got, b.ref_grad)
    # neither the workspace nor the batch around a graph changes a bit
    roomy = torch.empty(2 * engine.pd_grad_work_bytes(5000, 7500) + 4096, dtype=torch.uint8, device="cuda")
    assert np.array_equal(b.grad(torch, b.vertices(torch, work=roomy[1:]), b.d_g, work=roomy[3:]), got)
    one = b.single(torch, 1)
    ids1 = one.vertices(torch)
    assert np.array_equal(ids1["one"].cpu().numpy(), b.ids["one"].cpu().numpy()[b.eo[1]:b.eo[2]])
    assert np.array_equal(one.grad(torch, ids1, one.d_g), got[b.no[1]:b.no[2]])
    # a coordinate of the first graph that none of its vertices holds: that graph alone is refused
    keep = b.d_pd
    b.d_pd = dict(keep, down=keep["down"].clone())
    b.d_pd["down"][5, 0] = 0.123456789
    try:
        ids2 = b.vertices(torch)
        res = b.grad(torch, ids2, b.d_g)
    finally:
        b.d_pd = keep
    assert ids2["status"].tolist() == [ST_BAD_INPUT, ST_OK] and ids2["down"][5].tolist() == [-1, int(b.ref["down"][5, 1])]
    for k in KEYS:
        a, r = ids2[k].cpu().numpy(), b.ref[k][:len(ids2[k])].copy()
        if k == "down":
            r[5, 0] = -1
        assert np.array_equal(a, r), k
    assert (res[:2049] == FILL).all() and np.array_equal(res[2049:], got[2049:])


def test_below_the_cut_2048_nodes_5000_edges(torch_cuda):
    """the forward's HUGE class (more than 4096 edges), this feature's workgroup class"""
    torch = torch_cuda
    rs = np.random.RandomState(4)
    graphs = [(2048, cases.chord_graph(rs, 2048, 5000, "cycle"))]
    b = Batch(torch, graphs, [cases.distinct_values(rs, 2048)], KEEP0, pd_large="host")
    assert b.pd["counts"][0, 2] == 5000 - 2047
    ids = b.vertices(torch)
    ref, ref_status = cases.ref_vertices(b.no, b.eo, b.f, b.pd)
    same_ids(ids, ref, ref_status)
    b.random_grads(torch, 5)
    assert np.array_equal(b.grad(torch, ids, b.d_g), cases.ref_grad(b.no, b.eo, b.pd["counts"], ref, ref_status, b.g))


# ---- 3. gradient bits -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", ["distinct", "ties"])
def test_gradient_bits(torch_cuda, world, label):
    torch, b, named = torch_cuda, world[label], world["named"]
    got = b.grad(torch, b.ids, b.d_g)
    assert np.array_equal(got, b.ref_grad)
    assert np.array_equal(b.grad(torch, b.ids, b.d_g), got)                       # a second run
    # gradients in rows behind the points change nothing
    c = b.pd["counts"]
    clean = {k: b.g[k].copy() for k in KEYS}
    for key, offs, col in (("up", b.no, 0), ("down", b.no, 1), ("one", b.eo, 2)):
        row = np.arange(int(offs[-1])) - np.repeat(offs[:-1], np.diff(offs))
        clean[key][:int(offs[-1])][row >= np.repeat(c[:, col], np.diff(offs))] = 0.0
    assert any((clean[k] != b.g[k]).any() for k in KEYS)
    assert np.array_equal(b.grad(torch, b.ids, {k: _dev(torch, clean[k], torch.float64) for k in KEYS}), got)
    # NULL gradient arguments count as zeros
    for drop in (("one",), ("up", "ext0"), KEYS):
        part = {k: (None if k in drop else b.g[k]) for k in KEYS}
        ref = cases.ref_grad(b.no, b.eo, c, b.ref, b.ref_status, part, which=[named[k] for k in ("triangle", "star64", "n65", "n2048")], fill=FILL)
        res = b.grad(torch, b.ids, {k: (None if k in drop else b.d_g[k]) for k in KEYS})
        for k in ("triangle", "star64", "n65", "n2048"):
            g = named[k]
            assert np.array_equal(res[b.no[g]:b.no[g + 1]], ref[b.no[g]:b.no[g + 1]]), (drop, k)
        zeros = {k: (torch.zeros_like(b.d_g[k]) if k in drop else b.d_g[k]) for k in KEYS}
        assert np.array_equal(b.grad(torch, b.ids, zeros), res)
    # single graphs taken out of the batch and run alone: one per class, and the star whose hub collects many coordinates
    for k in ("two", "star64", "n64", "n65", "n2048"):
        g = named[k]
        one = b.single(torch, g)
        ids1 = one.vertices(torch)
        assert np.array_equal(ids1["up"].cpu().numpy()[:one.graphs[0][0]], b.h_ids["up"][b.no[g]:b.no[g + 1]]), k
        assert np.array_equal(one.grad(torch, ids1, one.d_g), got[b.no[g]:b.no[g + 1]]), k
    g = named["star64"]
    assert label == "ties" or (b.h_ids["up"][b.no[g]:b.no[g + 1]] == 0).sum() >= 62


# ---- 4. the ids are the true critical vertices ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(12, 20), (70, 105)])
def test_ids_are_the_critical_vertices(torch_cuda, n, m):
    """Exact finite differences.  f is a permutation of k / 1024 and the step 2^-12 is below half the gap (the key perturbation
    (min + 1) * 1e-6 too), so no simplex changes its place in either order and every number is exact in fp64:
    point(f + eps e_v) - point(f) == eps * [vertex == v], coordinate by coordinate."""
    torch = torch_cuda
    rs = np.random.RandomState(n)
    E = cases.chord_graph(rs, n, m)
    f0 = rs.permutation(n) / 1024.0
    eps = 2.0 ** -12
    fs = [f0] + [f0 + eps * (np.arange(n) == v) for v in range(n)]
    b = Batch(torch, [(n, E)] * (n + 1), fs, KEEP0)
    ids = {k: t.cpu().numpy() for k, t in b.vertices(torch).items()}
    assert (ids["status"] == ST_OK).all()
    c = b.pd["counts"]
    assert (c == c[0]).all() and c[0, 0] == n - 1 and c[0, 2] == m - n + 1
    seen = 0
    for key, offs, col in (("up", b.no, 0), ("down", b.no, 1), ("one", b.eo, 2), ("ext0", np.arange(n + 2), None)):
        k = 1 if col is None else c[0, col]
        base_pts, base_ids = b.pd[key][offs[0]:offs[0] + k], ids[key][offs[0]:offs[0] + k]
        assert (base_ids >= 0).all()
        for v in range(n):
            moved = b.pd[key][offs[v + 1]:offs[v + 1] + k]
            assert np.array_equal(moved - base_pts, eps * (base_ids == v)), (key, v)
            assert np.array_equal(ids[key][offs[v + 1]:offs[v + 1] + k], base_ids), (key, v)
        seen += base_ids.size
    assert seen == 2 * (2 * (n - 1) + (m - n + 1) + 1)


# ---- 5. gradcheck -----------------------------------------------------------------------------------------------------------------
def test_gradcheck(torch_cuda):
    from tlc_gnn_amd import autograd
    torch = torch_cuda
    rs = np.random.RandomState(8)
    E = cases.chord_graph(rs, 8, 11)
    f = _dev(torch, rs.permutation(8) * 0.013 + 0.1 + rs.random_sample(8) * 0.005, torch.float64).requires_grad_(True)   # gaps >= 8e-3
    no, eo = _dev(torch, [0, 8], torch.int64), _dev(torch, [0, 11], torch.int64)
    d_E = _dev(torch, E, torch.int32)
    out = autograd.extended_persistence(f, no, eo, d_E)
    assert len(out) == 5 and not out[4].requires_grad and out[4].dtype == torch.int32 and all(o.requires_grad for o in out[:4])
    for i in range(4):
        assert torch.autograd.gradcheck(lambda x: autograd.extended_persistence(x, no, eo, d_E)[i], (f,), eps=1e-6, atol=1e-7, rtol=0,
                                        nondet_tol=0.0), i


# ---- 6. composition and use -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def some(torch_cuda):
    """60 small graphs and three larger ones with distinct values"""
    rs = np.random.RandomState(21)
    graphs = [(n, cases.small_graph(rs, n)) for n in rs.randint(2, 17, size=60).tolist()]
    graphs += [(n, cases.chord_graph(rs, n, n + n // 2)) for n in (40, 65, 130)]
    return Batch(torch_cuda, graphs, [cases.distinct_values(rs, n) for n, _ in graphs], KEEP0)


def test_packed_points_and_diagrams(torch_cuda, some):
    from tlc_gnn_amd import autograd, topo
    torch, b = torch_cuda, some
    c = b.pd["counts"]
    d = topo.diagrams(b.d_f, b.d_no, b.d_eo, b.d_E)
    assert torch.equal(d["counts"], b.d_pd["counts"]) and torch.equal(d["ext0"], b.d_pd["ext0"])
    for key, src, offs, col in (("ord0", "up", b.no, 0), ("rel1", "down", b.no, 1), ("ext1", "one", b.eo, 2)):
        want = np.concatenate([b.pd[src][offs[g]:offs[g] + c[g, col]] for g in range(b.B)])            # the Python-loop slice
        pts, po = autograd.packed_points(b.d_pd[src], _dev(torch, offs, torch.int64), b.d_pd["counts"][:, col])
        assert np.array_equal(pts.cpu().numpy(), want) and np.array_equal(po.cpu().numpy(), np.concatenate([[0], np.cumsum(c[:, col])]))
        assert np.array_equal(d[key].cpu().numpy(), want) and torch.equal(d[key + "_offs"], po)
    # the packing is differentiable: every packed row sends its gradient to its slot row, every other row gets none
    x = b.d_pd["one"].clone().requires_grad_(True)
    pts, _ = autograd.packed_points(x, b.d_eo, b.d_pd["counts"][:, 2])
    w = torch.arange(1, pts.numel() + 1, dtype=torch.float64, device="cuda").reshape(-1, 2)
    (pts * w).sum().backward()
    want = np.zeros(x.shape)
    at = np.concatenate([np.arange(b.eo[g], b.eo[g] + c[g, 2]) for g in range(b.B)])
    want[at] = w.cpu().numpy()
    assert np.array_equal(x.grad.cpu().numpy(), want)


@pytest.mark.parametrize("which", ["ord0+ext1", "ord0", "ext1"])
def test_images_equal_todays_route(torch_cuda, some, which):
    from tlc_gnn_amd import engine, topo
    torch, b = torch_cuda, some
    c = b.pd["counts"]
    parts = []
    for g in range(b.B):
        d0, d1 = b.pd["up"][b.no[g]:b.no[g] + c[g, 0]], b.pd["one"][b.eo[g]:b.eo[g] + c[g, 2]]
        parts.append(np.concatenate([d0, d1]) if which == "ord0+ext1" else d0 if which == "ord0" else d1)
    offs = np.concatenate([[0], np.cumsum([len(p) for p in parts])])
    want = engine.pi_raster(_dev(torch, offs, torch.int64), _dev(torch, np.concatenate(parts), torch.float64), 5)
    f = b.d_f.clone().requires_grad_(True)
    img = topo.images(f, b.d_no, b.d_eo, b.d_E, which=which)
    assert img.shape == (b.B, 25) and img.requires_grad
    assert float((img.detach() - want).abs().max()) <= 1e-11
    img.sum().backward()
    assert bool(torch.isfinite(f.grad).all()) and float(f.grad.abs().max()) > 0


def test_training_smoke(torch_cuda):
    """a 32-cycle: the one Ext1 point is [min f, max f]; minimising its persistence pulls the two ends together"""
    from tlc_gnn_amd import topo
    torch = torch_cuda
    n = 32
    E = _dev(torch, np.stack([np.arange(n), (np.arange(n) + 1) % n], 1), torch.int32)
    no, eo = _dev(torch, [0, n], torch.int64), _dev(torch, [0, n], torch.int64)
    f = _dev(torch, cases.distinct_values(np.random.RandomState(2), n), torch.float64).requires_grad_(True)
    opt = torch.optim.Adam([f], lr=0.02)
    losses = []
    for _ in range(50):
        opt.zero_grad()
        d = topo.diagrams(f, no, eo, E)
        assert d["ext1"].shape == (1, 2)
        loss = (d["ext1"][:, 1] - d["ext1"][:, 0]).sum()
        loss.backward()
        assert bool(torch.isfinite(f.grad).all()) and int((f.grad != 0).sum()) == 2
        losses.append(float(loss.detach()))
        opt.step()
    final = float((f.max() - f.min()).detach())
    assert abs(losses[0] - float(np.ptp(cases.distinct_values(np.random.RandomState(2), n)))) < 1e-15
    assert final < 0.5 * losses[0], (losses[0], final)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_wasserstein_to(torch_cuda, some, dtype):
    from tlc_gnn_amd import topo
    torch, b = torch_cuda, some
    dt = getattr(torch, dtype)
    rs = np.random.RandomState(5)
    k = rs.randint(1, 5, size=b.B)
    lo = rs.random_sample(int(k.sum())) * 0.5
    target = _dev(torch, np.stack([lo, lo + 0.1 + rs.random_sample(len(lo)) * 0.4], 1), torch.float64)
    toffs = _dev(torch, np.concatenate([[0], np.cumsum(k)]), torch.int64)
    f = b.d_f.to(dt).clone().requires_grad_(True)
    for which in ("ord0+ext1", "ext1"):
        loss = topo.wasserstein_to(f, b.d_no, b.d_eo, b.d_E, target, toffs, which=which)
        assert loss.shape == (b.B,) and loss.dtype == dt and bool(torch.isfinite(loss).all()) and float(loss.detach().min()) >= 0
        f.grad = None
        loss.sum().backward()
        assert f.grad.dtype == dt and bool(torch.isfinite(f.grad).all()) and float(f.grad.abs().max()) > 0


# ---- 7. refusals on the device ----------------------------------------------------------------------------------------------------
def _others_unchanged(b, world_b, ids, grad, bad):
    keep_n = np.ones(len(b.f), dtype=bool)
    keep_n[b.no[bad]:b.no[bad + 1]] = False
    keep_m = np.ones(int(b.eo[-1]), dtype=bool)
    keep_m[b.eo[bad]:b.eo[bad + 1]] = False
    for k, keep in (("up", keep_n), ("down", keep_n), ("one", keep_m)):
        assert np.array_equal(ids[k].cpu().numpy()[:len(keep)][keep], world_b.h_ids[k][:len(keep)][keep]), k
    st = ids["status"].cpu().numpy()
    assert st[bad] == ST_BAD_INPUT and (np.delete(st, bad) == ST_OK).all()
    want = world_b.ref_grad.copy()
    want[b.no[bad]:b.no[bad + 1]] = FILL                                           # the refused graph's slice is left untouched
    assert np.array_equal(grad, want)


@pytest.mark.parametrize("what", ["foreign", "nan"])
@pytest.mark.parametrize("key", ["n2047", "star64"])
def test_a_coordinate_no_vertex_holds(torch_cuda, world, what, key):
    torch, w = torch_cuda, world["distinct"]
    bad = world["named"][key]
    b = Batch(torch, w.graphs, [w.f[w.no[g]:w.no[g + 1]] for g in range(w.B)], forward=False)
    b.d_pd = {k: w.d_pd[k].clone() for k in KEYS + ("counts",)}
    row = int(w.no[bad]) + 1                                                       # a point row of the graph: it has more than two points
    assert w.pd["counts"][bad, 0] > 2
    b.d_pd["up"][row, 1] = float("nan") if what == "nan" else 0.123456789
    b.pull()
    ids = b.vertices(torch)
    assert ids["up"][row].tolist() == [int(w.h_ids["up"][row, 0]), -1]
    _others_unchanged(b, w, ids, b.grad(torch, ids, w.d_g), bad)


def test_offsets_out_of_order(torch_cuda, world):
    torch, w = torch_cuda, world["distinct"]
    b = Batch(torch, w.graphs, [w.f[w.no[g]:w.no[g + 1]] for g in range(w.B)], forward=False)
    b.d_pd = w.d_pd
    b.pull()
    b.d_no = b.d_no.clone()
    b.d_no[-1] = b.d_no[-2] - 5                                                    # the last graph ends before it starts
    ids = b.vertices(torch)
    bad = w.B - 1
    assert (ids["up"][w.no[bad]:].cpu().numpy() == SENTINEL).all()                 # nothing written for it
    _others_unchanged(b, w, ids, b.grad(torch, ids, w.d_g), bad)


def test_above_the_host_cap(torch_cuda):
    from tlc_gnn_amd import autograd
    torch = torch_cuda
    n = 65536
    E = np.stack([np.arange(n - 1), np.arange(1, n)], 1)
    f = cases.distinct_values(np.random.RandomState(6), n)
    b = Batch(torch, [(n, E)], [f], KEEP0, pd_large="host")
    assert (b.pd["counts"] == -1).all()
    ids = b.vertices(torch)
    assert ids["status"].tolist() == [ST_TOO_LARGE]
    assert all((ids[k] == SENTINEL).all() for k in KEYS)                           # rows untouched
    b.random_grads(torch, 1)
    assert (b.grad(torch, ids, b.d_g) == FILL).all()
    with pytest.raises(RuntimeError, match=r"graph\(s\) \[0\]"):
        autograd.extended_persistence(b.d_f, b.d_no, b.d_eo, b.d_E, pd_large="host")
    # the same path on the whole device is computed
    x = b.d_f.clone().requires_grad_(True)
    up, down, one, ext0, counts = autograd.extended_persistence(x, b.d_no, b.d_eo, b.d_E, pd_large="device")
    assert counts.tolist() == [[n - 1, n - 1, 0, 1]]
    (up[:n - 1, 1] - up[:n - 1, 0]).sum().backward()
    big = Batch(torch, [(n, E)], [f], KEEP0, pd_large="device")
    ids = big.vertices(torch)
    assert ids["status"].tolist() == [ST_OK]
    v = ids["up"].cpu().numpy()[:n - 1]
    assert (v >= 0).all() and np.array_equal(f[v], big.pd["up"][:n - 1]) and (ids["up"][n - 1:] == -1).all()
    want = np.zeros(n)
    np.add.at(want, v[:, 1], 1.0)
    np.add.at(want, v[:, 0], -1.0)
    assert np.array_equal(x.grad.cpu().numpy(), want)                              # sums of +-1: exact in any order

"""GPU: the derivative of the heat-kernel signature in its diffusion time -- tlc_hks_batch_dt (csrc/hks.hip, the Jacobi tiers),
tlc_hks_large_batch_dt (csrc/hks_large.hip), `autograd.hks_signature`, `topo.hks_filtration` -- against the numpy restatement of
tests/hks_dt_cases.py (checked on the CPU by tests/test_cpu_hks_dt_host.py).

Bounds.  Raw derivative: 2e-11 absolute -- the project's tested bound of 1e-11 on the values times the largest eigenvalue, 2 (the
derivative is the value's sum with every term multiplied by -lambda_k, 0 <= lambda_k <= 2).  Normalised derivative: 1e-10 / mx, see
test_normalised_derivative.  The same graph through both entries: 4e-11, twice the raw bound."""
import numpy as np
import pytest

import hks_dt_cases as hc

pytestmark = pytest.mark.gpu

RAW_BOUND = 2e-11
JACOBI_SIZES = (1, 2, 3, 32, 33, 64, 65, 96, 97, 256)
JACOBI_TIMES = (0.0, 0.1, 10.0)
LARGE_SIZES = (257, 320, 321, 1025)
LARGE_TIMES = (0.0, 0.1, 0.5, 0.75, 1.5, 10.0, 64.0)        # 0.1, 0.5: no scaling, the diagonal; 0.75: one halving, no squaring


def _shapes(n, seed):
    out = [("K%d" % n, hc.complete(n)), ("star%d" % n, hc.star(n)), ("path+2iso%d" % n, hc.path_plus_isolated(n)),
           ("G(%d,0.1)" % n, hc.gnp(n, 0.1, seed + n))]
    if n >= 3:
        out.append(("C%d" % n, hc.cycle(n)))
    return out


_PAIRS = {}


def _oracle(name, graph, t):
    """(value, derivative) of the eigen form; one eigh per named graph, shared by all tests and left unchanged"""
    if name not in _PAIRS:
        _PAIRS[name] = hc.eigenpairs(*graph)
    return hc.eigen_form(graph[0], graph[1], t, _PAIRS[name])


def _cuda(graphs):
    import torch
    node_ptr, edge_ptr, edges = hc.pack(graphs)
    return torch.from_numpy(node_ptr).cuda(), torch.from_numpy(edge_ptr).cuda(), torch.from_numpy(edges).cuda(), node_ptr


def _jacobi(graphs, times, normalise, dt=True):
    from tlc_gnn_amd import engine
    no, eo, E, nptr = _cuda(graphs)
    return engine.hks_batch(no, eo, E, list(times), normalise=normalise, total_nodes=int(nptr[-1]), dt=dt) + (nptr,)


def _large(graphs, times, normalise, sel=None, sel_nodes=None, dt=True, fill=None, work_bytes=None):
    """engine.hks_large_batch on every graph (or `sel`); fill: out and dout start as this value instead of NaN"""
    import torch
    from tlc_gnn_amd import engine
    no, eo, E, nptr = _cuda(graphs)
    sel = list(range(len(graphs))) if sel is None else sel
    sel_nodes = [graphs[k][0] for k in sel] if sel_nodes is None else sel_nodes
    kw = dict(normalise=normalise, total_nodes=int(nptr[-1]), work_bytes=work_bytes)
    if fill is not None:
        kw["out"] = torch.full((len(times), int(nptr[-1])), fill, dtype=torch.float64, device="cuda")
        kw["status"] = torch.full((len(graphs),), 99, dtype=torch.uint8, device="cuda")
    if dt:
        kw["dout"] = True if fill is None else torch.full((len(times), int(nptr[-1])), fill, dtype=torch.float64, device="cuda")
    return engine.hks_large_batch(no, eo, E, sel, sel_nodes, list(times), **kw) + (nptr,)


def _bits(a, b):
    """the same bits (NaN sentinels included)"""
    import torch
    if a.dtype == torch.float64:
        return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))
    return torch.equal(a, b)


def _compare_raw(named, times, out, dout, nptr):
    """-> (worst |value - oracle|, worst |derivative - oracle|), with the edge cases asserted exactly"""
    out, dout = out.cpu().numpy(), dout.cpu().numpy()
    worst_v = worst_d = 0.0
    for g, (name, graph) in enumerate(named):
        n, e = graph
        deg = np.bincount(np.asarray(e).reshape(-1), minlength=n)
        for k, t in enumerate(times):
            val, dval = _oracle(name, graph, t)
            got_v, got_d = out[k, nptr[g]:nptr[g + 1]], dout[k, nptr[g]:nptr[g + 1]]
            assert np.isfinite(got_d).all() and np.isfinite(got_v).all(), (name, t)
            assert np.all(got_d[deg == 0] == 0.0) and np.all(got_v[deg == 0] == 1.0), (name, t)     # degree 0: exactly 1 and 0
            assert np.all(np.abs(got_d) <= 2.0 * got_v + RAW_BOUND), (name, t)
            if n:
                ev, ed = np.abs(got_v - val).max(), np.abs(got_d - dval).max()
                assert ed <= RAW_BOUND and ev <= 1e-11, (name, t, ev, ed)
                worst_v, worst_d = max(worst_v, ev), max(worst_d, ed)
    return worst_v, worst_d


def _jacobi_cases():
    return [c for n in JACOBI_SIZES for c in _shapes(n, 100)]


def _large_cases():
    cases = [c for n in LARGE_SIZES for c in _shapes(n, 200)]
    # small and empty graphs may be selected too (merely wasteful)
    cases[3:3] = [("G(5,0.5)", hc.gnp(5, 0.5, 7))]
    cases[9:9] = [("empty", (0, np.zeros((0, 2), dtype=np.int64)))]
    cases.append(("connected64", hc.random_connected(64, 8)))
    return cases


def test_raw_derivative_jacobi_tiers():
    """1. every tier edge (n = 32 | 33, 64 | 65, 96 | 97, 256) and n = 1, 2, 3; complete graphs, stars, cycles, a path with two isolated
    nodes, G(n, 0.1); t = 0 (every node of degree > 0: -1), 0.1, 10.  Measured on an MI355X: values 8.1e-14, derivative 8.2e-14."""
    from tlc_gnn_amd import _lib
    named = _jacobi_cases()
    out, dout, st, nptr = _jacobi([g for _, g in named], JACOBI_TIMES, normalise=False)
    assert bool((st == _lib.ST_OK).all())
    worst_v, worst_d = _compare_raw(named, JACOBI_TIMES, out, dout, nptr)
    print("jacobi tiers: worst |value - oracle| %.2e, worst |d/dt - oracle| %.2e" % (worst_v, worst_d))
    d0 = dout[0].cpu().numpy()
    for g, (name, (n, e)) in enumerate(named):
        deg = np.bincount(np.asarray(e).reshape(-1), minlength=n)
        assert np.abs(d0[nptr[g]:nptr[g + 1]][deg > 0] + 1.0).max(initial=0.0) <= RAW_BOUND, name
    # the closed forms, not only the oracle
    dn = dout.cpu().numpy()
    for g, (name, (n, e)) in enumerate(named):
        for k, t in enumerate(JACOBI_TIMES):
            got = dn[k, nptr[g]:nptr[g + 1]]
            if name.startswith("K"):
                assert np.abs(got - hc.d_complete(n, t)).max() <= RAW_BOUND, (name, t)
            elif name.startswith("star"):
                assert np.abs(got - hc.d_star(n, t)).max() <= RAW_BOUND, (name, t)
            elif name.startswith("C"):
                assert np.abs(got - hc.d_cycle(n, t)).max() <= RAW_BOUND, (name, t)


def test_raw_derivative_large_tier():
    """2. n = 257, 320 | 321 (a tile edge), 1 025; the same shapes plus a selected graph of 5, of 64 and of 0 nodes; t = 0, the diagonal
    path (0.1, 0.5), one halving without a squaring (0.75), and 1.5, 10, 64.  Measured on an MI355X: values 1.5e-13, derivative 1.2e-14."""
    from tlc_gnn_amd import _lib
    named = _large_cases()
    out, dout, st, nptr = _large([g for _, g in named], LARGE_TIMES, normalise=False)
    assert bool((st == _lib.ST_OK).all())
    worst_v, worst_d = _compare_raw(named, LARGE_TIMES, out, dout, nptr)
    print("large tier: worst |value - oracle| %.2e, worst |d/dt - oracle| %.2e" % (worst_v, worst_d))
    d0 = dout[0].cpu().numpy()                                          # t = 0 is answered directly: exactly -1 or 0
    for g, (name, (n, e)) in enumerate(named):
        deg = np.bincount(np.asarray(e).reshape(-1), minlength=n)
        assert np.array_equal(d0[nptr[g]:nptr[g + 1]], np.where(deg > 0, -1.0, 0.0)), name


def test_star_of_4095_leaves_at_the_largest_time():
    """2. K(1, 4095) at t = 64 against the closed form: the largest graph, six squarings, a centre whose derivative is a sum over
    4 095 neighbours that cancels -[K]_vv = -1/2 to exp(-128).  Measured: 7.2e-16."""
    from tlc_gnn_amd import _lib
    n, e = hc.star(4096)
    out, dout, st, _ = _large([(n, e)], [64.0], normalise=False)
    assert int(st[0]) == _lib.ST_OK
    err = np.abs(dout[0].cpu().numpy() - hc.d_star(n, 64.0)).max()
    print("K(1,4095), t = 64: worst |d/dt - closed form| %.2e" % err)
    assert err <= RAW_BOUND


def _normalised_cases_jacobi():
    return [("connected%d" % n, hc.random_connected(n, 300 + n)) for n in (33, 97, 256)] + \
           [("K32", hc.complete(32)), ("K65", hc.complete(65)), ("C64", hc.cycle(64)), ("C97", hc.cycle(97))]


def _normalised_cases_large():
    return [("connected300", hc.random_connected(300, 600)), ("K257", hc.complete(257)), ("C320", hc.cycle(320))]


def _compare_normalised(named, times, out, dout, nptr, factor=1.0):
    out, dout = out.cpu().numpy(), dout.cpu().numpy()
    worst = 0.0
    for g, (name, graph) in enumerate(named):
        for k, t in enumerate(times):
            val, dval = _oracle(name, graph, t)
            f, df = hc.quotient(val, dval)
            err = np.abs(dout[k, nptr[g]:nptr[g + 1]] - df).max() * val.max()
            assert np.abs(out[k, nptr[g]:nptr[g + 1]] - f).max() <= 1e-11, (name, t)
            assert err <= factor * 1e-10, (name, t, err)
            worst = max(worst, err)
    return worst


def test_normalised_derivative():
    """3. d f / d t = (hks'(v) - f(v) hks'(a)) / (mx + 1e-10) against the oracle's quotient rule, bound 1e-10 / mx with mx the oracle's
    largest raw value of the graph:
      numerator    hks'(v) to 2e-11, f(v) hks'(a): |f| <= 1 times 2e-11, plus |hks'(a)| <= 2 mx <= 2 (mx <= 1) times the error of f --
                   that of the value over mx, 1e-11 / mx, taken before the division below: 2e-11 + 2e-11 + 2e-11 = 6e-11 over mx;
      denominator  mx to 1e-11, i.e. a relative 1e-11 / mx on a result of at most (2 mx + 2 mx) / mx = 4: 4e-11 over mx.
    Random connected graphs (the maximum is attained once or at symmetric nodes), and K_n and C_n, where every node ties and the first
    index of the computed maximum decides: by symmetry hks'(a) is the same at every a.  Measured (error times mx): 3.8e-15 (Jacobi), 2.8e-15 (large)."""
    from tlc_gnn_amd import _lib
    times = (0.1, 10.0)
    named = _normalised_cases_jacobi()
    out, dout, st, nptr = _jacobi([g for _, g in named], times, normalise=True)
    assert bool((st == _lib.ST_OK).all())
    wj = _compare_normalised(named, times, out, dout, nptr)
    named = _normalised_cases_large()
    out, dout, st, nptr = _large([g for _, g in named], times + (1.5,), normalise=True)
    assert bool((st == _lib.ST_OK).all())
    wl = _compare_normalised(named, times + (1.5,), out, dout, nptr)
    print("normalised: worst |d f/dt - oracle| * mx: jacobi %.2e, large %.2e" % (wj, wl))


def test_ties_take_the_first_index():
    """3. two isolated nodes tie at exactly 1.0 = mx: a = the first of them, hks'(a) = 0, so the normalised derivative is the raw one
    over (1 + 1e-10) bit for bit -- in both tiers"""
    import torch
    for run, graphs, t in ((_jacobi, [hc.path_plus_isolated(40)], (0.5,)), (_large, [hc.path_plus_isolated(300)], (0.5, 3.0))):
        raw = run(graphs, t, normalise=False)
        nrm = run(graphs, t, normalise=True)
        assert torch.equal(nrm[1], raw[1] / (1.0 + 1e-10))
        assert torch.equal(nrm[0], raw[0] / (1.0 + 1e-10))


def test_same_graph_through_both_entries():
    """4. a 200-node and a 256-node graph through the Jacobi tier and the large tier: two independent algorithms, derivatives within
    4e-11 (raw; normalised 2e-10 / mx).  Measured: 4.2e-14 raw."""
    graphs = [hc.random_connected(200, 41, extra=400), hc.random_connected(256, 42, extra=500)]
    times = (0.1, 10.0)
    worst = 0.0
    for normalise in (False, True):
        a, da, _, nptr = _jacobi(graphs, times, normalise)
        b, db, _, _ = _large(graphs, times, normalise)
        diff = (da - db).abs().cpu().numpy()
        for g in range(2):
            scale = 1.0
            if normalise:
                scale = 5.0 / max(_oracle("both%d" % g, graphs[g], t)[0].max() for t in times)
            assert diff[:, nptr[g]:nptr[g + 1]].max() <= 4e-11 * scale
        if not normalise:
            worst = diff.max()
    print("both entries: worst raw |d/dt jacobi - d/dt large| %.2e" % worst)


def _refused_batch():
    """[ok, TOO_LARGE for the Jacobi entry (300 nodes), BAD_INPUT (edge (0, 1) twice), ok]"""
    rep = (20, np.concatenate([hc.cycle(20)[1], np.array([[1, 0]])]))
    return [hc.random_connected(50, 1), hc.cycle(300), rep, hc.random_connected(120, 2)]


def test_values_and_status_are_the_parents_bits():
    """5. d_out and d_status of both _dt entries are the parent entries' bit for bit, with and without TLC_HKS_NORMALISE; a TOO_LARGE
    and a BAD_INPUT graph keep the sentinel in both of their slices"""
    import torch
    from tlc_gnn_amd import _lib
    times = (0.1, 10.0, 0.0)
    graphs = [g for _, g in _jacobi_cases()] + _refused_batch()
    B = len(graphs)
    for normalise in (False, True):
        out, dout, st, nptr = _jacobi(graphs, times, normalise)
        out0, st0, _ = _jacobi(graphs, times, normalise, dt=False)
        assert _bits(out, out0) and torch.equal(st, st0)
        assert st[B - 3].item() == _lib.ST_TOO_LARGE and st[B - 2].item() == _lib.ST_BAD_INPUT and st[B - 1].item() == _lib.ST_OK
        for g in (B - 3, B - 2):
            assert bool(torch.isnan(out[:, nptr[g]:nptr[g + 1]]).all()) and bool(torch.isnan(dout[:, nptr[g]:nptr[g + 1]]).all())
        ok = torch.ones(int(nptr[-1]), dtype=torch.bool)
        ok[nptr[B - 3]:nptr[B - 1]] = False
        assert bool(torch.isfinite(dout[:, ok.cuda()]).all())
    # large entry: [ok, BAD_INPUT (a repeated edge), TOO_LARGE (5 000 nodes), not selected, ok]
    rep = (300, np.concatenate([hc.cycle(300)[1], np.array([[5, 4]])]))
    graphs = [hc.random_connected(257, 3), rep, hc.path_plus_isolated(5000), hc.cycle(270), hc.cycle(320)]
    sel = [0, 1, 2, 4]
    for normalise in (False, True):
        out, dout, st, nptr = _large(graphs, times, normalise, sel=sel, fill=-7.0)
        out0, st0, _ = _large(graphs, times, normalise, sel=sel, fill=-7.0, dt=False)
        assert _bits(out, out0) and torch.equal(st, st0)
        assert st.tolist() == [_lib.ST_OK, _lib.ST_BAD_INPUT, _lib.ST_TOO_LARGE, 99, _lib.ST_OK]
        for g in (1, 2, 3):
            assert bool((out[:, nptr[g]:nptr[g + 1]] == -7.0).all()) and bool((dout[:, nptr[g]:nptr[g + 1]] == -7.0).all())
        for g in (0, 4):
            assert bool(torch.isfinite(dout[:, nptr[g]:nptr[g + 1]]).all()) and bool((dout[:, nptr[g]:nptr[g + 1]] != -7.0).all())


def _many_small(count, seed):
    rs = np.random.RandomState(seed)
    return [hc.random_connected(int(n), int(s)) for n, s in zip(rs.randint(3, 41, size=count), rs.randint(1 << 30, size=count))]


def test_derivative_bits_do_not_depend_on_the_batch():
    """6. d_dout is the same bits run to run; for a graph alone and inside a batch larger than every grid (3 000 graphs of 3 .. 40
    nodes, 50 of them compared); for eight times at once and each time alone; in the large tier with min_bytes and with all_bytes"""
    import torch
    from tlc_gnn_amd import engine
    times = (0.0, 0.01, 0.1, 0.5, 1.0, 3.0, 10.0, 64.0)
    graphs = _many_small(3000, 17)
    for normalise in (True, False):
        out, dout, st, nptr = _jacobi(graphs, times, normalise)
        again = _jacobi(graphs, times, normalise)
        assert _bits(dout, again[1]) and _bits(out, again[0])
        assert bool(torch.isfinite(dout).all())
        if normalise:
            for k, t in enumerate(times):                                # row k is a call with times[k] alone
                one = _jacobi(graphs, (t,), normalise)
                assert _bits(one[1][0], dout[k]) and _bits(one[0][0], out[k]), t
        for g in np.random.RandomState(3).choice(len(graphs), 50, replace=False):
            alone = _jacobi([graphs[g]], times, normalise)
            assert _bits(alone[1], dout[:, nptr[g]:nptr[g + 1]]), g
    # the large tier: groups that fit the smallest workspace against all graphs at once; eight times against each alone
    graphs = [hc.random_connected(257, 5), hc.gnp(400, 0.02, 6), hc.cycle(321), hc.random_connected(700, 7)]
    lo, hi = engine.hks_large_work_bytes([n for n, _ in graphs], len(times))
    assert lo < hi
    for normalise in (True, False):
        out, dout, st, nptr = _large(graphs, times, normalise, work_bytes=hi)
        for other in (_large(graphs, times, normalise, work_bytes=hi), _large(graphs, times, normalise, work_bytes=lo)):
            assert _bits(other[1], dout) and _bits(other[0], out)
        alone = _large(graphs[1:2], times, normalise)
        assert _bits(alone[1], dout[:, nptr[1]:nptr[2]])
    for k, t in enumerate(times):
        one = _large(graphs, (t,), False)
        assert _bits(one[1][0], dout[k]) and _bits(one[0][0], out[k]), t


def _mixed_batch():
    """six graphs of 5 .. 40 nodes and one of 300: both tiers in one call"""
    return [hc.random_connected(n, 900 + n) for n in (5, 12, 19, 26, 33, 40)] + [hc.random_connected(300, 77)]


@pytest.mark.parametrize("normalise", [False, True])
def test_gradcheck_in_the_times(normalise):
    """7. torch.autograd.gradcheck of autograd.hks_signature in `times` (float64, eps 1e-6, atol 1e-6): the central difference of
    values good to 1e-13 over 2e-6 is good to 1e-7"""
    import torch
    from tlc_gnn_amd import autograd
    no, eo, E, nptr = _cuda(_mixed_batch())
    times = torch.tensor([0.3, 2.5], dtype=torch.float64, device="cuda", requires_grad=True)
    out = autograd.hks_signature(times, no, eo, E, normalise=normalise)
    assert out.shape == (2, int(nptr[-1])) and out.dtype == torch.float64 and out.requires_grad
    assert torch.autograd.gradcheck(lambda t: autograd.hks_signature(t, no, eo, E, normalise=normalise), (times,), eps=1e-6, atol=1e-6)
    # any float dtype, any device for the times: the gradient comes back where and as they are
    t32 = torch.tensor([0.3, 2.5], dtype=torch.float32, requires_grad=True)
    o32 = autograd.hks_signature(t32, no, eo, E, normalise=normalise)
    o32.sum().backward()
    assert o32.dtype == torch.float64 and t32.grad.dtype == torch.float32 and t32.grad.device.type == "cpu"


def test_hks_filtration_forward_is_the_ground_truth_route():
    """8. topo.hks_filtration(t) equals data_utils_LP.hks_filtration_device(..., hks_large='device') bit for bit"""
    import torch
    from tlc_gnn_amd import topo
    from tlc_gnn_amd.Knowledge_Distillation import data_utils_LP as kd_lp
    no, eo, E, nptr = _cuda(_mixed_batch())
    for t in (0.1, 10.0):
        want = kd_lp.hks_filtration_device(no, eo, E, t, int(nptr[-1]), hks_large='device')
        assert kd_lp.hks_large_device == 1 and kd_lp.hks_host_fallback == 0
        for time in (torch.tensor(t, dtype=torch.float64), torch.tensor([t], dtype=torch.float64, device="cuda", requires_grad=True)):
            got = topo.hks_filtration(time, no, eo, E)
            assert got.shape == (int(nptr[-1]),) and _bits(got.detach(), want)


def test_learning_the_time_through_the_images():
    """8. target images made at t = 3 on 64 random graphs; from t = 1, 60 Adam steps on the squared image distance through
    topo.images(topo.hks_filtration(t, ...)): the loss falls and t moves towards 3"""
    import torch
    from tlc_gnn_amd import topo
    rs = np.random.RandomState(4)
    graphs = [hc.random_connected(int(n), 50 + i, extra=int(n) // 2) for i, n in enumerate(rs.randint(8, 25, size=64))]
    no, eo, E, _ = _cuda(graphs)
    with torch.no_grad():
        target = topo.images(topo.hks_filtration(torch.tensor(3.0, dtype=torch.float64), no, eo, E), no, eo, E)
    t = torch.tensor(1.0, dtype=torch.float64, device="cuda", requires_grad=True)
    opt = torch.optim.Adam([t], lr=0.05)
    losses = []
    for _ in range(60):
        opt.zero_grad()
        loss = ((topo.images(topo.hks_filtration(t, no, eo, E), no, eo, E) - target) ** 2).sum()
        loss.backward()
        assert t.grad is not None and bool(torch.isfinite(t.grad))
        opt.step()
        losses.append(float(loss.detach()))
    print("learned time: t 1 -> %.4f, loss %.4e -> %.4e" % (float(t), losses[0], losses[-1]))
    assert losses[-1] < losses[0] and abs(float(t) - 3.0) < 2.0


def test_signature_refusals():
    """8. no host fallback: a 5 000-node graph, a time of 70 with a large graph present and a repeated edge raise RuntimeError naming the
    graph; a time of 70 without a large graph is the Jacobi tiers' business and is computed"""
    import torch
    from tlc_gnn_amd import autograd, topo
    small = hc.random_connected(20, 1)
    one = torch.tensor([1.0], dtype=torch.float64)
    no, eo, E, _ = _cuda([small, hc.path_plus_isolated(5000)])
    with pytest.raises(RuntimeError, match=r"\[1\]"):
        autograd.hks_signature(one, no, eo, E)
    no, eo, E, _ = _cuda([small, hc.cycle(300), small])
    with pytest.raises(RuntimeError, match=r"\[1\]"):
        topo.hks_filtration(torch.tensor(70.0), no, eo, E)
    assert bool(torch.isfinite(topo.hks_filtration(torch.tensor(64.0), no, eo, E)).all())
    rep = (20, np.concatenate([hc.cycle(20)[1], np.array([[1, 0]])]))
    no, eo, E, _ = _cuda([small, small, rep])
    with pytest.raises(RuntimeError, match=r"\[2\]"):
        autograd.hks_signature(one, no, eo, E)
    no, eo, E, _ = _cuda([small])
    assert bool(torch.isfinite(autograd.hks_signature(torch.tensor([70.0]), no, eo, E)).all())

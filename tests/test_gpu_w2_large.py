"""GPU: the workspace tier of the matching Wasserstein loss (csrc/w2_large.hip; ops.w2_large_matching; `large='device'` of
ops.w2_partial_matching / ops.w2_inference_matching; autograd.diagram_loss(large=); topo.wasserstein_to(w2_large=);
Teacher_Model.forward(w2_large=)) against scipy's assignment solver (oracle/w2_ref.py), against the LDS kernels of csrc/w2_match.hip on
the same problems, and against itself across batches, slots and workspaces.  Tolerances: those of tests/test_gpu_train.py.

Point clouds are that file's `random` style (continuous coordinates: no tied costs, so the optimum and every output are unique); the
grid style only where ties are the point.  Above the cut of 4 096 rows every pair is balanced: a lopsided pair in the evaluation form
(4 100 against 50) is the tier's weak spot, millions of steps, and stays out of the suite.

What the cases cost on one MI355X (a step of the tier takes 4.4 us, DESIGN.md 6.12, so the shapes the cases are set at decide): the
scipy and LDS comparisons 2 - 6 s each, the cut 15 s (4 096 against 3 000 twice through the LDS kernel, 4 097 against 3 000 through the
tier, scipy on the host), the evaluation form above the cut 10 s, the forty problems on one slot 16 s, the teacher's 4 200-edge graph
52 s (an untrained model's points lie almost on one spot: its matching takes several million steps, twice)."""
import numpy as np
import pytest

from w2_checks import _check_inference, _check_training, _host, _pack, _pair

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2049)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _problems(infer, order):
    """every size of SIZES as the matrix dimension N (training form: N = n; evaluation form: N = n + m), m from 0 to n"""
    rs = np.random.RandomState(1000 + 10 * int(infer) + order)
    xs, ys = [], []
    for N in SIZES:
        for m in sorted({0, N // 3, N // 2, N} if N < 2049 else {0, N // 2, N}):
            n = N - m if infer else N
            X, Y = _pair(rs, n, m)
            xs.append(X); ys.append(Y)
    return xs, ys


_CACHE = {}


def _solved(torch, infer, order):
    """the problems, the tier's outputs with min_rows = -1 and scipy's optimum of every problem: computed once per (form, order)"""
    from tlc_gnn_amd import ops
    from oracle import w2_ref
    key = (infer, order)
    if key not in _CACHE:
        xs, ys = _problems(infer, order)
        xoff, yoff, dxo, dX, dyo, dY = _pack(torch, xs, ys)
        r = _host(ops.w2_large_matching(dxo, dX, dyo, dY, order=order, infer=infer, min_rows=-1, want_grad=True))
        ref = [(w2_ref.inference_matching if infer else w2_ref.partial_matching)(x, y, order) for x, y in zip(xs, ys)]
        for v in r.values():
            if v is not None:
                v.setflags(write=False)
        _CACHE[key] = dict(xs=xs, ys=ys, xoff=xoff, yoff=yoff, dev=(dxo, dX, dyo, dY), r=r, ref=ref)
    return _CACHE[key]


@pytest.mark.parametrize("order", [2, 1])
@pytest.mark.parametrize("infer", [False, True])
def test_against_scipy(torch_cuda, infer, order):
    """the entry alone, min_rows = -1 (every problem, the ones without rows too), one batch"""
    s = _solved(torch_cuda, infer, order)
    r, xoff, yoff = s["r"], s["xoff"], s["yoff"]
    assert (r["status"] == 0).all(), r["status"]
    for b, (Xb, Yb) in enumerate(zip(s["xs"], s["ys"])):
        sx, sy = slice(xoff[b], xoff[b + 1]), slice(yoff[b], yoff[b + 1])
        if infer:
            _check_inference(torch_cuda, Xb, Yb, order, r["assign_x"][sx], r["assign_y"][sy], r["loss"][b], r["wxy"][b], r["wxd"][b],
                             r["wyd"][b], r["grad"][sx], s["ref"][b])
        else:
            _check_training(torch_cuda, Xb, Yb, order, r["assign_x"][sx], r["loss"][b], r["wxy"][b], r["wxd"][b], r["grad"][sx], s["ref"][b][4])


@pytest.mark.parametrize("order", [2, 1])
@pytest.mark.parametrize("infer", [False, True])
def test_against_the_lds_kernels(torch_cuda, infer, order):
    """the same problems through the kernels of csrc/w2_match.hip: the loss to rounding, and at order 2 the same matching and gradient.
    At order 1 the optimum is not unique even on continuous coordinates -- where the death coordinate decides all four distances of two
    predicted and two target points, (Y1 - X1) + (Y2 - X2) = (Y2 - X1) + (Y1 - X2) -- and the two solvers, which start differently,
    return different optimal matchings (seen on the device: the training form of these problems); there the equal loss, which at
    order 1 is the cost itself, is what both being optimal means."""
    from tlc_gnn_amd import ops
    s = _solved(torch_cuda, infer, order)
    dxo, dX, dyo, dY = s["dev"]
    if infer:
        q = _host(ops.w2_inference_matching(dxo, dX, dyo, dY, order=order, want_grad=True))
        same = np.array_equal(q["assign_x"], s["r"]["assign_x"]) and np.array_equal(q["assign_y"], s["r"]["assign_y"])
    else:
        q = _host(ops.w2_partial_matching(dxo, dX, dyo, dY, order=order, want_grad=True))
        same = np.array_equal(q["assign"], s["r"]["assign_x"])
    assert (q["status"] == 0).all()
    rel = np.abs(q["loss"] - s["r"]["loss"]) / np.maximum(1.0, np.abs(q["loss"]))
    print("order %d: largest relative loss difference to the LDS kernels %.3g, same matching: %s" % (order, rel.max(), same))
    assert rel.max() <= 1e-12
    if order == 2:
        assert same
        assert np.abs(q["grad"] - s["r"]["grad"]).max() <= 1e-12
        if infer:
            assert np.abs(q["wyd"] - s["r"]["wyd"]).max() <= 1e-12


@pytest.mark.parametrize("infer", [False, True])
def test_ties(torch_cuda, infer):
    """grid coordinates, N about 300 and 1 100: many optimal assignments; the cost of the device's one is the optimum"""
    from tlc_gnn_amd import ops
    from oracle import w2_ref
    torch = torch_cuda
    rs = np.random.RandomState(77 + int(infer))
    xs, ys = [], []
    for N, m in ((300, 170), (1100, 500), (301, 0), (1100, 1100) if not infer else (1100, 550)):
        X, Y = _pair(rs, N - m if infer else N, m, "grid")
        xs.append(X); ys.append(Y)
    xoff, yoff, dxo, dX, dyo, dY = _pack(torch, xs, ys)
    for order in (2, 1):
        r = _host(ops.w2_large_matching(dxo, dX, dyo, dY, order=order, infer=infer, want_grad=True))
        assert (r["status"] == 0).all()
        for b, (Xb, Yb) in enumerate(zip(xs, ys)):
            sx, sy = slice(xoff[b], xoff[b + 1]), slice(yoff[b], yoff[b + 1])
            if infer:
                _check_inference(torch, Xb, Yb, order, r["assign_x"][sx], r["assign_y"][sy], r["loss"][b], r["wxy"][b], r["wxd"][b], r["wyd"][b],
                                 r["grad"][sx], w2_ref.inference_matching(Xb, Yb, order), unique=False)
            else:
                _check_training(torch, Xb, Yb, order, r["assign_x"][sx], r["loss"][b], r["wxy"][b], r["wxd"][b], r["grad"][sx],
                                w2_ref.partial_matching(Xb, Yb, order)[4], unique=False)


def test_the_cut_at_4096_rows(torch_cuda):
    """one batch around the cut through ops.w2_partial_matching(large='device'): the LDS kernels keep the problems of up to 4 096 rows,
    bit for bit, and the tier overwrites exactly those they refused"""
    from tlc_gnn_amd import ops
    from oracle import w2_ref
    torch = torch_cuda
    rs = np.random.RandomState(4096)
    sizes = [(4096, 3000), (4097, 3000), (40, 17), (0, 0), (4097, 0), (5, 9)]
    pairs = [_pair(rs, n, m) for n, m in sizes]
    xs, ys = [p[0] for p in pairs], [p[1] for p in pairs]
    xoff, yoff, dxo, dX, dyo, dY = _pack(torch, xs, ys)
    plain = _host(ops.w2_partial_matching(dxo, dX, dyo, dY, order=2))
    assert plain["status"].tolist() == [0, 2, 0, 0, 2, 1]                  # without `large`: status 2 as ever
    assert plain["loss"][1] == 0.0 and (plain["assign"][xoff[1]:xoff[2]] == -1).all()
    r = _host(ops.w2_partial_matching(dxo, dX, dyo, dY, order=2, large="device"))
    assert r["status"].tolist() == [0, 0, 0, 0, 0, 1]
    for b in (0, 2, 3, 5):
        sx = slice(xoff[b], xoff[b + 1])
        for k in ("loss", "wxy", "wxd", "status"):
            assert np.array_equal(r[k][b], plain[k][b]), (b, k)
        assert np.array_equal(r["assign"][sx], plain["assign"][sx]) and np.array_equal(r["grad"][sx], plain["grad"][sx]), b
    sx = slice(xoff[1], xoff[2])
    _check_training(torch, xs[1], ys[1], 2, r["assign"][sx], r["loss"][1], r["wxy"][1], r["wxd"][1], r["grad"][sx],
                    w2_ref.partial_matching(xs[1], ys[1], 2)[4])
    # 4 097 points against no target: every point to the diagonal
    d = (xs[4][:, 1] - xs[4][:, 0]) * 0.5
    assert (r["assign"][xoff[4]:xoff[5]] == -1).all() and abs(r["loss"][4] - np.sqrt((d ** 2).sum())) <= 1e-12 * r["loss"][4]
    assert r["wxy"][4] == 0.0 and r["wxd"][4] == r["loss"][4]
    # the same through autograd on the last three of them (4 097 against none is above the cut and costs no augmentation): refused
    # without the keyword, and the text names the cap that applies
    from tlc_gnn_amd import autograd
    xo, yo = torch.as_tensor(xoff[2:6] - xoff[2]).cuda(), torch.as_tensor(yoff[2:6] - yoff[2]).cuda()
    Xg = dX[xoff[2]:xoff[5]].clone().requires_grad_(True)
    Yg = dY[yoff[2]:yoff[5]]
    with pytest.raises(ValueError, match="4096"):
        autograd.diagram_loss(Xg, Yg, order=2, xoff=xo, yoff=yo)
    loss = autograd.diagram_loss(Xg, Yg, order=2, xoff=xo, yoff=yo, large="device")[0]
    assert np.array_equal(loss.detach().cpu().numpy(), r["loss"][2:5])
    loss.sum().backward()
    assert np.array_equal(Xg.grad.cpu().numpy(), r["grad"][xoff[2]:xoff[5]])


def test_the_evaluation_form_above_the_cut(torch_cuda):
    """2 049 + 2 048 points through ops.w2_inference_matching(large='device'), beside a small pair the LDS kernel keeps"""
    from tlc_gnn_amd import ops
    from oracle import w2_ref
    torch = torch_cuda
    rs = np.random.RandomState(2049)
    pairs = [_pair(rs, 2049, 2048), _pair(rs, 30, 41)]
    xs, ys = [p[0] for p in pairs], [p[1] for p in pairs]
    xoff, yoff, dxo, dX, dyo, dY = _pack(torch, xs, ys)
    plain = _host(ops.w2_inference_matching(dxo, dX, dyo, dY, order=2, want_grad=True))
    assert plain["status"].tolist() == [2, 0]
    r = _host(ops.w2_inference_matching(dxo, dX, dyo, dY, order=2, want_grad=True, large="device"))
    assert r["status"].tolist() == [0, 0]
    for k in ("loss", "wxy", "wxd", "wyd"):
        assert r[k][1] == plain[k][1], k
    assert np.array_equal(r["assign_x"][xoff[1]:], plain["assign_x"][xoff[1]:]) and np.array_equal(r["assign_y"][yoff[1]:], plain["assign_y"][yoff[1]:])
    assert np.array_equal(r["grad"][xoff[1]:], plain["grad"][xoff[1]:])
    _check_inference(torch, xs[0], ys[0], 2, r["assign_x"][:xoff[1]], r["assign_y"][:yoff[1]], r["loss"][0], r["wxy"][0], r["wxd"][0], r["wyd"][0],
                     r["grad"][:xoff[1]], w2_ref.inference_matching(xs[0], ys[0], 2))


@pytest.mark.parametrize("infer", [True])
def test_batch_slots_and_workspace_do_not_change_a_bit(torch_cuda, infer):
    """(The evaluation form only: the slots, the stride and the workspace are handled by code both forms share, and the one-slot run of
    forty problems, one after another, is what this test costs: 16 s measured, 41 s in the training form.)
    40 problems of 600 to 1 100 rows: one call on the least workspace (one slot: one after another), one call on a roomy one, on
    the default one, the roomy one again, and each problem alone: every output equal to the bit"""
    from tlc_gnn_amd import _lib, ops
    import ctypes as C
    torch = torch_cuda
    rs = np.random.RandomState(40 + int(infer))
    xs, ys = [], []
    for _ in range(40):
        N = int(rs.randint(600, 1101))
        m = int(rs.randint(N // 4, N // 2 + 1))
        X, Y = _pair(rs, N - m if infer else N, m)
        xs.append(X); ys.append(Y)
    xoff, yoff, dxo, dX, dyo, dY = _pack(torch, xs, ys)
    rows = max(len(x) + (len(y) if infer else 0) for x, y in zip(xs, ys))
    least = int(_lib.lib().tlc_w2_large_work_bytes(C.c_int64(rows), C.c_int32(1)))
    keys = ("loss", "wxy", "wxd", "assign_x", "grad", "status") + (("wyd", "assign_y") if infer else ())
    run = lambda nbytes: ops.w2_large_matching(dxo, dX, dyo, dY, order=2, infer=infer, want_grad=True,
                                               work=None if nbytes is None else torch.empty(nbytes, dtype=torch.uint8, device="cuda"))
    one = run(least)
    ctr = one["work"][:8 * _lib.W2_LARGE_COUNTERS].view(torch.int64).cpu().tolist()
    assert ctr[3] == 40 and ctr[0] >= ctr[1] > 0, ctr                     # one slot took all forty; steps >= augmentations
    one = _host(one)
    assert (one["status"] == 0).all()
    roomy = _host(run(40 * least + 12345))
    default = _host(run(None))
    again = _host(run(40 * least + 12345))
    for k in keys:
        assert np.array_equal(one[k], roomy[k]) and np.array_equal(one[k], default[k]) and np.array_equal(one[k], again[k]), k
    for b in range(40):
        sx, sy = slice(xoff[b], xoff[b + 1]), slice(yoff[b], yoff[b + 1])
        o = _pack(torch, [xs[b]], [ys[b]])
        alone = _host(ops.w2_large_matching(o[2], o[3], o[4], o[5], order=2, infer=infer, want_grad=True))
        for k in ("loss", "wxy", "wxd", "status") + (("wyd",) if infer else ()):
            assert np.array_equal(alone[k][0], one[k][b]), (b, k)
        assert np.array_equal(alone["assign_x"], one["assign_x"][sx]) and np.array_equal(alone["grad"], one["grad"][sx]), b
        if infer:
            assert np.array_equal(alone["assign_y"], one["assign_y"][sy]), b


def test_refusals(torch_cuda):
    from tlc_gnn_amd import _lib, ops
    import ctypes as C
    torch = torch_cuda
    rs = np.random.RandomState(3)
    # a NaN in one problem of a batch: status 3 there, its neighbours solved
    pairs = [_pair(rs, 700, 300), _pair(rs, 650, 650), _pair(rs, 90, 20), _pair(rs, 20, 30)]
    pairs[1][1][17, 0] = np.nan
    xs, ys = [p[0] for p in pairs], [p[1] for p in pairs]
    xoff, yoff, dxo, dX, dyo, dY = _pack(torch, xs, ys)
    good = [_pair(np.random.RandomState(3), 700, 300)]
    for infer in (False, True):
        r = _host(ops.w2_large_matching(dxo, dX, dyo, dY, order=2, infer=infer, want_grad=True))
        assert r["status"].tolist() == [0, 3, 0, 0 if infer else 1]
        assert np.isnan(r["loss"][1]) and np.isfinite(r["loss"][[0, 2]]).all() and (r["loss"][[0, 2]] > 0).all()
        assert (r["assign_x"][xoff[1]:xoff[2]] == -1).all() and np.abs(r["grad"][xoff[1]:xoff[2]]).max() == 0.0
        assert r["wxy"][1] == 0.0 and r["wxd"][1] == 0.0
        if infer:
            assert (r["assign_y"][yoff[1]:yoff[2]] == -1).all()
        else:
            assert r["loss"][3] == 0.0 and (r["assign_x"][xoff[3]:] == -1).all()          # n < m: loss 0, no matching
        o = _pack(torch, [good[0][0]], [good[0][1]])
        alone = _host(ops.w2_large_matching(o[2], o[3], o[4], o[5], order=2, infer=infer, want_grad=True))
        assert alone["loss"][0] == r["loss"][0] and np.array_equal(alone["assign_x"], r["assign_x"][:xoff[1]])
    # 65 537 points: status 2 at once (the call returns in well under the second a million steps would take), outputs defined
    big = [np.sort(rs.rand(65537, 2), axis=1)]
    o = _pack(torch, big + [xs[2]], [np.zeros((0, 2)), ys[2]])
    r = _host(ops.w2_large_matching(o[2], o[3], o[4], o[5], order=2, infer=False, want_grad=True))
    assert r["status"].tolist() == [2, 0] and r["loss"][0] == 0.0 and (r["assign_x"][:65537] == -1).all() and r["loss"][1] > 0
    r = _host(ops.w2_large_matching(o[2], o[3], o[4], o[5], order=1, infer=True, want_grad=True))
    assert r["status"].tolist() == [2, 0]
    # a workspace one byte short: the error code, and nothing is written
    need = int(_lib.lib().tlc_w2_large_work_bytes(C.c_int64(700), C.c_int32(1)))
    work = torch.zeros(need, dtype=torch.uint8, device="cuda")
    out = dict(loss=torch.full((4,), 7.0, dtype=torch.float64, device="cuda"), wxy=torch.full((4,), 7.0, dtype=torch.float64, device="cuda"),
               wxd=torch.full((4,), 7.0, dtype=torch.float64, device="cuda"), wyd=None,
               assign_x=torch.full((int(xoff[-1]),), 7, dtype=torch.int32, device="cuda"), assign_y=None,
               grad=torch.full((int(xoff[-1]), 2), 7.0, dtype=torch.float64, device="cuda"), status=torch.full((4,), 7, dtype=torch.uint8, device="cuda"))
    with pytest.raises(_lib.TlcError, match="tlc_w2_large_work_bytes"):
        ops.w2_large_matching(dxo, dX, dyo, dY, order=2, infer=False, work=work[:need - 1], _out=out)
    torch.cuda.synchronize()
    assert all(bool((v == 7).all()) for v in out.values() if v is not None) and not bool(work.any())
    ops.w2_large_matching(dxo, dX, dyo, dY, order=2, infer=False, work=work, _out=out)
    assert out["status"].cpu().tolist() == [0, 3, 0, 1]
    with pytest.raises(ValueError, match="refuse"):
        ops.w2_partial_matching(dxo, dX, dyo, dY, large="host")


# ---- through the stack ---------------------------------------------------------------------------------------------------------------
def test_topo_wasserstein_to_above_the_cut(torch_cuda):
    """one graph whose Ord0 + Ext1 diagram has more than 4 096 points against a target of the same size: its own diagram, every point
    moved by up to 0.01 (a balanced pair close to its target, like a model late in training)"""
    import pd_grad_cases as pg
    from tlc_gnn_amd import ops, topo
    torch = torch_cuda
    rs = np.random.RandomState(21)
    gs = [(1500, pg.chord_graph(rs, 1500, 4500))]
    no, eo, E, f = pg.pack(gs, [pg.distinct_values(rs, 1500)])
    dev = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda()
    no, eo, E, f = dev(no, torch.int64), dev(eo, torch.int64), dev(E, torch.int32), dev(f, torch.float64)
    pts, offs = topo._select(f, no, eo, E, "ord0+ext1", "host")
    k = int(offs[-1])
    assert k > 4096
    target = pts.detach() + dev(rs.uniform(-0.01, 0.01, size=(k, 2)), torch.float64)
    toffs = offs.clone()
    with pytest.raises(ValueError, match="4096"):
        topo.wasserstein_to(f, no, eo, E, target, toffs)
    fg = f.clone().requires_grad_(True)
    loss = topo.wasserstein_to(fg, no, eo, E, target, toffs, w2_large="device")
    assert loss.shape == (1,) and bool(torch.isfinite(loss).all()) and float(loss) > 0
    loss.sum().backward()
    assert fg.grad is not None and bool(torch.isfinite(fg.grad).all()) and float(fg.grad.abs().max()) > 0
    r = ops.w2_large_matching(offs, pts.detach(), toffs, target, order=2, infer=True, want_grad=False)
    assert int(r["status"][0]) == 0 and float(r["loss"][0]) == float(loss[0])


def _random_edges(rs, n, m, torch):
    s = rs.randint(0, n, size=4 * m); t = rs.randint(0, n, size=4 * m)
    keep = s != t
    e = np.unique(np.stack([s[keep], t[keep]]), axis=1)
    e = e[:, rs.permutation(e.shape[1])[:m]]
    assert e.shape[1] == m
    return torch.tensor(e, dtype=torch.int64)


def _rel(a, b):
    a = a.detach().cpu().double().reshape(-1); b = b.detach().cpu().double().reshape(-1)
    return float((a - b).abs().max() / max(1e-12, float(b.abs().max())))


def test_teacher_batch_with_a_graph_above_the_cut_equals_the_sum_over_its_graphs(torch_cuda):
    """Teacher_Model.forward(kernel='wasserstein', w2_large='device') on a block-diagonal batch of one 4 200-edge graph and two small
    ones: loss and parameter gradients are the sums over the three graphs run alone (tolerances of the batch test of
    tests/test_gpu_train.py: 1e-5 on the loss, 1e-4 on a gradient)."""
    from tlc_gnn_amd.Knowledge_Distillation.Teacher_model import Teacher_Model
    torch = torch_cuda
    torch.manual_seed(13)
    rs = np.random.RandomState(13)
    graphs, fs, pds = [], [], []
    for n, m, k in ((900, 4200, 3000), (30, 70, 70), (12, 20, 9)):
        graphs.append((n, _random_edges(rs, n, m, torch)))
        fs.append(torch.rand(n, 1))
        bb = rs.rand(k)
        pds.append(torch.tensor(np.stack([bb, bb + rs.uniform(0, 0.6, size=k)], 1), dtype=torch.float32))
    model = Teacher_Model(type='GAT', dropout=0.0)
    with torch.no_grad():
        for conv in (model.DIM0_Model.conv1, model.DIM0_Model.conv2, model.DIM0_Model.conv3, model.DIM0_Model.conv4):
            conv.bias.uniform_(-0.2, 0.2)
            torch.nn.init.xavier_uniform_(conv.lin_ij.weight)
    model = model.cuda().train()

    # the big graph's targets: what the untrained model predicts for it, every point moved by up to 0.02 -- a balanced pair close to its
    # target.  (An untrained model's points lie almost on one spot; against unrelated targets that is several million steps.)
    with torch.no_grad():
        n0, e0 = graphs[0]
        lp = torch.arange(n0, dtype=torch.int64)
        pred = model(fs[0].cuda(), torch.cat([e0, torch.stack([lp, lp])], dim=1).cuda(), pds[0].cuda(), compute_loss=False, grad_PI=False)[0]
    pds[0] = (pred.detach().cpu().float() + torch.tensor(rs.uniform(-0.02, 0.02, size=(e0.shape[1], 2)), dtype=torch.float32))

    def run(idx, **kw):
        gptr = np.concatenate([[0], np.cumsum([graphs[b][0] for b in idx])])
        eptr = np.concatenate([[0], np.cumsum([graphs[b][1].shape[1] for b in idx])])
        pptr = np.concatenate([[0], np.cumsum([len(pds[b]) for b in idx])])
        ei = torch.cat([graphs[b][1] + int(gptr[i]) for i, b in enumerate(idx)], dim=1)
        loops = torch.arange(int(gptr[-1]), dtype=torch.int64)
        ei = torch.cat([ei, torch.stack([loops, loops])], dim=1)              # self loops LAST
        model.zero_grad()
        out = model(torch.cat([fs[b] for b in idx]).cuda(), ei.cuda(), torch.cat([pds[b] for b in idx]).cuda(), kernel='wasserstein', p=2,
                    grad_PI=False, graph_ptr=torch.tensor(gptr).cuda(), edge_ptr=torch.tensor(eptr).cuda(), pd_ptr=torch.tensor(pptr).cuda(), **kw)
        out[2].backward()
        return float(out[2].detach()), {k: v.grad.detach().clone() for k, v in model.named_parameters() if v.grad is not None}

    with pytest.raises(ValueError, match="4096"):
        run([0, 1, 2])
    loss, grads = run([0, 1, 2], w2_large="device")
    total, acc = 0.0, {}
    for b in range(3):
        lb, gb = run([b], w2_large="device")
        total += lb
        for k, v in gb.items():
            acc[k] = acc[k] + v if k in acc else v
    assert np.isfinite(loss) and abs(loss - total) <= 1e-5 * max(1.0, abs(total)), (loss, total)
    assert set(grads) == set(acc) and grads
    for k in grads:
        assert _rel(grads[k], acc[k]) <= 1e-4, (k, _rel(grads[k], acc[k]))

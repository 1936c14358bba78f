"""GPU: the bottleneck distance (csrc/bottleneck.hip; ops.bottleneck_matching; autograd.bottleneck_loss; topo.bottleneck_to;
data_utils_GC.evaluate_packed / evaluate_batch with bottleneck=True) against the numpy + scipy restatement of include/tlcgnn.h in
tests/bottleneck_cases.py.  d_B is one entry of the cost matrix: every value is compared with ==, no tolerance anywhere but gradcheck's.

The matching is a witness, not a unique output: it is checked for being a perfect matching whose largest cost is d_dist; d_arg and the
gradients are then the restatement's rules applied to THAT matching.  The size classes: a wavefront per problem up to 512 rows, a
workgroup up to 4 096 (N = n + m)."""
import numpy as np
import pytest

import bottleneck_cases as cases
from bottleneck_checks import _check_witness, _pack, _raw_call, _raw_outputs, _solve

pytestmark = pytest.mark.gpu

CUT = 512                                                             # _lib.BN_WAVE_NMAX, asserted below
SIZES = (0, 1, 2, 63, 64, 65, CUT - 1, CUT, CUT + 1, 1023, 1024, 1025)
# the tied clouds stop behind the cut (513 rows already take the workgroup kernel): at 1 025 tied rows scipy's matcher alone needs 16 s
# for the one threshold that is tight
TIE_SIZES = SIZES[:9]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    from tlc_gnn_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    assert _lib.BN_WAVE_NMAX == CUT and _lib.BN_NMAX == 4096
    return torch


_CACHE = {}


def _solved(torch, style):
    """every size of SIZES as N = n + m with m in {0, N/3, N/2, N}: the batch solved once, the restatement computed once"""
    if style not in _CACHE:
        rs = np.random.RandomState(100 if style == "random" else 200)
        problems, index = [], {}
        for N in (SIZES if style == "random" else TIE_SIZES):
            for m in sorted({0, N // 3, N // 2, N}):
                index[(N, m)] = len(problems)
                problems.append(cases.pair(rs, N - m, m, style))
        xoff, yoff, h = _solve(torch, problems)
        want = [cases.bottleneck(X, Y) for X, Y in problems]
        _CACHE[style] = dict(problems=problems, index=index, xoff=xoff, yoff=yoff, h=h, want=want)
    return _CACHE[style]


@pytest.mark.parametrize("N", SIZES)
def test_values_and_witness(torch_cuda, N):
    s = _solved(torch_cuda, "random")
    for m in sorted({0, N // 3, N // 2, N}):
        b = s["index"][(N, m)]
        _check_witness(*s["problems"][b], s["h"], s["xoff"], s["yoff"], b, s["want"][b])


@pytest.mark.parametrize("N", TIE_SIZES)
def test_ties(torch_cuda, N):
    """coordinates k / 5: the value stays exact; the matching is one of many, valid and attaining the value"""
    s = _solved(torch_cuda, "grid")
    for m in sorted({0, N // 3, N // 2, N}):
        b = s["index"][(N, m)]
        X, Y = s["problems"][b]
        h, xoff, yoff = s["h"], s["xoff"], s["yoff"]
        assert h["status"][b] == 0 and h["dist"][b] == s["want"][b] and not np.signbit(h["dist"][b]), (N, m, h["dist"][b], s["want"][b])
        ax, ay = h["assign_x"][xoff[b]:xoff[b + 1]], h["assign_y"][yoff[b]:yoff[b + 1]]
        assert cases.check_matching(X, Y, ax, ay) == h["dist"][b]
        # the pair named is one of the matching's and attains the value
        i, j = h["arg"][b].tolist()
        if N == 0:
            assert (i, j) == (-1, -1)
        else:
            assert (i, j) in cases.pairs_of(ax, ay) and cases.pair_cost(X, Y, i, j) == h["dist"][b]
            assert (i, j) == cases.arg_of(X, Y, ax, ay)


def test_closed_forms_on_the_device(torch_cuda):
    rs = np.random.RandomState(3)
    X, _ = cases.pair(rs, 33, 0)
    E = np.zeros((0, 2))
    P = np.array([[0.25, 1.0]])
    _, _, h = _solve(torch_cuda, [(X, X), (P, E), (E, P), (E, E), (P[:, ::-1].copy(), E)])
    assert h["dist"].tolist() == [0.0, 0.375, 0.375, 0.0, 0.375] and not np.signbit(h["dist"]).any()
    assert h["arg"].tolist() == [[0, int(h["assign_x"][0])], [0, -1], [-1, 0], [-1, -1], [0, -1]]
    # a point below the diagonal moves the other way
    assert h["grad"][33].tolist() == [-0.5, 0.5] and h["grad"][34].tolist() == [0.5, -0.5] and h["grad_target"][33].tolist() == [-0.5, 0.5]


def test_cap(torch_cuda):
    """N = 4 096 = the cap with n = m = 2 048 and Y = X + 1e-3 noise (the start leaves little to augment); N = 4 097: status 2, and the
    wrappers raise naming the cap.  A random pair of 4 096 rows lives in tools/time_bottleneck.py."""
    from tlc_gnn_amd import autograd, ops
    torch = torch_cuda
    rs = np.random.RandomState(4)
    X, _ = cases.pair(rs, 2048, 0)
    Y = X + 1e-3 * rs.standard_normal(X.shape)
    xoff, yoff, h = _solve(torch, [(X, Y)])
    ident = np.maximum(np.abs(X[:, 0] - Y[:, 0]), np.abs(X[:, 1] - Y[:, 1])).max()
    _check_witness(X, Y, h, xoff, yoff, 0, cases.bottleneck(X, Y, upper=ident))
    X2, Y2 = cases.pair(rs, 2049, 2048)
    small = cases.pair(rs, 5, 4)
    xoff, yoff, h = _solve(torch, [small, (X2, Y2), small], check=False)
    assert h["status"].tolist() == [0, 2, 0] and h["dist"][1] == 0.0 and h["arg"][1].tolist() == [-1, -1]
    assert (h["assign_x"][5:5 + 2049] == -1).all() and (h["assign_y"][4:4 + 2048] == -1).all()
    assert not h["grad"][5:5 + 2049].any() and not h["grad_target"][4:4 + 2048].any()
    for b in (0, 2):
        _check_witness(*small, h, xoff, yoff, b, cases.bottleneck(*small))
    dX, dY = torch.as_tensor(X2).cuda(), torch.as_tensor(Y2).cuda()
    o = lambda k: torch.tensor([0, k], dtype=torch.int64).cuda()
    with pytest.raises(RuntimeError, match="4096"):
        ops.bottleneck_matching(o(2049), dX, o(2048), dY)
    with pytest.raises(RuntimeError, match="4096"):
        autograd.bottleneck_loss(dX.requires_grad_(True), dY)


def test_topo_refuses_above_the_cap(torch_cuda):
    import pd_grad_cases as pg
    from tlc_gnn_amd import topo
    torch = torch_cuda
    rs = np.random.RandomState(21)
    gs = [(1500, pg.chord_graph(rs, 1500, 4500))]
    no, eo, E, f = pg.pack(gs, [pg.distinct_values(rs, 1500)])
    dev = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a)).to(dt).cuda()
    t = dev(np.array([[0.0, 1.0]]), torch.float64)
    with pytest.raises(RuntimeError, match="4096"):
        topo.bottleneck_to(dev(f, torch.float64), dev(no, torch.int64), dev(eo, torch.int64), dev(E, torch.int32), t, dev(np.array([0, 1]), torch.int64))


def test_a_batch_larger_than_the_grid_equals_its_problems_alone(torch_cuda):
    torch = torch_cuda
    rs = np.random.RandomState(8)
    B = 20000
    problems = []
    for k in range(B):
        N = int(rs.randint(0, 41))
        m = int(rs.randint(0, N + 1))
        problems.append(cases.pair(rs, N - m, m, "grid" if k % 5 == 0 else "random"))
    xoff, yoff, (dxo, dX, dyo, dY) = _pack(torch, problems)
    nx, ny = int(xoff[-1]), int(yoff[-1])
    whole, alone = _raw_outputs(torch, B, nx, ny), _raw_outputs(torch, B, nx, ny)
    _raw_call(whole, dxo, dX, dyo, dY, 0, B, 40)
    for b in range(B):
        _raw_call(alone, dxo, dX, dyo, dY, b, 1, 40)
    torch.cuda.synchronize()
    for k in whole:
        assert torch.equal(whole[k], alone[k]), k
    assert int(whole["status"].max()) == 0 and float(whole["dist"].min()) >= 0.0
    # a sample against the restatement
    d = whole["dist"].cpu().numpy()
    for b in rs.randint(0, B, size=200).tolist() + [B - 1, 16383, 16384]:
        assert d[b] == cases.bottleneck(*problems[b]), b


def test_bad_problems_leave_their_neighbours_alone(torch_cuda):
    torch = torch_cuda
    rs = np.random.RandomState(9)
    good = [cases.pair(rs, 9, 7), cases.pair(rs, 300, 400), cases.pair(rs, 30, 3), cases.pair(rs, 2, 60)]
    nan = cases.pair(rs, 12, 10)
    nan[0][5, 1] = np.nan
    inf = cases.pair(rs, 400, 300)
    inf[1][17, 0] = np.inf
    big = cases.pair(rs, 2000, 2097)
    xoff, yoff, h = _solve(torch, [good[0], nan, good[1], big, good[2], inf, good[3]], check=False)
    assert h["status"].tolist() == [0, 3, 0, 2, 0, 3, 0]
    assert np.isnan(h["dist"][[1, 5]]).all() and h["dist"][3] == 0.0 and (h["arg"][[1, 3, 5]] == -1).all()
    for b in (1, 3, 5):
        assert (h["assign_x"][xoff[b]:xoff[b + 1]] == -1).all() and (h["assign_y"][yoff[b]:yoff[b + 1]] == -1).all()
        assert not h["grad"][xoff[b]:xoff[b + 1]].any() and not h["grad_target"][yoff[b]:yoff[b + 1]].any()
    for k, b in enumerate((0, 2, 4, 6)):
        xo1, yo1, h1 = _solve(torch, [good[k]])
        assert h1["dist"][0] == h["dist"][b] and np.array_equal(h1["arg"][0], h["arg"][b])
        for key, off in (("assign_x", xoff), ("assign_y", yoff), ("grad", xoff), ("grad_target", yoff)):
            assert np.array_equal(h1[key], h[key][off[b]:off[b + 1]]), (b, key)
        _check_witness(*good[k], h, xoff, yoff, b, cases.bottleneck(*good[k]))
    from tlc_gnn_amd import ops
    _, _, (dxo, dX, dyo, dY) = _pack(torch, [good[0], nan])
    with pytest.raises(RuntimeError, match="NaN"):
        ops.bottleneck_matching(dxo, dX, dyo, dY)


def test_gradcheck_in_both_diagrams(torch_cuda):
    from tlc_gnn_amd import autograd
    torch = torch_cuda
    rs = np.random.RandomState(10)
    problems = [cases.pair(rs, 4, 3), cases.pair(rs, 2, 5), cases.pair(rs, 3, 0), cases.pair(rs, 0, 2)]
    xoff, yoff, (dxo, dX, dyo, dY) = _pack(torch, problems)
    dX.requires_grad_(True)
    dY.requires_grad_(True)
    fn = lambda a, b: autograd.bottleneck_loss(a, b, xoff=dxo, yoff=dyo)
    assert torch.autograd.gradcheck(fn, (dX, dY))                     # the fp64 defaults: eps 1e-6, atol 1e-5, rtol 1e-3
    # only pd_hat requires grad: the target gets none
    Y0 = dY.detach()
    loss = autograd.bottleneck_loss(dX, Y0, xoff=dxo, yoff=dyo)
    assert loss.shape == (4,) and loss.dtype == torch.float64
    loss.sum().backward()
    assert int((dX.grad.abs().sum(1) > 0).sum()) <= 4 and Y0.grad is None


@pytest.fixture(scope="module")
def graphs(torch_cuda):
    """64 small graphs with their values, and the diagrams of hidden values of the same graphs as targets"""
    import pd_grad_cases as pg
    from tlc_gnn_amd import topo
    torch = torch_cuda
    rs = np.random.RandomState(22)
    gs = [(n, pg.small_graph(rs, n)) for n in rs.randint(3, 17, size=64).tolist()]
    no, eo, E, f = pg.pack(gs, [pg.distinct_values(rs, n) for n, _ in gs])
    _, _, _, hidden = pg.pack(gs, [pg.distinct_values(rs, n) for n, _ in gs])
    dev = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a)).to(dt).cuda()
    g = dict(no=dev(no, torch.int64), eo=dev(eo, torch.int64), E=dev(E, torch.int32), f=dev(f, torch.float64), B=len(gs))
    with torch.no_grad():
        g["target"], g["toffs"] = topo._select(dev(hidden, torch.float64), g["no"], g["eo"], g["E"], "ord0+ext1", "host")
    return g


def test_topo_bottleneck_to(torch_cuda, graphs):
    from tlc_gnn_amd import topo
    torch, g = torch_cuda, graphs
    f = g["f"].clone().requires_grad_(True)
    loss = topo.bottleneck_to(f, g["no"], g["eo"], g["E"], g["target"], g["toffs"])
    assert loss.shape == (g["B"],) and loss.dtype == torch.float64
    d = topo.diagrams(g["f"], g["no"], g["eo"], g["E"])
    P0, o0, P1, o1 = (d[k].cpu().numpy() for k in ("ord0", "ord0_offs", "ext1", "ext1_offs"))
    T, to = g["target"].cpu().numpy(), g["toffs"].cpu().numpy()
    got = loss.detach().cpu().numpy()
    for b in range(g["B"]):
        X = np.concatenate([P0[o0[b]:o0[b + 1]], P1[o1[b]:o1[b + 1]]])
        assert got[b] == cases.bottleneck(X, T[to[b]:to[b + 1]]), b
    loss.sum().backward()
    # per graph at most one point of the predicted diagram moves: two node values
    assert bool(torch.isfinite(f.grad).all()) and 0 < int((f.grad != 0).sum()) <= 2 * g["B"]
    with pytest.raises(ValueError, match="which"):
        topo.bottleneck_to(f, g["no"], g["eo"], g["E"], g["target"], g["toffs"], which="rel1")


# measured on an MI355X: end / start = 0.705.  Three times that is above 1 and would assert nothing, so the margin of
# three is taken on the decrease: 1 - (1 - 0.705) / 3
TRAIN_RATIO_BOUND = 0.902


def test_training_smoke(torch_cuda, graphs):
    """100 Adam steps on the node values toward the diagrams of the hidden values: the summed bottleneck distance falls, by at
    least a third of the measured decrease (TRAIN_RATIO_BOUND)."""
    from tlc_gnn_amd import topo
    torch, g = torch_cuda, graphs
    f = g["f"].clone().requires_grad_(True)
    opt = torch.optim.Adam([f], lr=0.01)
    losses = []
    for _ in range(100):
        opt.zero_grad()
        loss = topo.bottleneck_to(f, g["no"], g["eo"], g["E"], g["target"], g["toffs"]).sum()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print("bottleneck training: start %.6g end %.6g ratio %.4f" % (losses[0], losses[-1], losses[-1] / losses[0]))
    assert losses[-1] < losses[0] and losses[-1] / losses[0] <= TRAIN_RATIO_BOUND


def test_evaluate_packed_with_bottleneck(torch_cuda):
    import gc_cases as gc
    from tlc_gnn_amd.Knowledge_Distillation import data_utils_GC as kd
    from tlc_gnn_amd.Knowledge_Distillation.Teacher_model import Teacher_Model
    torch = torch_cuda
    graphs = gc.route_graphs()
    assert len(graphs) == 300
    torch.manual_seed(5)
    model = Teacher_Model(type='GAT').cuda().eval()
    gt = kd.ground_truth_packed(*kd.pack_dataset(graphs), filt="degree")
    plain = kd.evaluate_packed(model, gt)
    rec = kd.evaluate_packed(model, gt, bottleneck=True)
    assert len(plain) == 2 and len(rec) == 3 and rec[1] == plain[1] and torch.equal(rec[0], plain[0]) and len(rec[1]) > 200
    ref_img, ref_kept = kd.evaluate_batch(model, gt.tuples())
    assert plain[1] == ref_kept and torch.equal(plain[0], ref_img)
    rec_b = kd.evaluate_batch(model, gt.tuples(), bottleneck=True)
    assert len(rec_b) == 3 and torch.equal(rec_b[2], rec[2]) and rec[2].dtype == torch.float64 and rec[2].shape == (len(rec[1]),)
    # the predicted diagrams: the model's point per edge, as evaluate_packed feeds it
    K = gt.f.numel()
    base = torch.repeat_interleave(gt.node_ptr[:-1], gt.edge_ptr[1:] - gt.edge_ptr[:-1], output_size=gt.edges.shape[0])
    loops = torch.arange(K, dtype=torch.int64, device="cuda")
    edge_index = torch.cat([(gt.edges.to(torch.int64) + base[:, None]).t(), torch.stack([loops, loops])], dim=1)
    with torch.no_grad():
        pd_hat = model(gt.f.float().view(-1, 1), edge_index, None, compute_loss=False, grad_PI=False, graph_ptr=gt.node_ptr, edge_ptr=gt.edge_ptr)[0]
    P, ep = pd_hat.double().cpu().numpy(), gt.edge_ptr.cpu().numpy()
    d0, o0, d1, o1 = (getattr(gt, k).cpu().numpy() for k in ("d0", "o0", "d1", "o1"))
    got = rec[2].cpu().numpy()
    for i in range(len(rec[1])):
        exact = np.concatenate([d0[o0[i]:o0[i + 1]], d1[o1[i]:o1[i + 1]]])
        assert got[i] == cases.bottleneck(P[ep[i]:ep[i + 1]], exact), i

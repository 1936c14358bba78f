"""GPU: the sliced Wasserstein diagram loss and its gradient (csrc/sliced_w.hip; ops.sliced_wasserstein; autograd.sliced_diagram_loss;
topo.sliced_wasserstein_to; Teacher_Model(kernel='sliced_wasserstein')).

The reference is the numpy restatement of include/tlcgnn.h's definition in tests/sliced_w_cases.py: gradients are compared with ==, the
loss within the suite's standing fp64 bound (1e-11 relative, as in the HKS tests: the rank sums differ in order only)."""
import ctypes as C

import numpy as np
import pytest

import sliced_w_cases as cases
from tlc_gnn_amd import _lib

pytestmark = pytest.mark.gpu
LDS_NMAX = _lib.SW_LDS_NMAX
LOSS_RTOL = 1e-11
# one problem of every class: (n, m)
PER_CLASS = {"wave": (23, 17), "lds": (170, 131), "wide": (LDS_NMAX // 2 + 40, LDS_NMAX // 2 + 90)}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _dev(torch, a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def run(torch, problems, dirs, scale, want_grad=("x", "y"), work_bytes=None):
    """-> (loss [B], gradX [sum n, 2], gradY [sum m, 2], status [B]) as numpy"""
    from tlc_gnn_amd import ops
    xoff, X, yoff, Y = cases.pack(problems)
    r = ops.sliced_wasserstein(_dev(torch, xoff, torch.int64), _dev(torch, X, torch.float64).reshape(-1, 2), _dev(torch, yoff, torch.int64),
                               _dev(torch, Y, torch.float64).reshape(-1, 2), dirs=torch.as_tensor(np.asarray(dirs), dtype=torch.float64),
                               scale=scale, want_grad=want_grad, work_bytes=work_bytes)
    return tuple(None if r[k] is None else r[k].cpu().numpy() for k in ("loss", "grad_x", "grad_y", "status"))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def close(got, want):
    return abs(got - want) <= LOSS_RTOL * max(abs(want), 1e-300)


@pytest.fixture(scope="module")
def dirs5():
    from tlc_gnn_amd import ops
    return ops.sliced_directions(5)                     # theta = 0.5, 0.7, ... 1.3: l0 + l1 != 0 in every direction


# ---- 1. gradient bits at every edge of the classes -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edge_problems(dirs5):
    rs = np.random.RandomState(11)
    problems = [cases.tie_free(rs, n, m, dirs5[0]) for n, m in cases.class_sizes()]
    return problems, [cases.restate(X, Y, *dirs5) for X, Y in problems]


def test_gradient_bits_at_the_class_edges(torch_cuda, dirs5, edge_problems):
    problems, want = edge_problems
    sizes = sorted(len(X) + len(Y) for X, Y in problems)
    assert sizes[:2] == [1, 2] and {63, 64, 65, LDS_NMAX - 1, LDS_NMAX, LDS_NMAX + 1} <= set(sizes) and sizes[-1] > 2.9 * LDS_NMAX
    assert all(len(X) != len(Y) for X, Y in problems) and any(len(X) == 0 for X, _ in problems) and any(len(Y) == 0 for _, Y in problems)
    loss, gx, gy, status = run(torch_cuda, problems, *dirs5)
    assert not status.any()
    xoff, _, yoff, _ = cases.pack(problems)
    for k, (wl, wx, wy) in enumerate(want):
        label = "n=%d m=%d" % (len(problems[k][0]), len(problems[k][1]))
        print(label, "loss", loss[k], "restatement", wl, "rel", abs(loss[k] - wl) / max(abs(wl), 1e-300))
        assert np.array_equal(gx[xoff[k]:xoff[k + 1]], wx), label
        assert np.array_equal(gy[yoff[k]:yoff[k + 1]], wy), label
        assert close(loss[k], wl), (label, loss[k], wl)


def test_one_gradient_alone(torch_cuda, dirs5, edge_problems):
    """grad_x without grad_y and the other way round: the same bits, and the side that was not asked for is None"""
    problems, _ = edge_problems
    both = run(torch_cuda, problems, *dirs5)
    lx, gx, none_y, _ = run(torch_cuda, problems, *dirs5, want_grad=("x",))
    ly, none_x, gy, _ = run(torch_cuda, problems, *dirs5, want_grad=("y",))
    assert none_y is None and none_x is None
    assert same_bits(gx, both[1]) and same_bits(gy, both[2]) and same_bits(lx, both[0]) and same_bits(ly, both[0])


# ---- 2. exact values --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", sorted(PER_CLASS))
def test_exact_values(torch_cuda, cls):
    n, m = PER_CLASS[cls]
    X, Y = cases.even_grid(np.random.RandomState(5), n, m)
    want = cases.exact_loss(X, Y)
    loss, gx, gy, status = run(torch_cuda, [(X, Y)], cases.EXACT_DIRS, cases.EXACT_SCALE)
    assert status[0] == 0 and want > 0
    assert loss[0] == want, (loss[0], want)
    _, wx, wy = cases.restate(X, Y, cases.EXACT_DIRS, cases.EXACT_SCALE)
    assert np.array_equal(gx, wx) and np.array_equal(gy, wy)


# ---- 3. ties ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", sorted(PER_CLASS))
def test_ties_follow_the_stable_order(torch_cuda, cls):
    n, m = PER_CLASS[cls]
    X, Y = cases.tied(np.random.RandomState(6), n, m)
    assert np.signbit(X[1, 0]) and X[0].sum() == 0
    from tlc_gnn_amd import ops
    dirs, scale = ops.sliced_directions(4)              # theta = 0.75 among them: l0 + l1 == 0, every diagonal key equal
    assert dirs[1].sum() == 0
    dirs = np.concatenate([dirs, cases.EXACT_DIRS])
    loss, gx, gy, status = run(torch_cuda, [(X, Y)], dirs, scale)
    wl, wx, wy = cases.restate(X, Y, dirs, scale)
    assert status[0] == 0
    assert np.array_equal(gx, wx) and np.array_equal(gy, wy)
    assert close(loss[0], wl), (loss[0], wl)
    assert wx.any() and wy.any()


# ---- 4. identities ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", sorted(PER_CLASS))
def test_identities(torch_cuda, dirs5, cls):
    n, m = PER_CLASS[cls]
    rs = np.random.RandomState(7)
    X, Y = cases.tie_free(rs, n, m, dirs5[0])
    # SW(X, X): the two lists are equal element by element
    Z = np.concatenate([X, Y])[: max((n + m) // 2, 1)]
    loss, gx, gy, status = run(torch_cuda, [(Z, Z)], *dirs5)
    assert status[0] == 0 and bits(loss)[0] == 0 and not gx.any() and not gy.any()
    # symmetry
    lxy, gx_xy, gy_xy, _ = run(torch_cuda, [(X, Y)], *dirs5)
    lyx, gx_yx, gy_yx, _ = run(torch_cuda, [(Y, X)], *dirs5)
    assert same_bits(lxy, lyx)
    assert np.array_equal(gx_xy, gy_yx) and np.array_equal(gy_xy, gx_yx)
    assert lxy[0] > 0 and gx_xy.any()


# ---- 5. batches -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed(dirs5):
    """more problems than the wave class's grid has wavefronts (4 x 2 048) and than the workgroup class's grid has workgroups, in an
    order that mixes the classes"""
    rs = np.random.RandomState(3)
    sizes = [(int(a), int(b)) for a, b in rs.randint(0, 7, size=(8400, 2))]
    for at, nm in ((17, (70, 30)), (3000, (200, 190)), (8300, (33, 100)), (100, (LDS_NMAX // 2 + 5, LDS_NMAX // 2)), (8390, (LDS_NMAX, 300)),
                   (5000, (40, 24)), (5001, (0, 0)), (8399, (64, 1))):
        sizes[at] = nm
    dirs = dirs5[0][:3]
    problems = []
    for n, m in sizes:
        problems.append(cases.tie_free(rs, n, m, dirs))
    return problems, dirs, dirs5[1]


def test_a_batch_equals_its_problems_alone(torch_cuda, mixed):
    from tlc_gnn_amd import ops
    torch = torch_cuda
    problems, dirs, scale = mixed
    sizes = np.array([len(X) + len(Y) for X, Y in problems])
    assert len(problems) > 4 * 2048 and (sizes <= 64).sum() > 4 * 2048 and ((sizes > 64) & (sizes <= LDS_NMAX)).any() and (sizes > LDS_NMAX).sum() == 2
    loss, gx, gy, status = run(torch, problems, dirs, scale)
    again = run(torch, problems, dirs, scale)
    assert not status.any()
    assert all(same_bits(a, b) for a, b in zip((loss, gx, gy), again[:3])), "two runs differ"
    # every problem alone: one library call each, on its own slice of the packed arrays (raw pointers: 8 400 wrapper calls would spend
    # their time in Python), with a workspace as large as the largest problem wants
    xoff, X, yoff, Y = cases.pack(problems)
    B = len(problems)
    d_dirs = torch.as_tensor(dirs, dtype=torch.float64).cuda()
    dX, dY = _dev(torch, X, torch.float64), _dev(torch, Y, torch.float64)
    pair = lambda o: _dev(torch, np.stack([np.zeros(B, dtype=np.int64), np.diff(o)], 1), torch.int64)
    xo, yo = pair(xoff), pair(yoff)
    al, ax, ay = torch.full((B,), 7.0, dtype=torch.float64, device="cuda"), torch.full_like(dX, 7.0), torch.full_like(dY, 7.0)
    st = torch.full((B,), 9, dtype=torch.uint8, device="cuda")
    nbytes = ops.sliced_w_work_bytes(1, int(sizes.max()), int(sizes.max()), len(dirs))
    work = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    L, stream = _lib.lib(), _lib.stream_ptr()
    at = lambda t, rows, width: C.c_void_p(t.data_ptr() + int(rows) * width)
    for k in range(B):
        rc = L.tlc_sliced_wasserstein(C.c_int32(1), at(xo, k, 16), at(dX, xoff[k], 16), at(yo, k, 16), at(dY, yoff[k], 16), C.c_int32(len(dirs)),
                                      _lib.ptr(d_dirs), C.c_double(scale), C.c_int64(int(sizes[k])), at(al, k, 8), at(ax, xoff[k], 16),
                                      at(ay, yoff[k], 16), at(st, k, 1), _lib.ptr(work), C.c_int64(nbytes), stream)
        assert rc == 0, (k, L.tlc_last_error())
    assert not st.cpu().numpy().any()
    al, ax, ay = al.cpu().numpy(), ax.cpu().numpy(), ay.cpu().numpy()
    assert same_bits(loss, al) and same_bits(gx, ax) and same_bits(gy, ay)
    # and the restatement on the named problems
    for k in (17, 100, 5000, 5001, 8390, 8399):
        wl, wx, wy = cases.restate(*problems[k], dirs, scale)
        assert np.array_equal(gx[xoff[k]:xoff[k + 1]], wx) and np.array_equal(gy[yoff[k]:yoff[k + 1]], wy) and close(loss[k], wl), k


def test_any_workspace_gives_the_same_bits(torch_cuda):
    from tlc_gnn_amd import ops
    rs = np.random.RandomState(9)
    # M = 8 directions without theta = 0.75 (where l0 + l1 == 0 makes every diagonal key equal): the first eight of nine
    dirs, scale = ops.sliced_directions(9)[0][:8], 1.0 / 8
    n, m = LDS_NMAX + 300, LDS_NMAX - 100
    prob = [cases.tie_free(rs, n, m, dirs)]
    least, full = ops.sliced_w_work_bytes(1, n + m, n + m, 1), ops.sliced_w_work_bytes(1, n + m, n + m, 8)
    assert 0 < least < full
    want = run(torch_cuda, prob, dirs, scale, work_bytes=full)
    assert same_bits(want[0], run(torch_cuda, prob, dirs, scale)[0])
    for wb in (least, least + (full - least) // 3, full - 1, 2 * full):
        got = run(torch_cuda, prob, dirs, scale, work_bytes=wb)
        assert all(same_bits(a, c) for a, c in zip(got[:3], want[:3])), wb
    wl, wx, wy = cases.restate(*prob[0], dirs, scale)
    assert np.array_equal(want[1], wx) and np.array_equal(want[2], wy) and close(want[0][0], wl)
    with pytest.raises(_lib.TlcError):
        run(torch_cuda, prob, dirs, scale, work_bytes=least - 1)


# ---- 6. autograd ------------------------------------------------------------------------------------------------------------------------
def test_gradcheck_in_both_arguments(torch_cuda, dirs5):
    from tlc_gnn_amd import autograd
    torch = torch_cuda
    rs = np.random.RandomState(12)
    dirs = torch.as_tensor(dirs5[0][:3]).cuda()
    problems = [cases.tie_free(rs, 4, 3, dirs5[0][:3]), cases.tie_free(rs, 2, 5, dirs5[0][:3])]
    xoff, X, yoff, Y = cases.pack(problems)
    dX = _dev(torch, X, torch.float64).requires_grad_(True)
    dY = _dev(torch, Y, torch.float64).requires_grad_(True)
    xo, yo = _dev(torch, xoff, torch.int64), _dev(torch, yoff, torch.int64)
    fn = lambda a, b: autograd.sliced_diagram_loss(a, b, xoff=xo, yoff=yo, dirs=dirs, scale=dirs5[1])
    # piecewise linear: with every gap far above eps the difference quotient is the gradient up to rounding
    assert torch.autograd.gradcheck(fn, (dX, dY), eps=1e-7, atol=1e-6, rtol=1e-6, nondet_tol=0.0)
    loss = fn(dX, dY.detach())
    assert loss.shape == (2,) and loss.requires_grad
    f32 = autograd.sliced_diagram_loss(dX.detach().float().requires_grad_(True), dY.detach().float(), xoff=xo, yoff=yo, M=5)
    assert f32.dtype == torch.float32                    # the input's dtype, like DiagramLoss


@pytest.fixture(scope="module")
def graphs(torch_cuda):
    """a packed batch of small graphs and one graph whose Ord0 + Ext1 diagram has more than 4 096 points"""
    import pd_grad_cases as pg
    torch = torch_cuda
    rs = np.random.RandomState(21)
    small = [(n, pg.small_graph(rs, n)) for n in (5, 9, 16, 12)] + [(70, pg.chord_graph(rs, 70, 120))]
    big = [(1500, pg.chord_graph(rs, 1500, 4500))]
    out = {}
    for label, gs in (("small", small), ("big", big)):
        no, eo, E, f = pg.pack(gs, [pg.distinct_values(rs, n) for n, _ in gs])
        k = [max(len(e) - 2, 1) for _, e in gs]
        t = rs.random_sample((sum(k), 2))
        t[:, 1] += t[:, 0]
        out[label] = dict(no=_dev(torch, no, torch.int64), eo=_dev(torch, eo, torch.int64), E=_dev(torch, E, torch.int32), f=_dev(torch, f, torch.float64),
                          target=_dev(torch, t, torch.float64), toffs=_dev(torch, np.concatenate([[0], np.cumsum(k)]), torch.int64), B=len(gs))
    return out


@pytest.mark.parametrize("label", ["small", "big"])
def test_topo_sliced_wasserstein_to(torch_cuda, graphs, label):
    from tlc_gnn_amd import ops, topo
    torch, g = torch_cuda, graphs[label]
    M = 6
    f = g["f"].clone().requires_grad_(True)
    loss = topo.sliced_wasserstein_to(f, g["no"], g["eo"], g["E"], g["target"], g["toffs"], M=M)
    assert loss.shape == (g["B"],) and bool(torch.isfinite(loss).all()) and float(loss.min()) > 0
    loss.sum().backward()
    assert bool(torch.isfinite(f.grad).all()) and float(f.grad.abs().max()) > 0
    # the same gradient from its two halves: the restatement's point gradients pushed through pd_grad's selection
    f2 = g["f"].clone().requires_grad_(True)
    pts, offs = topo._select(f2, g["no"], g["eo"], g["E"], "ord0+ext1", "host")
    if label == "big":
        assert int(offs[-1]) > 4096
        with pytest.raises(ValueError):
            topo.wasserstein_to(g["f"], g["no"], g["eo"], g["E"], g["target"], g["toffs"])
    P, T, po, to = pts.detach().cpu().numpy(), g["target"].cpu().numpy(), offs.cpu().numpy(), g["toffs"].cpu().numpy()
    dirs, scale = ops.sliced_directions(M)
    gp = np.zeros_like(P)
    for b in range(g["B"]):
        wl, wx, _ = cases.restate(P[po[b]:po[b + 1]], T[to[b]:to[b + 1]], dirs, scale)
        gp[po[b]:po[b + 1]] = wx
        assert close(float(loss[b]), wl), (b, float(loss[b]), wl)
    pts.backward(_dev(torch, gp, torch.float64))
    assert torch.equal(f.grad, f2.grad)


def test_training_smoke(torch_cuda, graphs):
    """ten steps of gradient descent on the filtration values themselves: the sliced distance to the target diagrams goes down"""
    from tlc_gnn_amd import topo
    torch, g = torch_cuda, graphs["small"]
    f = g["f"].clone().requires_grad_(True)
    opt = torch.optim.SGD([f], lr=0.01)
    losses = []
    for _ in range(10):
        opt.zero_grad()
        loss = topo.sliced_wasserstein_to(f, g["no"], g["eo"], g["E"], g["target"], g["toffs"], M=8).sum()
        loss.backward()
        opt.step()
        losses.append(float(loss))
    print("losses", losses)
    assert losses[-1] < losses[0]


# ---- 7. the teacher, and what is refused ------------------------------------------------------------------------------------------------
def test_teacher_sliced_wasserstein(torch_cuda):
    from tlc_gnn_amd import ops
    from tlc_gnn_amd.Knowledge_Distillation.Teacher_model import Teacher_Model
    torch = torch_cuda
    torch.manual_seed(0)
    n = 12
    src = torch.arange(n)
    ei = torch.cat([torch.stack([src, (src + 1) % n]), torch.stack([src, (src + 5) % n]), torch.stack([src, src])], 1).cuda()
    m = ei.shape[1] - n
    f = torch.rand(n, 1).cuda()
    PD = torch.rand(m, 2).cuda()
    PD[:, 1] += PD[:, 0]
    model = Teacher_Model(type='GAT', dropout=0.0).cuda().train()
    out = model(f, ei, PD, kernel='sliced_wasserstein', M=50, grad_PI=False)
    pts, loss0 = out[0], out[2]
    assert loss0.shape == (1,) and loss0.requires_grad
    for part in out[3:6]:
        assert part.shape == (1,) and float(part) == 0.0 and not part.requires_grad
    off = lambda k: torch.tensor([0, k], dtype=torch.int64, device="cuda")
    want = ops.sliced_wasserstein(off(m), pts.detach().double(), off(m), PD.double(), M=50)
    assert int(want["status"][0]) == 0
    assert float(loss0) == float(want["loss"][0].to(loss0.dtype))
    # p and pair_diagonal have no effect
    other = model(f, ei, PD, kernel='sliced_wasserstein', M=50, p=2, pair_diagonal=True, grad_PI=False)[2]
    assert float(other) == float(loss0)
    loss0.backward()
    d = model.DIM0_Model
    on_path = [p for conv in (d.conv1, d.conv2, d.conv4, d.conv3) for p in (conv.lin_l.weight, conv.att_l, conv.lin_ij.weight, conv.bias)]
    on_path += [model.lin5.weight, model.lin5.bias, model.lin6.weight, model.lin6.bias]
    for k, p in enumerate(on_path):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
    assert any(float(p.grad.abs().max()) > 0 for p in on_path)
    assert model.lin1.weight.grad is None                # not on the path
    with pytest.raises(NotImplementedError, match="sliced_wasserstein"):
        model(f, ei, PD, kernel='sliced', grad_PI=False)


@pytest.mark.parametrize("cls", sorted(PER_CLASS))
def test_non_finite_coordinates(torch_cuda, dirs5, cls):
    from tlc_gnn_amd import autograd
    torch = torch_cuda
    n, m = PER_CLASS[cls]
    rs = np.random.RandomState(13)
    good = cases.tie_free(rs, 9, 4, dirs5[0])
    for value, side, row in ((np.nan, 0, n - 1), (np.inf, 1, 0), (-np.inf, 1, m - 1)):
        X, Y = cases.tie_free(rs, n, m, dirs5[0])
        (X, Y)[side][row, side] = value
        loss, gx, gy, status = run(torch, [good, (X, Y), good], *dirs5)
        assert status.tolist() == [0, 3, 0] and np.isnan(loss[1]) and np.isfinite(loss[[0, 2]]).all()
        assert not gx[9:9 + n].any() and not gy[4:4 + m].any()
        assert same_bits(gx[:9], gx[9 + n:]) and gx[:9].any()                 # the neighbours are computed, and equal
        with pytest.raises(ValueError, match="status"):
            autograd.sliced_diagram_loss(_dev(torch, X, torch.float64), _dev(torch, Y, torch.float64), M=5)


def test_refusals(torch_cuda, dirs5):
    from tlc_gnn_amd import ops
    torch = torch_cuda
    X, Y = cases.tie_free(np.random.RandomState(14), 6, 5, dirs5[0])
    for M in (0, _lib.SW_MAX_DIRS + 1):
        with pytest.raises(_lib.TlcError, match="n_dirs"):
            run(torch, [(X, Y)], np.zeros((M, 2)), 0.5)
    assert run(torch, [(X, Y)], np.ones((_lib.SW_MAX_DIRS, 2)), 0.5)[3][0] == 0
    big = cases.tie_free(np.random.RandomState(15), LDS_NMAX, 7, dirs5[0][:1])
    least = ops.sliced_w_work_bytes(1, LDS_NMAX + 7, LDS_NMAX + 7, 1)
    with pytest.raises(_lib.TlcError, match=str(least)):
        run(torch, [big], dirs5[0][:1], 1.0, work_bytes=least - 256)
    # offsets that decrease
    dX, dY = _dev(torch, X, torch.float64), _dev(torch, Y, torch.float64)
    with pytest.raises(_lib.TlcError, match="decrease"):
        ops.sliced_wasserstein(torch.tensor([0, 4, 2, 6]).cuda(), dX, torch.tensor([0, 1, 3, 5]).cuda(), dY, M=3)
    with pytest.raises(ValueError):
        ops.sliced_wasserstein(torch.tensor([0, 7]).cuda(), dX, torch.tensor([0, 5]).cuda(), dY, M=3)

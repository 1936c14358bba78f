"""GPU: the teacher's GIN / GCN / SAGE baselines (csrc/gnn_layers.hip; ops.gnn_layer / gnn_layer_bwd / gnn_stack; autograd.GnnLayer;
Knowledge_Distillation/gnn_layers.py and Teacher_model.py) against the float64 torch restatement of tests/gnn_baseline_cases.py with
autograd.  Tolerances are the project's for this precision class (tests/test_gpu_train.py:128-171): max-abs difference over max-abs
reference <= 2e-5 for a forward, <= 1e-4 for every gradient; determinism is compared with torch.equal."""
import ctypes as C

import numpy as np
import pytest

import gnn_baseline_cases as gb

pytestmark = pytest.mark.gpu

FWD_TOL, GRAD_TOL = 2e-5, 1e-4
KINDS = gb.KINDS
ACTS = ((None, 0.0), ("relu", 0.0), ("prelu", 0.1))
ROWS = 64                                              # GN_ROWS of csrc/gnn_layers.hip (_lib.GNN_ROWS): node rows per group


def _dev_layer(kind, ei, n, x, p, act, slope, G=None, need_gx=True):
    """The device layer on edge list `ei` (CPU int64): (out, agg, grads or None); grads = (gX, gWa, gWs, gb)."""
    import torch
    from tlc_gnn_amd import ops
    from tlc_gnn_amd.Knowledge_Distillation.gnn_layers import GnnBatch
    b = GnnBatch(ei.cuda(), n, kind)
    wa, ws, bias = (None if t is None else t.cuda() for t in gb.device_operands(kind, p))
    xd = x.to(torch.float32).cuda()
    out, agg = ops.gnn_layer(b.rowptr, b.src, b.coef, b.self_scale, xd, wa, ws, bias, act, slope, want_agg=True)
    if G is None:
        return out, agg, None
    rt, ct, cft = b.transpose() if need_gx else (None, None, None)
    grads = ops.gnn_layer_bwd(rt, ct, cft, b.self_scale, xd, agg, out, G.to(torch.float32).cuda(), wa, ws, True, act, slope, need_gx=need_gx)
    return out, agg, grads


def _ref_layer(kind, ei, x, p, act, slope, G):
    """float64 restatement with autograd: (out, {x, wa, ws, b} gradients in the device's layouts)."""
    import torch
    xr = x.double().clone().requires_grad_()
    pr = {k: v.double().clone().requires_grad_() for k, v in p.items()}
    out = gb.layer(kind, xr, ei, pr, act, slope)
    (out * G.double()).sum().backward()
    if kind == "GIN":
        g = {"wa": pr["w"].grad, "ws": None, "b": pr["b"].grad}
    elif kind == "GCN":
        g = {"wa": pr["weight"].grad.t(), "ws": None, "b": pr["bias"].grad}
    else:
        g = {"wa": pr["wl"].grad, "ws": pr["wr"].grad, "b": pr["bl"].grad}
    g["x"] = xr.grad
    return out.detach(), g


def _check_layer(kind, ei, n, c_in, c_out, seed, acts=ACTS):
    import torch
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(n, c_in, generator=gen, dtype=torch.float64).float()
    p = {k: v.float() for k, v in gb.random_layer_params(kind, c_in, c_out, gen).items()}
    G = torch.randn(n, c_out, generator=gen, dtype=torch.float64).float()
    m = ei.shape[1]
    for act, slope in acts:
        want, gw = _ref_layer(kind, ei, x, p, act, slope, G)
        out, agg, (gx, gwa, gws, gb_) = _dev_layer(kind, ei, n, x, p, act, slope, G)
        assert out.shape == (n, c_out) and agg.shape == (n, c_in)
        assert gb.rel(out, want) <= FWD_TOL, (kind, act, gb.rel(out, want))
        for name, got, ref in (("x", gx, gw["x"]), ("wa", gwa, gw["wa"]), ("ws", gws, gw["ws"]), ("b", gb_, gw["b"])):
            if ref is None:
                assert got is None, name
                continue
            assert got.shape == ref.shape, name
            if float(ref.abs().max()) == 0.0:
                assert float(got.abs().max()) == 0.0, (kind, act, name)
            else:
                assert gb.rel(got, ref) <= GRAD_TOL, (kind, act, name, gb.rel(got, ref))
        if m == 0 and kind == "SAGE":
            assert float(gwa.abs().max()) == 0.0 and float(agg.abs().max()) == 0.0       # no in-edges: lin_l sees zeros, exactly
        if m == 0 and kind == "GIN":
            assert torch.equal(agg.cpu(), x)                                              # (1 + eps) x_i alone
        # the first layer's form: no input gradient, the same weight gradients
        _, _, (gx0, gwa0, gws0, gb0) = _dev_layer(kind, ei, n, x, p, act, slope, G, need_gx=False)
        assert gx0 is None and torch.equal(gwa0, gwa) and torch.equal(gb0, gb_) and (gws is None or torch.equal(gws0, gws))


@pytest.mark.parametrize("n,m", [(300, 2400), (7, 12), (1, 0)])
@pytest.mark.parametrize("c_in,c_out", [(1, 32), (32, 32), (64, 8), (5, 16)])
@pytest.mark.parametrize("kind", KINDS)
def test_layer_forward_and_backward_match_autograd_of_the_restatement(kind, c_in, c_out, n, m):
    rs = np.random.RandomState(c_in * 100 + c_out + n)
    _check_layer(kind, gb.random_edges(rs, n, m, loops="some"), n, c_in, c_out, seed=n + c_in + c_out)


@pytest.mark.parametrize("kind", KINDS)
def test_layer_at_the_mfma_block_and_row_group_edges(kind):
    """n = 15 / 16 / 17 (one 16-row MFMA block) and 63 / 64 / 65 (one group of ROWS rows: one below, at, one above)."""
    from tlc_gnn_amd import _lib
    assert _lib.GNN_ROWS == ROWS
    for n in (15, 16, 17, ROWS - 1, ROWS, ROWS + 1):
        rs = np.random.RandomState(n)
        _check_layer(kind, gb.random_edges(rs, n, 5 * n, loops="some"), n, 32, 32, seed=n, acts=(("prelu", 0.1),))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("style", ["repeats", "double_loop", "no_loops", "one_orientation", "missing_loops"])
def test_layer_on_special_edge_lists(kind, style):
    """GIN / SAGE keep the list as given: repeated edges, two self loops on one node, no self loop at all, one orientation per edge (the
    teacher's own convention).  GCN replaces the list's loops: repeated ones count once, missing ones are added."""
    import torch
    rs = np.random.RandomState(len(style))
    n = 40
    if style == "repeats":
        e = gb.random_edges(rs, n, 120, loops="none")
        e = torch.cat([e, e[:, :30], e[:, :10]], dim=1)
    elif style == "double_loop":
        e = gb.random_edges(rs, n, 120, loops="double")
    elif style == "no_loops":
        e = gb.random_edges(rs, n, 120, loops="none")
    elif style == "one_orientation":
        e = gb.connected_graph(rs, n, 60)
    else:
        e = gb.random_edges(rs, n, 120, loops="none")
        lp = torch.arange(0, n, 3)
        e = torch.cat([e, torch.stack([lp, lp])], dim=1)                # a loop on every third node only
    _check_layer(kind, e, n, 32, 32, seed=7, acts=((None, 0.0), ("prelu", 0.1)))


@pytest.mark.parametrize("kind", KINDS)
def test_prelu_and_relu_at_a_pre_activation_of_exactly_zero(kind):
    """An isolated node with a zero row and a zero bias has z = 0 exactly: the output is 0 and the derivative there is torch's
    (0 for ReLU, the slope for PReLU)."""
    import torch
    rs = np.random.RandomState(3)
    n, c = 20, 32
    e = gb.random_edges(rs, n, 60, loops="none")
    e = e[:, (e[0] != 5) & (e[1] != 5)]
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(n, c, generator=gen, dtype=torch.float64).float()
    x[5] = 0.0
    p = {k: v.float() for k, v in gb.random_layer_params(kind, c, c, gen).items()}
    for k in ("b", "bias", "bl"):
        if k in p:
            p[k] = torch.zeros_like(p[k])
    G = torch.randn(n, c, generator=gen, dtype=torch.float64).float()
    for act, slope in (("relu", 0.0), ("prelu", 0.1)):
        want, gw = _ref_layer(kind, e, x, p, act, slope, G)
        assert float(want[5].abs().max()) == 0.0
        out, _, (gx, gwa, gws, gb_) = _dev_layer(kind, e, n, x, p, act, slope, G)
        assert float(out[5].abs().max()) == 0.0
        assert gb.rel(gb_, gw["b"]) <= GRAD_TOL and gb.rel(gx, gw["x"]) <= GRAD_TOL and gb.rel(gwa, gw["wa"]) <= GRAD_TOL


# ---- the one-launch stack -----------------------------------------------------------------------------------------------------------
def _stack_params(kind, seed, dtype):
    import torch
    gen = torch.Generator().manual_seed(seed)
    return {name: gb.random_layer_params(kind, 1 if name == "conv1" else 32, 32, gen, dtype) for name in gb.ORDER}


def _stack_layers(kind, params):
    layers = []
    for name in gb.ORDER:
        wa, ws, b = gb.device_operands(kind, params[name])
        last = name == "conv3"
        act = (None if last else "relu") if kind == "GIN" else (None if last else "prelu")
        layers.append((wa.cuda(), None if ws is None else ws.cuda(), b.cuda(), act, 0.1 if act == "prelu" else 0.0))
    return layers


def _layer_by_layer(b, x, layers):
    from tlc_gnn_amd import ops
    for wa, ws, bias, act, slope in layers:
        x = ops.gnn_layer(b.rowptr, b.src, b.coef, b.self_scale, x, wa, ws, bias, act, slope)
    return x


def _stack_tolerance(kind, f, ei, p64):
    """max(2e-5, 4 x the distance of the float32 restatement on the CPU from its float64 value): four layers of float32."""
    import torch
    want = gb.stack(kind, f.double(), ei, p64)
    p32 = {name: {k: v.float() for k, v in d.items()} for name, d in p64.items()}
    d32 = gb.rel(gb.stack(kind, f.float(), ei, p32), want)
    assert d32 <= 1e-4, d32                                # float32 itself stays at its own rounding level
    tol = max(FWD_TOL, 4 * d32)
    print("stack %s: float32 restatement %.3g from float64, tolerance %.3g" % (kind, d32, tol))
    return want, tol


def _hand_cut(gptr, tile_nodes=192):
    """Whole graphs packed greedily into tiles of at most tile_nodes nodes: a caller-made cut (int32 node offsets)."""
    cuts = [0]
    for g in range(1, len(gptr)):
        if gptr[g] - cuts[-1] > tile_nodes:
            cuts.append(int(gptr[g - 1]))
    cuts.append(int(gptr[-1]))
    return np.array(sorted(set(cuts)), dtype=np.int32)


@pytest.mark.parametrize("sizes,n_tiles", [((64, 64, 63), 1), ((64, 64, 64), 1), ((64, 64, 65), 2), ((192,), 1), ((90, 50, 7, 1, 30, 96, 60, 3), 2)],
                         ids=["191", "192", "193", "one-of-192", "mixed"])
@pytest.mark.parametrize("kind", KINDS)
def test_stack_kernel_equals_the_layer_route_and_the_restatement(kind, sizes, n_tiles):
    """Tiles of 191 / 192 nodes worth of graphs, 193 nodes (a second tile), one graph of exactly 192 nodes -- cut by hand, whole graphs
    packed up to 192 nodes -- and, where the device's cut (tlc_gat_tile_cut: none for a graph above 96 nodes) gives one, that cut too."""
    import torch
    from tlc_gnn_amd import ops
    from tlc_gnn_amd.Knowledge_Distillation.gnn_layers import GnnBatch
    rs = np.random.RandomState(sum(sizes))
    _, ei, gptr, _ = gb.batch_of(rs, sizes)
    N = int(gptr[-1])
    f = torch.tensor(rs.rand(N, 1), dtype=torch.float32)
    p64 = _stack_params(kind, 11, torch.float64)
    want, tol = _stack_tolerance(kind, f, ei, p64)
    b = GnnBatch(ei.cuda(), N, kind)
    cut = _hand_cut(gptr)
    assert len(cut) - 1 == n_tiles and cut[-1] == N and (np.diff(cut) <= 192).all()
    tiles = torch.tensor(cut).cuda()
    assert ops.gnn_stack_ok(1, 32, tiles)
    layers = _stack_layers(kind, p64)
    got = ops.gnn_stack(b.rowptr, b.src, b.coef, b.self_scale, tiles, f.cuda(), layers)
    by_layer = _layer_by_layer(b, f.cuda(), layers)
    assert torch.equal(got, by_layer)                      # the same device code, operation for operation
    assert torch.equal(got, ops.gnn_stack(b.rowptr, b.src, b.coef, b.self_scale, tiles, f.cuda(), layers))
    assert gb.rel(got, want) <= tol, (gb.rel(got, want), tol)
    dev = b.tiles
    assert (dev is None) == (max(sizes) > 96)
    if dev is not None:
        t = dev.cpu().numpy()
        assert t[0] == 0 and t[-1] == N and (np.diff(t) <= 192).all() and (np.diff(t) >= 1).all()
        assert torch.equal(ops.gnn_stack(b.rowptr, b.src, b.coef, b.self_scale, dev, f.cuda(), layers), got)


def test_stack_kernel_marks_a_tile_above_192_rows_instead_of_overrunning():
    import torch
    from tlc_gnn_amd import ops
    from tlc_gnn_amd.Knowledge_Distillation.gnn_layers import GnnBatch
    rs = np.random.RandomState(6)
    _, ei, gptr, _ = gb.batch_of(rs, (20, 193, 20))
    N = int(gptr[-1])
    b = GnnBatch(ei.cuda(), N, "GIN")
    layers = _stack_layers("GIN", _stack_params("GIN", 1, torch.float64))
    f = torch.rand(N, 1).cuda()
    got = ops.gnn_stack(b.rowptr, b.src, b.coef, b.self_scale, torch.tensor(gptr.astype(np.int32)).cuda(), f, layers)
    want = _layer_by_layer(b, f, layers)
    assert torch.equal(got[:20], want[:20]) and torch.equal(got[213:], want[213:]) and bool(torch.isnan(got[20:213]).all())


@pytest.mark.parametrize("kind", KINDS)
def test_a_graph_above_the_tile_goes_layer_by_layer_with_the_same_values(kind):
    """One graph of 193 nodes among small ones: no cut at that graph, Base_Model runs its four layers one by one."""
    import torch
    from tlc_gnn_amd.Knowledge_Distillation.Teacher_model import Teacher_Model
    from tlc_gnn_amd.Knowledge_Distillation.gnn_layers import GnnBatch
    rs = np.random.RandomState(193)
    _, ei, gptr, _ = gb.batch_of(rs, (10, 193, 12))
    N = int(gptr[-1])
    f = torch.tensor(rs.rand(N, 1), dtype=torch.float32)
    torch.manual_seed(2)
    model = Teacher_Model(type=kind)
    _randomise_biases(model)
    params, _ = gb.teacher_params(model, kind)
    p64 = {name: {k: v.detach() for k, v in params[name].items()} for name in gb.ORDER}
    want, tol = _stack_tolerance(kind, f, ei, p64)
    model = model.cuda().eval()
    eid = ei.cuda()
    b = GnnBatch(eid, N, kind)
    assert b.tiles is None
    with torch.no_grad():
        got = model.DIM0_Model(f.cuda(), eid, csr=b)
    assert gb.rel(got, want) <= tol


def test_more_tiles_than_the_launch_has_workgroups():
    """The stack kernel walks the tiles from a fixed grid of two workgroups per CU: 1 100 graphs of 96 nodes are a tile each, more
    than any device's grid."""
    import torch
    from tlc_gnn_amd import ops
    from tlc_gnn_amd.Knowledge_Distillation.gnn_layers import GnnBatch
    kind = "SAGE"
    rs = np.random.RandomState(8)
    _, ei, gptr, _ = gb.batch_of(rs, (96,) * 1100, extra=0.5)
    N = int(gptr[-1])
    f = torch.tensor(rs.rand(N, 1), dtype=torch.float32)
    p64 = _stack_params(kind, 5, torch.float64)
    want, tol = _stack_tolerance(kind, f, ei, p64)
    b = GnnBatch(ei.cuda(), N, kind)
    assert b.tiles is not None and b.tiles.numel() - 1 > 2 * torch.cuda.get_device_properties(0).multi_processor_count
    layers = _stack_layers(kind, p64)
    got = ops.gnn_stack(b.rowptr, b.src, b.coef, b.self_scale, b.tiles, f.cuda(), layers)
    assert torch.equal(got, _layer_by_layer(b, f.cuda(), layers))
    assert gb.rel(got, want) <= tol


# ---- determinism ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_rows_are_the_same_bits_alone_and_inside_a_batch_of_300_and_from_run_to_run(kind):
    import torch
    from tlc_gnn_amd import ops
    from tlc_gnn_amd.Knowledge_Distillation.gnn_layers import GnnBatch
    rs = np.random.RandomState(300)
    sizes = tuple(int(v) for v in rs.randint(2, 24, size=300))
    graphs, ei, gptr, eptr = gb.batch_of(rs, sizes)
    N = int(gptr[-1])
    gen = torch.Generator().manual_seed(300)
    x = torch.randn(N, 32, generator=gen).cuda()
    G = torch.randn(N, 32, generator=gen).cuda()
    f = torch.rand(N, 1, generator=gen).cuda()
    p = {k: v.float() for k, v in gb.random_layer_params(kind, 32, 32, gen).items()}
    wa, ws, bias = (None if t is None else t.cuda() for t in gb.device_operands(kind, p))
    layers = _stack_layers(kind, _stack_params(kind, 4, torch.float64))

    def run(b, xs, Gs, fs):
        out, agg = ops.gnn_layer(b.rowptr, b.src, b.coef, b.self_scale, xs, wa, ws, bias, "prelu", 0.1, want_agg=True)
        grads = ops.gnn_layer_bwd(*b.transpose(), b.self_scale, xs, agg, out, Gs, wa, ws, True, "prelu", 0.1)
        st = ops.gnn_stack(b.rowptr, b.src, b.coef, b.self_scale, b.tiles, fs, layers)
        return out, agg, grads, st

    whole = GnnBatch(ei.cuda(), N, kind)
    out, agg, grads, st = run(whole, x, G, f)
    out2, agg2, grads2, st2 = run(GnnBatch(ei.cuda(), N, kind), x, G, f)
    assert torch.equal(out, out2) and torch.equal(agg, agg2) and torch.equal(st, st2)
    for a, c in zip(grads, grads2):                        # gX and the weight gradients, run to run
        assert (a is None and c is None) or torch.equal(a, c)
    for g, (n, e) in enumerate(graphs):
        lo, hi = int(gptr[g]), int(gptr[g + 1])
        o1, a1, g1, s1 = run(GnnBatch(gb.with_loops(n, e).cuda(), n, kind), x[lo:hi].contiguous(), G[lo:hi].contiguous(), f[lo:hi].contiguous())
        assert torch.equal(o1, out[lo:hi]) and torch.equal(a1, agg[lo:hi]) and torch.equal(g1[0], grads[0][lo:hi]) and torch.equal(s1, st[lo:hi]), g


# ---- the teacher -----------------------------------------------------------------------------------------------------------------------
def _teacher_case(seed, n_graphs=12):
    import torch
    rs = np.random.RandomState(seed)
    sizes = tuple(int(v) for v in rs.randint(5, 40, size=n_graphs))
    graphs, ei, gptr, eptr = gb.batch_of(rs, sizes, extra=1.5)
    fs = [torch.tensor(rs.rand(n, 1), dtype=torch.float32) for n, _ in graphs]
    pds = []
    for _, e in graphs:
        bb = rs.rand(e.shape[1])
        pds.append(torch.tensor(np.stack([bb, bb + rs.uniform(0, 0.6, size=e.shape[1])], 1), dtype=torch.float32))
    return graphs, ei, gptr, eptr, fs, pds


def _randomise_biases(model):
    import torch
    with torch.no_grad():
        for name, p in model.DIM0_Model.named_parameters():
            if name.endswith("bias") and not name.startswith("BN"):
                p.uniform_(-0.2, 0.2)


@pytest.mark.parametrize("order", [2, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_teacher_training_step_on_a_batch_of_12_graphs(kind, order):
    """model(f, edge_index, PD, kernel='wasserstein', p, grad_PI=False, graph_ptr, edge_ptr); loss0.backward(): the batch step equals the
    sum over its graphs, every parameter gradient against autograd of the restatement run graph by graph (the loss expression on the
    device's matching, a constant of the differentiation), and the eval forward equals the train-route forward."""
    import torch
    from oracle import w2_ref
    from tlc_gnn_amd import ops
    from tlc_gnn_amd.Knowledge_Distillation.Teacher_model import Teacher_Model
    graphs, ei, gptr, eptr, fs, pds = _teacher_case(12 + order)
    torch.manual_seed(3)
    model = Teacher_Model(type=kind, dropout=0.0)
    _randomise_biases(model)
    params, leaves = gb.teacher_params(model, kind)
    model = model.cuda().train()
    gp, ep = torch.tensor(gptr).cuda(), torch.tensor(eptr).cuda()
    x0, img, loss0, lxy, lxd, lyd, _, _ = model(torch.cat(fs).cuda(), ei.cuda(), torch.cat(pds).cuda(), kernel='wasserstein', p=order,
                                                grad_PI=False, graph_ptr=gp, edge_ptr=ep)
    assert img.shape == (12, 25) and loss0.shape == (1,) and loss0.requires_grad and not img.requires_grad
    loss0.backward()
    r = ops.w2_partial_matching(ep, x0.detach().double(), ep, torch.cat(pds).double().cuda(), order=order)
    assign = r["assign"].cpu().numpy()
    total = 0.0
    for b, (n, e) in enumerate(graphs):
        _, pd_ref = gb.teacher_forward(kind, fs[b].double(), gb.with_loops(n, e), params)
        assert gb.rel(x0[eptr[b]:eptr[b + 1]], pd_ref) <= 5e-5, b          # (five layers deep; the per-graph bound of test_gpu_train.py:430)
        total = total + w2_ref.loss_torch(pd_ref, pds[b].double(), assign[eptr[b]:eptr[b + 1]], order)
    assert abs(float(loss0.detach()) - float(total.detach())) <= 1e-5 * max(1.0, abs(float(total.detach())))
    total.backward()
    named = dict(model.named_parameters())
    for name, leaf in leaves.items():
        got = named[name].grad
        assert got is not None, name
        assert gb.rel(got.reshape(leaf.shape), leaf.grad) <= GRAD_TOL, (name, gb.rel(got.reshape(leaf.shape), leaf.grad))
    assert len(leaves) == 4 + 4 * {"GIN": 2, "GCN": 2, "SAGE": 3}[kind]
    for name in ("lin1.weight", "lin2.weight", "DIM0_Model.conv5." + ("nn.0.weight" if kind == "GIN" else "weight" if kind == "GCN" else "lin_l.weight")):
        assert named[name].grad is None                                     # not on the path
    # eval: the one-launch stack, the fused head, the imager -- the same points and images
    model.eval()
    with torch.no_grad():
        xe, img_e, l0, *_ = model(torch.cat(fs).cuda(), ei.cuda(), None, compute_loss=False, grad_PI=False, graph_ptr=gp, edge_ptr=ep)
    assert l0 is None and gb.rel(xe, x0) <= FWD_TOL and gb.rel(img_e, img) <= FWD_TOL


@pytest.mark.parametrize("kind", KINDS)
def test_teacher_train_mode_dropout_draws_the_masks_of_the_same_seed(kind):
    """Train mode with dropout 0.2: F.dropout in front of every layer (Teacher_model.py:219-240) and between lin5 and lin6 (:58), on
    tensors of the reference's shapes, so one seed draws the restatement's masks."""
    import torch
    import torch.nn.functional as F
    from tlc_gnn_amd.Knowledge_Distillation.Teacher_model import Teacher_Model
    rs = np.random.RandomState(5)
    n = 50
    e = gb.connected_graph(rs, n, 90)
    m = e.shape[1]
    ei = gb.with_loops(n, e)
    f = torch.tensor(rs.rand(n, 1), dtype=torch.float32)
    bb = rs.rand(m)
    PD = torch.tensor(np.stack([bb, bb + rs.uniform(0, 0.6, size=m)], 1), dtype=torch.float32)
    torch.manual_seed(5)
    model = Teacher_Model(type=kind, dropout=0.2)
    _randomise_biases(model)
    params, _ = gb.teacher_params(model, kind)
    model = model.cuda().train()
    torch.cuda.manual_seed(1234)
    x0, _, loss0, *_ = model(f.cuda(), ei.cuda(), PD.cuda(), kernel='wasserstein', p=2, grad_PI=False)
    torch.cuda.manual_seed(1234)
    masks = [F.dropout(torch.ones(shape, device="cuda"), p=0.2, training=True).cpu().double() for shape in ((n, 1), (n, 32), (n, 32), (n, 32), (m, 32))]
    assert all(0.05 < float((mk == 0).float().mean()) < 0.5 for mk in masks[1:])
    with torch.no_grad():
        _, pd_ref = gb.teacher_forward(kind, f.double(), ei, params, masks=masks)
        _, pd_eval = gb.teacher_forward(kind, f.double(), ei, params)
    assert gb.rel(x0, pd_ref) <= FWD_TOL
    assert gb.rel(x0, pd_eval) > 1e-2                                       # (the masks did something)
    assert bool(torch.isfinite(loss0).all())


@pytest.mark.parametrize("kind", KINDS)
def test_thirty_adam_steps_reduce_the_diagram_loss(kind):
    import torch
    from tlc_gnn_amd.Knowledge_Distillation.Teacher_model import Teacher_Model
    graphs, ei, gptr, eptr, fs, pds = _teacher_case(30, n_graphs=4)
    torch.manual_seed(5)
    model = Teacher_Model(type=kind, dropout=0.0).cuda().train()
    opt = torch.optim.Adam(model.parameters(), lr=5e-3)
    f, eid, PD = torch.cat(fs).cuda(), ei.cuda(), torch.cat(pds).cuda()
    gp, ep = torch.tensor(gptr).cuda(), torch.tensor(eptr).cuda()
    losses = []
    for _ in range(30):
        opt.zero_grad()
        loss0 = model(f, eid, PD, kernel='wasserstein', p=2, grad_PI=False, graph_ptr=gp, edge_ptr=ep)[2]
        loss0.backward()
        opt.step()
        losses.append(float(loss0.detach()))
    print("%s: diagram loss %.6g -> %.6g" % (kind, losses[0], losses[-1]))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses


def test_teacher_with_the_reference_defaults_runs_and_evaluate_packed_takes_it():
    """Teacher_Model() is type='GIN': inference on one graph (no graph_ptr), and data_utils_GC.evaluate_packed on a packed ground truth."""
    import torch
    import gc_cases as gc
    from tlc_gnn_amd.Knowledge_Distillation import data_utils_GC as kd
    from tlc_gnn_amd.Knowledge_Distillation.Teacher_model import Teacher_Model
    torch.manual_seed(5)
    model = Teacher_Model().cuda().eval()
    assert model.DIM0_Model.type == "GIN"
    rs = np.random.RandomState(1)
    n = 30
    e = gb.connected_graph(rs, n, 40)
    with torch.no_grad():
        pd_hat, img, *rest = model(torch.rand(n, 1).cuda(), gb.with_loops(n, e).cuda(), None, compute_loss=False, grad_PI=False)
    assert pd_hat.shape == (e.shape[1], 2) and img.shape == (25,) and rest[0] is None and bool(torch.isfinite(img).all())
    gt = kd.ground_truth_packed(*kd.pack_dataset(gc.route_graphs()[:60]), filt="degree")
    imgs, kept = kd.evaluate_packed(model, gt)
    assert imgs.shape == (len(kept), 25) and len(kept) > 30 and bool(torch.isfinite(imgs).all())
    ref_img, ref_kept = kd.evaluate_batch(model, gt.tuples())                # the same batch built from the per-sample tuples
    assert ref_kept == kept and gb.rel(imgs, ref_img) <= FWD_TOL


# ---- refusals of the C ABI -----------------------------------------------------------------------------------------------------------
def test_c_abi_refuses_unsupported_widths_and_null_pointers_and_writes_nothing():
    import torch
    from tlc_gnn_amd import _lib
    L = _lib.lib()
    n = 8
    rowptr = torch.arange(n + 1, dtype=torch.int32).cuda()
    src = torch.arange(n, dtype=torch.int32).cuda()
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    s = _lib.stream_ptr()

    def fwd(c_in, c_out, x=True, wa=True, out=True, rp=True, act=0, slope=0.0):
        X = torch.ones(n, max(c_in, 1)).cuda()
        W = torch.ones(max(c_out, 1), max(c_in, 1)).cuda()
        O = torch.full((n, max(c_out, 1)), 7.0).cuda()
        rc = L.tlc_gnn_layer_fwd(n, P(rowptr) if rp else None, P(src), None, C.c_float(1.0), P(X) if x else None, c_in, c_out, P(W) if wa else None,
                                 None, None, act, C.c_float(slope), P(O) if out else None, None, s)
        torch.cuda.synchronize()
        assert bool((O == 7.0).all()) or rc == 0
        return rc

    assert fwd(32, 32) == 0
    for c_in, c_out in ((65, 32), (0, 32), (32, 2), (32, 24), (32, 128)):
        assert fwd(c_in, c_out) == 4, (c_in, c_out)                          # TLC_ERR_UNSUPPORTED
    assert fwd(32, 32, x=False) == 1 and fwd(32, 32, wa=False) == 1 and fwd(32, 32, out=False) == 1 and fwd(32, 32, rp=False) == 1
    assert fwd(32, 32, act=3) == 1 and fwd(32, 32, act=2, slope=0.0) == 1    # TLC_ERR_INVALID_ARG
    # backward: widths, null pointers, a scratch one byte short
    X = torch.ones(n, 32).cuda()
    W = torch.ones(32, 32).cuda()
    gW = torch.full((32, 32), 7.0).cuda()
    nbytes = L.tlc_gnn_layer_bwd_work_bytes(n, 32, 32)
    work = torch.empty(nbytes, dtype=torch.uint8).cuda()

    def bwd(c_in=32, c_out=32, gwa=True, gout=True, wb=nbytes, gx=False, csr_t=False):
        rc = L.tlc_gnn_layer_bwd(n, P(rowptr) if csr_t else None, P(src) if csr_t else None, None, C.c_float(1.0), P(X), P(X), P(X),
                                 P(X) if gout else None, c_in, c_out, P(W), None, 0, C.c_float(0.0), P(X.clone()) if gx else None,
                                 P(gW) if gwa else None, None, None, P(work), C.c_int64(wb), s)
        torch.cuda.synchronize()
        return rc

    assert bwd(c_out=24) == 4 and bwd(c_in=65) == 4
    assert bwd(gwa=False) == 1 and bwd(gout=False) == 1 and bwd(wb=nbytes - 1) == 1 and bwd(gx=True, csr_t=False) == 1
    assert bool((gW == 7.0).all())
    assert bwd() == 0 and float(gW[0, 0]) == float(n)                        # dZ^T agg with all ones
    # the stack: another width is refused, and the Python side routes by gnn_stack_ok
    from tlc_gnn_amd import ops
    tiles = torch.tensor([0, n], dtype=torch.int32).cuda()
    arr = (C.c_void_p * 12)(*([W.data_ptr(), None, None] * 4))
    acts, slopes = (C.c_int32 * 4)(0, 0, 0, 0), (C.c_float * 4)(0, 0, 0, 0)
    O = torch.full((n, 32), 7.0).cuda()
    assert L.tlc_gnn_stack_fwd(n, P(rowptr), P(src), None, C.c_float(1.0), 1, P(tiles), P(X), 64, arr, acts, slopes, P(O), s) == 4
    assert L.tlc_gnn_stack_fwd(n, P(rowptr), P(src), None, C.c_float(1.0), 1, P(tiles), None, 32, arr, acts, slopes, P(O), s) == 1
    torch.cuda.synchronize()
    assert bool((O == 7.0).all())
    assert not ops.gnn_stack_ok(1, 64, tiles) and not ops.gnn_stack_ok(32, 32, tiles) and not ops.gnn_stack_ok(1, 32, None)
    assert ops.gnn_stack_ok(1, 32, tiles)

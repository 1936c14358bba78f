"""GPU: the PDGNN layer family (csrc/msg_layers.hip; ops.msg_layer / msg_layer_bwd / csr_transpose_pos; autograd.MsgLayer; GATConv's
new_node_feat / use_edge_attn ablations, PDConv, Teacher_Model(type='GAT') with the flags) against the float64 torch restatement of
tests/msg_layer_cases.py with autograd.  Tolerances are the project's for this precision class (tests/test_gpu_train.py:128-171): max-abs
difference over max-abs reference <= 2e-5 for a forward, <= 1e-4 for every gradient; determinism is compared with torch.equal."""
import ctypes as C

import numpy as np
import pytest

import msg_layer_cases as mc

pytestmark = pytest.mark.gpu

FWD_TOL, GRAD_TOL = 2e-5, 1e-4
NEW_MODES = ((True, False), (False, True), (False, False))           # (node_feat, edge_attn) with a flag off
GRAD_KEYS = ("x", "wl", "att", "wij", "bias")


def _csr(e, n):
    """(rowptr, col) int32 CUDA of a final entry list e [2, nnz] (CPU int64), sources ascending inside a row."""
    import torch
    key = e[1] * n + e[0]
    order = torch.sort(key, stable=True).indices
    rowptr = torch.zeros(n + 1, dtype=torch.int32)
    rowptr[1:] = torch.cumsum(torch.bincount(e[1], minlength=n), 0)
    return rowptr.cuda(), e[0][order].to(torch.int32).cuda()


def _dev_layer(csr, n, x, p, nf, ea, agg, slope, G=None, need_gx=True):
    """The device layer on a CSR by target: (out, grads or None); grads as GRAD_KEYS (None where the switch is off)."""
    import torch
    from tlc_gnn_amd import ops
    rowptr, col = csr
    mode = ops.msg_mode(nf, ea)
    d = {k: v.to(torch.float32).cuda() for k, v in p.items()}
    xd = x.to(torch.float32).cuda()
    out = ops.msg_layer(rowptr, col, xd, d["wl"], d["att"], d["wij"], d["bias"], mode, agg, slope)
    if G is None:
        return out, None
    t = ops.csr_transpose_pos(rowptr, col, n)
    grads = ops.msg_layer_bwd(rowptr, col, *t, xd, d["wl"], d["att"], d["wij"], mode, agg, slope, out, G.to(torch.float32).cuda(), need_gx=need_gx)
    return out, dict(zip(GRAD_KEYS, grads))


def _ref_layer(e, x, p, nf, ea, agg, slope, G):
    """float64 restatement with autograd on the final entry list e."""
    xr = x.double().clone().requires_grad_()
    pr = {k: v.double().clone().requires_grad_() for k, v in p.items()}
    out = mc.layer(xr, e, pr, nf, ea, agg, slope, edges_as_given=True)
    (out * G.double()).sum().backward()
    g = {"x": xr.grad, "wl": pr["wl"].grad, "att": pr["att"].grad if ea else None, "wij": pr["wij"].grad if nf else None, "bias": pr["bias"].grad}
    return out.detach(), g


def _case(seed, n, c_in, c_out, att_scale=1.0):
    import torch
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(n, c_in, generator=gen, dtype=torch.float64).float()
    p = {k: v.float() for k, v in mc.random_layer_params(c_in, c_out, gen, att_scale=att_scale).items()}
    G = torch.randn(n, 2 * c_out, generator=gen, dtype=torch.float64).float()
    return x, p, G


def _check(e, n, c_in, c_out, seed, modes=mc.MODES, aggs=mc.AGGS, slopes=(-1.0, 0.1), need_gx=True, tag=""):
    """Forward and every gradient of the device layer on the final entry list e against the restatement."""
    x, p, G = _case(seed, n, c_in, c_out)
    csr = _csr(e, n)
    for nf, ea in modes:
        for agg in aggs:
            for slope in slopes:
                out, g = _dev_layer(csr, n, x, p, nf, ea, agg, slope, G, need_gx)
                ref, gr = _ref_layer(e, x, p, nf, ea, agg, slope, G)
                what = (tag, n, c_in, c_out, nf, ea, agg, slope)
                print(what, "fwd %.3g" % mc.rel(out, ref), " ".join("%s %.3g" % (k, mc.rel(g[k], gr[k])) for k in GRAD_KEYS if g[k] is not None))
                assert mc.rel(out, ref) <= FWD_TOL, what
                for k in GRAD_KEYS:
                    if k == "x" and not need_gx:
                        assert g[k] is None
                    elif gr[k] is None:
                        assert g[k] is None, (what, k)
                    else:
                        assert mc.rel(g[k].reshape(gr[k].shape), gr[k]) <= GRAD_TOL, (what, k, mc.rel(g[k].reshape(gr[k].shape), gr[k]))


# ---- every configuration ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("node_feat,edge_attn", mc.MODES)
@pytest.mark.parametrize("c_in,c_out,n", [(1, 32, 65), (64, 16, 63), (17, 8, 130), (33, 64, 64)])
def test_forward_and_every_gradient_match_autograd_of_the_restatement(c_in, c_out, n, node_feat, edge_attn):
    rs = np.random.RandomState(c_in + n)
    e = mc.looped(mc.random_edges(rs, n, 4 * n, loops="some", repeats=True), n)
    _check(e, n, c_in, c_out, seed=7 * c_in + n, modes=((node_feat, edge_attn),))


# ---- kernel edges -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c_in", [15, 16, 17, 63, 64])
def test_input_widths_at_the_mfma_k_block(c_in):
    rs = np.random.RandomState(c_in)
    e = mc.looped(mc.random_edges(rs, 65, 200, loops="some", repeats=True), 65)
    _check(e, 65, c_in, 16, seed=c_in, modes=NEW_MODES, aggs=("sum_minmax",), slopes=(0.1,))


@pytest.mark.parametrize("n", [63, 64, 65, 127, 128, 129])
def test_node_counts_at_the_row_group(n):
    rs = np.random.RandomState(n)
    e = mc.looped(mc.random_edges(rs, n, 3 * n, loops="some", repeats=True), n)
    _check(e, n, 5, 32, seed=n, modes=NEW_MODES, aggs=("sum_min",), slopes=(-1.0,))


def test_a_node_whose_only_entry_is_its_self_loop():
    rs = np.random.RandomState(11)
    raw = mc.random_edges(rs, 40, 160, loops="none", repeats=False)
    raw = raw[:, (raw[1] != 0) & (raw[1] != 39)]                          # nodes 0 and 39 receive nothing but their loop
    _check(mc.looped(raw, 40), 40, 6, 16, seed=11, slopes=(0.1,))


@pytest.mark.parametrize("c_out", [8, 64])
def test_rows_of_63_64_and_65_entries(c_out):
    _check(mc.looped(mc.rows_of(80, [63, 64, 65]), 80), 80, 4, c_out, seed=63 + c_out, aggs=("sum_minmax",), slopes=(-1.0,))


def test_a_hub_row_of_1000_entries_and_a_source_with_1000_out_entries():
    n = 1003
    e = mc.looped(mc.hub_edges(n, 3, 999), n)
    assert int((e[1] == 3).sum()) == 1000 and int((e[0] == 3).sum()) == 1000
    _check(e, n, 4, 16, seed=1000, aggs=("sum_minmax",), slopes=(0.1,))


def test_a_first_layer_wants_no_input_gradient():
    rs = np.random.RandomState(12)
    e = mc.looped(mc.random_edges(rs, 70, 250, loops="some", repeats=True), 70)
    _check(e, 70, 1, 32, seed=12, aggs=("sum_minmax",), slopes=(0.1,), need_gx=False)


def test_an_empty_row_through_the_abi_is_the_bias_and_takes_no_gradient():
    import torch
    rs = np.random.RandomState(13)
    e = mc.looped(mc.random_edges(rs, 50, 150, loops="some", repeats=True), 50)
    e = e[:, (e[1] != 7) & (e[1] != 49)]                                  # rows 7 and 49 (the last) without entries
    _check(e, 50, 6, 16, seed=13, slopes=(-1.0,))
    x, p, G = _case(13, 50, 6, 16)
    out, _ = _dev_layer(_csr(e, 50), 50, x, p, True, True, "sum_minmax", -1.0)
    assert torch.equal(out[7].cpu(), p["bias"]) and torch.equal(out[49].cpu(), p["bias"])


def test_a_source_id_outside_the_batch_makes_its_row_nan_and_reads_nothing():
    import torch
    rs = np.random.RandomState(14)
    e = mc.looped(mc.random_edges(rs, 20, 60, loops="none", repeats=False), 20)
    rowptr, col = _csr(e, 20)
    bad = col.clone()
    k = int(rowptr[5])
    bad[k] = 1 << 30
    x, p, G = _case(14, 20, 3, 8)
    for nf, ea in mc.MODES:
        good, _ = _dev_layer((rowptr, col), 20, x, p, nf, ea, "sum_minmax", -1.0)
        out, _ = _dev_layer((rowptr, bad), 20, x, p, nf, ea, "sum_minmax", -1.0)
        assert bool(torch.isnan(out[5]).all())
        keep = torch.arange(20) != 5
        assert torch.equal(out[keep], good[keep])


@pytest.mark.parametrize("node_feat", [True, False])
def test_softmax_with_logits_of_plus_and_minus_200(node_feat):
    import torch
    import torch.nn.functional as F
    n, c_in, c_out = 65, 4, 8
    rs = np.random.RandomState(200)
    e = mc.looped(mc.random_edges(rs, n, 4 * n, loops="some", repeats=True), n)
    x, p, G = _case(200, n, c_in, c_out, att_scale=260.0)
    alpha = (x.double() @ p["wl"].double().t()) @ p["att"].double()
    logit = F.leaky_relu(alpha[e[0]] + alpha[e[1]], 0.2)
    assert float(logit.max()) >= 200.0 and float((alpha[e[0]] + alpha[e[1]]).min()) <= -200.0
    out, _ = _dev_layer(_csr(e, n), n, x, p, node_feat, True, "sum_minmax", -1.0)
    ref = mc.layer(x.double(), e, {k: v.double() for k, v in p.items()}, node_feat, True, "sum_minmax", edges_as_given=True)
    print("logits in [%.1f, %.1f]: fwd %.3g" % (float(logit.min()), float(logit.max()), mc.rel(out, ref)))
    assert bool(torch.isfinite(out).all())
    assert mc.rel(out, ref) <= FWD_TOL


def test_prelu_at_a_pre_activation_of_exactly_zero_takes_the_slope():
    """Wl = 0 makes every message 0, so the channels with a zero bias have a pre-activation of exactly 0: torch's PReLU gives them the
    gradient slope * g, and so does the kernel (visible in gbias)."""
    import torch
    n, c_in, c_out = 33, 5, 8
    rs = np.random.RandomState(15)
    e = mc.looped(mc.random_edges(rs, n, 100, loops="some", repeats=True), n)
    x, p, G = _case(15, n, c_in, c_out)
    p["wl"] = torch.zeros_like(p["wl"])
    p["bias"][::2] = 0.0
    for nf, ea in NEW_MODES:
        out, g = _dev_layer(_csr(e, n), n, x, p, nf, ea, "sum_minmax", 0.1, G)
        ref, gr = _ref_layer(e, x, p, nf, ea, "sum_minmax", 0.1, G)
        assert bool((out[:, ::2] == 0).all())
        assert mc.rel(g["bias"], gr["bias"]) <= GRAD_TOL
        assert mc.rel(g["bias"][::2], 0.1 * G.double().sum(0)[::2]) <= GRAD_TOL


# ---- the two implementations of the full configuration check each other ---------------------------------------------------------------------
@pytest.mark.parametrize("c_in,c_out,n", [(1, 32, 65), (64, 16, 63), (33, 64, 64)])
def test_full_configuration_against_the_gat_layer_kernels(c_in, c_out, n):
    import torch
    from tlc_gnn_amd import ops
    rs = np.random.RandomState(n)
    e = mc.looped(mc.random_edges(rs, n, 4 * n, loops="some", repeats=True), n)
    rowptr, col = _csr(e, n)
    x, p, G = _case(n, n, c_in, c_out)
    d = {k: v.cuda() for k, v in p.items()}
    for slope in (-1.0, 0.1):
        out, g = _dev_layer((rowptr, col), n, x, p, True, True, "sum_minmax", slope, G)
        old = ops.gat_layer(rowptr, col, x.cuda(), d["wl"], d["att"], d["wij"], d["bias"], prelu_slope=slope)
        assert mc.rel(out, old) <= FWD_TOL
        og = dict(zip(GRAD_KEYS, ops.gat_layer_bwd(rowptr, col, x.cuda(), d["wl"], d["att"], d["wij"], slope, old, G.cuda())))
        for k in GRAD_KEYS:
            assert mc.rel(g[k].reshape(og[k].shape), og[k]) <= GRAD_TOL, (k, slope)


# ---- determinism -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("node_feat,edge_attn,agg", [(True, True, "sum_minmax"), (True, False, "sum_min"), (False, True, "sum_minmax"),
                                                      (False, False, "sum_minmax")])
def test_rows_are_the_same_bits_alone_and_inside_a_batch_of_300_and_from_run_to_run(node_feat, edge_attn, agg):
    import torch
    from tlc_gnn_amd import ops
    from tlc_gnn_amd.Knowledge_Distillation.gat_conv import GraphBatch
    rs = np.random.RandomState(300)
    sizes = tuple(int(v) for v in rs.randint(2, 24, size=300))
    graphs, ei, gptr, eptr = mc.batch_of(rs, sizes)
    N = int(gptr[-1])
    x, p, G = _case(300, N, 32, 32)
    x, G = x.cuda(), G.cuda()
    d = {k: v.cuda() for k, v in p.items()}
    mode = ops.msg_mode(node_feat, edge_attn)

    def run(b, xs, Gs):
        out = ops.msg_layer(b.rowptr, b.col, xs, d["wl"], d["att"], d["wij"], d["bias"], mode, agg, 0.1)
        grads = ops.msg_layer_bwd(b.rowptr, b.col, *b.transpose(), xs, d["wl"], d["att"], d["wij"], mode, agg, 0.1, out, Gs)
        return out, grads

    whole = GraphBatch(ei.cuda(), N, tiled=False)
    out, grads = run(whole, x, G)
    out2, grads2 = run(GraphBatch(ei.cuda(), N, tiled=False), x, G)
    assert torch.equal(out, out2)
    for a, c in zip(grads, grads2):                                        # gX and every weight gradient, run to run
        assert (a is None and c is None) or torch.equal(a, c)
    for g, (n, e) in enumerate(graphs):
        lo, hi = int(gptr[g]), int(gptr[g + 1])
        o1, g1 = run(GraphBatch(mc.with_loops(n, e).cuda(), n, tiled=False), x[lo:hi].contiguous(), G[lo:hi].contiguous())
        assert torch.equal(o1, out[lo:hi]) and torch.equal(g1[0], grads[0][lo:hi]), g


# ---- the teacher ---------------------------------------------------------------------------------------------------------------------------
def _teacher_case(seed, n_graphs=12):
    import torch
    rs = np.random.RandomState(seed)
    sizes = tuple(int(v) for v in rs.randint(5, 40, size=n_graphs))
    graphs, ei, gptr, eptr = mc.batch_of(rs, sizes, extra=1.5)
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
            if name.endswith("bias"):
                p.uniform_(-0.2, 0.2)


@pytest.mark.parametrize("order", [2, 1])
@pytest.mark.parametrize("node_feat,edge_attn", NEW_MODES)
def test_teacher_training_step_on_a_batch_of_12_graphs(node_feat, edge_attn, order):
    """model(f, edge_index, PD, kernel='wasserstein', p, grad_PI=False, graph_ptr, edge_ptr); loss0.backward(): every parameter gradient
    against autograd of the restatement run graph by graph (the loss expression on the device's matching, a constant of the
    differentiation), the predicted diagram per graph, and the eval forward against the train-mode forward."""
    import torch
    from oracle import w2_ref
    from tlc_gnn_amd import ops
    from tlc_gnn_amd.Knowledge_Distillation.Teacher_model import Teacher_Model
    graphs, ei, gptr, eptr, fs, pds = _teacher_case(12 + order)
    torch.manual_seed(3)
    model = Teacher_Model(type='GAT', dropout=0.0, new_node_feat=node_feat, use_edge_attn=edge_attn)
    _randomise_biases(model)
    params, leaves = mc.teacher_params(model, node_feat, edge_attn)
    model = model.cuda().train()
    gp, ep = torch.tensor(gptr).cuda(), torch.tensor(eptr).cuda()
    x0, img, loss0, lxy, lxd, lyd, _, _ = model(torch.cat(fs).cuda(), ei.cuda(), torch.cat(pds).cuda(), kernel='wasserstein', p=order,
                                                grad_PI=False, graph_ptr=gp, edge_ptr=ep)
    assert img.shape == (12, 25) and loss0.shape == (1,) and loss0.requires_grad
    loss0.backward()
    r = ops.w2_partial_matching(ep, x0.detach().double(), ep, torch.cat(pds).double().cuda(), order=order)
    assign = r["assign"].cpu().numpy()
    total = 0.0
    for b, (n, e) in enumerate(graphs):
        _, pd_ref = mc.teacher_forward(fs[b].double(), mc.with_loops(n, e), params, node_feat, edge_attn)
        assert mc.rel(x0[eptr[b]:eptr[b + 1]], pd_ref) <= 5e-5, b          # (five layers deep; the per-graph bound of test_gpu_train.py:430)
        total = total + w2_ref.loss_torch(pd_ref, pds[b].double(), assign[eptr[b]:eptr[b + 1]], order)
    total.backward()
    named = dict(model.named_parameters())
    for name, leaf in leaves.items():
        got = named[name].grad
        assert got is not None, name
        print(name, "%.3g" % mc.rel(got.reshape(leaf.shape), leaf.grad))
        assert mc.rel(got.reshape(leaf.shape), leaf.grad) <= GRAD_TOL, (name, mc.rel(got.reshape(leaf.shape), leaf.grad))
    assert len(leaves) == 4 + 4 * (2 + int(node_feat) + int(edge_attn))
    for name in ("lin1.weight", "DIM0_Model.conv5.lin_l.weight", "DIM0_Model.conv1.att_r") + (() if edge_attn else ("DIM0_Model.conv1.att_l",)):
        assert named[name].grad is None                                     # not on the path
    model.eval()
    with torch.no_grad():
        xe, img_e, l0, *_ = model(torch.cat(fs).cuda(), ei.cuda(), None, compute_loss=False, grad_PI=False, graph_ptr=gp, edge_ptr=ep)
    assert l0 is None and mc.rel(xe, x0) <= FWD_TOL and mc.rel(img_e, img) <= FWD_TOL


@pytest.mark.parametrize("node_feat,edge_attn", NEW_MODES)
def test_thirty_adam_steps_reduce_the_diagram_loss(node_feat, edge_attn):
    import torch
    from tlc_gnn_amd.Knowledge_Distillation.Teacher_model import Teacher_Model
    graphs, ei, gptr, eptr, fs, pds = _teacher_case(30, n_graphs=4)
    torch.manual_seed(5)
    model = Teacher_Model(type='GAT', dropout=0.0, new_node_feat=node_feat, use_edge_attn=edge_attn).cuda().train()
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
    print("new_node_feat=%s use_edge_attn=%s: diagram loss %.6g -> %.6g" % (node_feat, edge_attn, losses[0], losses[-1]))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses


def test_evaluate_packed_takes_an_ablated_teacher():
    import torch
    import gc_cases as gc
    from tlc_gnn_amd.Knowledge_Distillation import data_utils_GC as kd
    from tlc_gnn_amd.Knowledge_Distillation.Teacher_model import Teacher_Model
    torch.manual_seed(5)
    model = Teacher_Model(type='GAT', new_node_feat=False, use_edge_attn=False).cuda().eval()
    gt = kd.ground_truth_packed(*kd.pack_dataset(gc.route_graphs()[:60]), filt="degree")
    imgs, kept = kd.evaluate_packed(model, gt)
    assert imgs.shape == (len(kept), 25) and len(kept) > 30 and bool(torch.isfinite(imgs).all())
    ref_img, ref_kept = kd.evaluate_batch(model, gt.tuples())
    assert ref_kept == kept and mc.rel(imgs, ref_img) <= FWD_TOL


def test_with_both_flags_the_teacher_keeps_todays_route_bit_for_bit():
    """new_node_feat=True, use_edge_attn=True: GATConv and Teacher_Model.forward still run tlc_gat_layer_fwd / tlc_edge_head_fwd."""
    import torch
    from tlc_gnn_amd import ops
    from tlc_gnn_amd.Knowledge_Distillation.gat_conv import GraphBatch
    from tlc_gnn_amd.Knowledge_Distillation.Teacher_model import Teacher_Model
    graphs, ei, gptr, eptr, fs, pds = _teacher_case(40, n_graphs=6)
    torch.manual_seed(7)
    model = Teacher_Model(type='GAT', dropout=0.0, new_node_feat=True, use_edge_attn=True).cuda().train()
    f, eid = torch.cat(fs).cuda(), ei.cuda()
    x0 = model(f, eid, None, compute_loss=False, grad_PI=False, graph_ptr=torch.tensor(gptr).cuda(), edge_ptr=torch.tensor(eptr).cuda())[0]
    b = GraphBatch(eid, f.shape[0], tiled=False)
    d = model.DIM0_Model
    h = f
    with torch.no_grad():
        for conv, slope in ((d.conv1, 0.1), (d.conv2, 0.1), (d.conv4, 0.1), (d.conv3, -1.0)):
            h = ops.gat_layer(b.rowptr, b.col, h, conv.lin_l.weight, conv.att_l.reshape(-1), conv.lin_ij.weight, conv.bias, prelu_slope=slope)
        m = eid.shape[1] - f.shape[0]
        src, dst = b.edge_ends(m)
        want = ops.edge_head(src, dst, h, model.lin5.weight, model.lin5.bias, 0.1, model.lin6.weight, model.lin6.bias)
    assert x0.requires_grad and torch.equal(x0.detach(), want)


# ---- PDConv ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("node_feat", [True, False])
def test_a_pdconv_stack_built_as_base_models_pdgnn_branch_builds_it(node_feat):
    """Teacher_model.py:177-181: 1 -> 32, 64 -> 32, 64 -> 32, 64 -> 16, run conv1 -> conv2 -> conv4 -> conv3 with F.prelu(0.1) between."""
    import torch
    from tlc_gnn_amd.Knowledge_Distillation.gat_conv import GraphBatch
    from tlc_gnn_amd.Knowledge_Distillation.PD_conv import PDConv
    rs = np.random.RandomState(21)
    graphs, ei, gptr, eptr = mc.batch_of(rs, (30, 17, 64, 5), extra=1.5)
    N = int(gptr[-1])
    torch.manual_seed(21)
    convs = {"conv1": PDConv(1, 32, new_node_feat=node_feat), "conv2": PDConv(32, 32, double_input=True, new_node_feat=node_feat),
             "conv4": PDConv(32, 32, double_input=True, new_node_feat=node_feat), "conv3": PDConv(32, 16, double_input=True, new_node_feat=node_feat)}
    params, leaves = {}, {}
    for name, conv in convs.items():
        with torch.no_grad():
            conv.bias.uniform_(-0.2, 0.2)
        w = conv.weight.detach().double().clone().requires_grad_()
        bias = conv.bias.detach().double().clone().requires_grad_()
        params[name] = {"wl": w.t(), "bias": bias}
        leaves[name + ".weight"], leaves[name + ".bias"] = w, bias
        if node_feat:
            params[name]["wij"] = leaves[name + ".lin_ij.weight"] = conv.lin_ij.weight.detach().double().clone().requires_grad_()
        conv.cuda()
    gen = torch.Generator().manual_seed(21)
    f = torch.rand(N, 1, generator=gen)
    G = torch.randn(N, 32, generator=gen)
    eid = ei.cuda()
    batch = GraphBatch(eid, N, tiled=False)
    h = f.cuda()
    for name in mc.ORDER:
        h = convs[name](h, eid, prelu_slope=-1.0 if name == "conv3" else 0.1, csr=batch)
    ref = mc.stack(f.double(), ei, params, node_feat, False, "sum_min")
    print("PDConv stack, new_node_feat=%s: fwd %.3g" % (node_feat, mc.rel(h, ref)))
    assert h.shape == (N, 32) and mc.rel(h, ref) <= FWD_TOL
    (h * G.cuda()).sum().backward()
    (ref * G.double()).sum().backward()
    for name, conv in convs.items():
        for k, v in conv.named_parameters():
            want = leaves[name + "." + k].grad
            print(name, k, "%.3g" % mc.rel(v.grad, want))
            assert mc.rel(v.grad, want) <= GRAD_TOL, (name, k)
    with torch.no_grad():
        h2 = f.cuda()
        for name in mc.ORDER:
            h2 = convs[name](h2, eid, prelu_slope=-1.0 if name == "conv3" else 0.1)       # (no held batch: built per call)
    assert torch.equal(h2, h.detach())
    with torch.no_grad():                                                  # a (rowptr, col) pair, as GATConv takes; anything else raises
        pair = convs["conv1"](f.cuda(), eid, prelu_slope=0.1, csr=(batch.rowptr, batch.col))
        assert torch.equal(pair, convs["conv1"](f.cuda(), eid, prelu_slope=0.1, csr=batch))
        with pytest.raises(TypeError):
            convs["conv1"](f.cuda(), eid, csr="rowptr")


def test_gcn_norm_has_the_values_of_the_gcn_baselines_operator():
    """PD_conv.gcn_norm (edge-list form, torch ops) against ops.gcn_norm_csr (tlc_gcn_norm_csr: CSR by target, sources ascending) on a
    list with self loops and repeats: the same entries with the same values; both are float32, so 1e-6 relative."""
    import torch
    from tlc_gnn_amd import ops
    from tlc_gnn_amd.Knowledge_Distillation.PD_conv import gcn_norm
    rs = np.random.RandomState(31)
    n = 70
    ei = mc.random_edges(rs, n, 300, loops="some", repeats=True).cuda()
    e2, w = gcn_norm(ei, None, n, dtype=torch.float32)
    rowptr, col, val = ops.gcn_norm_csr(ei, n)
    order = torch.sort(e2[1] * n + e2[0], stable=True).indices
    assert int(rowptr[n]) == e2.shape[1] == col.numel()
    assert torch.equal(e2[0][order].to(torch.int32), col)
    assert torch.equal(torch.bincount(e2[1], minlength=n).cumsum(0).to(torch.int32), rowptr[1:])
    assert mc.rel(w[order], val) <= 1e-6


def test_the_wrappers_refuse_operands_of_the_wrong_shape():
    """The library cannot see a tensor's size: ops.msg_layer / msg_layer_bwd check the operands against c_out = wl.shape[0] first."""
    import torch
    from tlc_gnn_amd import ops
    n = 10
    rowptr, col = _csr(mc.looped(mc.random_edges(np.random.RandomState(2), n, 20), n), n)
    x, p, G = _case(2, n, 4, 8)
    d = {k: v.cuda() for k, v in p.items()}
    x, G = x.cuda(), G.cuda()
    ok = ops.msg_layer(rowptr, col, x, d["wl"], d["att"], d["wij"], d["bias"], 3)
    for bad in ({"wl": d["wl"][:, :3]}, {"att": d["att"][:7]}, {"wij": d["wij"][:, :15]}, {"bias": d["bias"][:15]}):
        q = {**d, **bad}
        with pytest.raises(ValueError):
            ops.msg_layer(rowptr, col, x, q["wl"], q["att"], q["wij"], q["bias"], 3)
    with pytest.raises(ValueError):
        ops.msg_layer(rowptr[:-1], col, x, d["wl"], d["att"], d["wij"], d["bias"], 3)
    t = ops.csr_transpose_pos(rowptr, col, n)
    with pytest.raises(ValueError):
        ops.msg_layer_bwd(rowptr, col, *t, x, d["wl"], d["att"], d["wij"], 3, "sum_minmax", -1.0, ok, G[:, :15].contiguous())
    with pytest.raises(ValueError):
        ops.msg_layer_bwd(rowptr, col, t[0], t[1], t[2][:-1], x, d["wl"], d["att"], d["wij"], 3, "sum_minmax", -1.0, ok, G)
    assert ops.msg_layer(rowptr, col, x, d["wl"], None, None, d["bias"], 0).shape == (n, 16)       # (switched off: not read, not checked)


# ---- refusals of the C ABI -----------------------------------------------------------------------------------------------------------------
def test_c_abi_refusals_write_nothing():
    import torch
    from tlc_gnn_amd import _lib
    L = _lib.lib()
    n, ci, co = 8, 32, 32
    rowptr = torch.arange(n + 1, dtype=torch.int32).cuda()
    src = torch.arange(n, dtype=torch.int32).cuda()
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    s = _lib.stream_ptr()
    X, Wl, att, Wij, bias = (torch.ones(*sh).cuda() for sh in ((n, 64), (64, 64), (64,), (64, 128), (128,)))
    fb = L.tlc_msg_layer_fwd_work_bytes(n, ci, co, 3)
    bb = L.tlc_msg_layer_bwd_work_bytes(n, n, ci, co, 3)
    assert fb > 0 and bb > fb and L.tlc_msg_layer_fwd_work_bytes(-1, ci, co, 3) == -1 and L.tlc_msg_layer_fwd_work_bytes(n, ci, co, 4) == -1
    assert L.tlc_msg_layer_bwd_work_bytes(n, -1, ci, co, 3) == -1 and L.tlc_msg_layer_bwd_work_bytes(n, 1 << 40, ci, co, 3) == bb
    work = torch.empty(2 * bb + 64, dtype=torch.uint8).cuda()

    def fwd(c_in=ci, c_out=co, mode=3, agg=0, n_=n, x=True, wl=True, a=True, wij=True, b=True, out=True, rp=True, wb=fb, woff=0):
        O = torch.full((n, 128), 7.0).cuda()
        rc = L.tlc_msg_layer_fwd(n_, P(rowptr) if rp else None, P(src), P(X) if x else None, c_in, c_out, P(Wl) if wl else None, P(att) if a else None,
                                 P(Wij) if wij else None, P(bias) if b else None, mode, agg, C.c_float(-1.0), C.c_void_p(work.data_ptr() + woff),
                                 C.c_int64(wb), P(O) if out else None, s)
        torch.cuda.synchronize()
        assert rc == 0 or bool((O == 7.0).all())
        return rc

    assert fwd() == 0 and fwd(mode=0, a=False, wij=False) == 0 and fwd(mode=1, a=False) == 0 and fwd(mode=2, wij=False) == 0
    for c_in, c_out in ((65, 32), (0, 32), (32, 2), (32, 24), (32, 128)):
        assert fwd(c_in, c_out) == 4, (c_in, c_out)                          # TLC_ERR_UNSUPPORTED
    assert fwd(x=False) == 1 and fwd(wl=False) == 1 and fwd(a=False) == 1 and fwd(wij=False) == 1 and fwd(b=False) == 1 and fwd(out=False) == 1
    assert fwd(rp=False) == 1 and fwd(n_=-1) == 1 and fwd(mode=4) == 1 and fwd(mode=-1) == 1 and fwd(agg=2) == 1          # TLC_ERR_INVALID_ARG
    assert fwd(wb=fb - 1) == 1 and fwd(woff=4, wb=fb) == 1                   # too small; not 16-byte aligned

    t = [torch.zeros(n + 1, dtype=torch.int32).cuda(), torch.arange(n, dtype=torch.int32).cuda(), torch.arange(n, dtype=torch.int32).cuda()]
    t[0] = rowptr.clone()
    out = torch.ones(n, 128).cuda()

    def bwd(c_in=ci, c_out=co, mode=3, agg=0, n_=n, gout=True, gwl=True, gatt=True, gwij=True, gb=True, tr=True, wb=bb, woff=0):
        outs = [torch.full(sh, 7.0).cuda() for sh in ((n, 64), (64, 64), (64,), (64, 128), (128,))]
        rc = L.tlc_msg_layer_bwd(n_, P(rowptr), P(src), P(t[0]) if tr else None, P(t[1]), P(t[2]), P(X), c_in, c_out, P(Wl), P(att), P(Wij), mode, agg,
                                 C.c_float(0.1), P(out), P(out) if gout else None, P(outs[0]), P(outs[1]) if gwl else None, P(outs[2]) if gatt else None,
                                 P(outs[3]) if gwij else None, P(outs[4]) if gb else None, C.c_void_p(work.data_ptr() + woff), C.c_int64(wb), s)
        torch.cuda.synchronize()
        assert rc == 0 or all(bool((o == 7.0).all()) for o in outs)
        return rc

    assert bwd() == 0 and bwd(mode=0, gatt=False, gwij=False) == 0
    for c_in, c_out in ((65, 32), (0, 32), (32, 2), (32, 24), (32, 128)):
        assert bwd(c_in, c_out) == 4, (c_in, c_out)
    assert bwd(gout=False) == 1 and bwd(gwl=False) == 1 and bwd(gatt=False) == 1 and bwd(gwij=False) == 1 and bwd(gb=False) == 1 and bwd(tr=False) == 1
    assert bwd(n_=-1) == 1 and bwd(mode=8) == 1 and bwd(agg=-1) == 1 and bwd(wb=bb - 1) == 1 and bwd(woff=8) == 1
    # n_nodes == 0: TLC_OK with zero weight gradients
    outs = [torch.full(sh, 7.0).cuda() for sh in ((co, ci), (co,), (co, 2 * co), (2 * co,))]
    rc = L.tlc_msg_layer_bwd(0, None, None, None, None, None, None, ci, co, P(Wl), P(att), P(Wij), 3, 0, C.c_float(-1.0), None, None, None,
                             P(outs[0]), P(outs[1]), P(outs[2]), P(outs[3]), None, C.c_int64(0), s)
    torch.cuda.synchronize()
    assert rc == 0 and all(bool((o == 0).all()) for o in outs)
    assert L.tlc_msg_layer_fwd(0, None, None, None, ci, co, P(Wl), P(att), P(Wij), P(bias), 3, 0, C.c_float(-1.0), None, C.c_int64(0), None, s) == 0

"""GPU: node classification on PDGNN images (Knowledge_Distillation/ConvCurv_GIN.py + pipelines_GIN.py) -- curvGN on the HIP kernels of
nc_curv.hip (tlc_nc_group, tlc_nc_linear_f32 / _bwd_f32, tlc_nc_curv_fwd_f32 / _bwd_f32) against torch restatements with autograd."""
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def _softmax(src, index, n):
    """PyG 1.6.1 softmax on any device: subtract the segment max, exp, divide by (segment sum + 1e-16)."""
    import torch
    idx = index.view(-1, 1).expand_as(src)
    mx = torch.full((n, src.shape[1]), float("-inf"), dtype=src.dtype, device=src.device)
    mx = mx.scatter_reduce(0, idx, src, reduce="amax", include_self=True)
    out = (src - mx[index]).exp()
    den = torch.zeros((n, src.shape[1]), dtype=src.dtype, device=src.device).index_add_(0, index, out)
    return out / (den[index] + 1e-16)


def _ref_layer(x, ei, w_mul, p, n, by="source", oracle_softmax=False, keep=None):
    """curvGN.forward (:159-170): lin, w_mlp_out = Linear(no bias) -> PReLU -> Linear, softmax grouped by edge_index[0], sum at
    edge_index[1].  by='target' groups the softmax by edge_index[1] instead (the wrong restatement of test 2)."""
    import torch
    import torch.nn.functional as F
    xl = F.linear(x, p["lin.weight"], p["lin.bias"])
    wt = F.linear(F.prelu(F.linear(w_mul, p["w_mlp_out.0.weight"]), p["w_mlp_out.1.weight"]), p["w_mlp_out.2.weight"], p["w_mlp_out.2.bias"])
    if keep is not None:
        wt.retain_grad()
        keep.append(wt)
    idx = ei[0] if by == "source" else ei[1]
    if oracle_softmax:
        from oracle import lp_forward_ref as ref
        alpha = ref.segment_softmax(wt, idx, n)
    else:
        alpha = _softmax(wt, idx, n)
    out = torch.zeros((n, xl.shape[1]), dtype=xl.dtype, device=xl.device).index_add(0, ei[1], alpha * xl[ei[0]])
    if "lin1.weight" in p:
        x1 = F.linear(x, p["lin1.weight"], p["lin1.bias"])
        out = torch.cat((out, x1), dim=-1) if p.get("_cat") else out + x1
    return out


def _graph(n=300, e_rand=1400, seed=0):
    """Directed random edges + a hub with 150 out-edges (its softmax spans chunks) + duplicates + self loops; node n-1 has only
    in-edges, n-2 only out-edges, n-3 .. n-6 no edge at all."""
    rs = np.random.RandomState(seed)
    m = n - 6
    src = rs.randint(0, m, e_rand)
    dst = rs.randint(0, m, e_rand)
    hub = np.stack([np.full(150, 7), rs.randint(0, m, 150)])
    dup = np.stack([src[:40], dst[:40]])
    loops = np.stack([np.arange(0, m, 3), np.arange(0, m, 3)])
    extra = np.array([[0, 1, 2, n - 2, n - 2], [n - 1, n - 1, n - 1, 3, 4]])
    ei = np.concatenate([np.stack([src, dst]), hub, dup, loops, extra], axis=1)
    return ei[:, rs.permutation(ei.shape[1])].astype(np.int64)


def _layer(torch, F_in, C, D=50, seed=0, skip_cat=False, skip_sum=False):
    from tlc_gnn_amd.Knowledge_Distillation.ConvCurv_GIN import curvGN
    torch.manual_seed(seed)
    conv = curvGN(F_in, C, dimension=5, skip_cat=skip_cat, skip_sum=skip_sum)
    with torch.no_grad():
        conv.w_mlp_out[1].weight.uniform_(0.05, 0.4)
        conv.w_mlp_out[2].bias.uniform_(-0.3, 0.3)
    assert D == 50
    return conv.cuda()


def _params(mod, dtype, device):
    return {k: v.detach().to(device=device, dtype=dtype).clone().requires_grad_(True) for k, v in mod.named_parameters()}


def _max_rel(a, b):
    return float((a.double() - b.double()).abs().max() / max(float(b.double().abs().max()), 1e-30))


# ---- 1. forward against the f64 restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 3, 7, 64, 256])
def test_layer_forward_matches_f64_restatement(C):
    torch = _torch()
    n, F_in = 300, 37
    ei = torch.from_numpy(_graph(n))
    rs = np.random.RandomState(C)
    x = torch.from_numpy(rs.randn(n, F_in)).float()
    w_mul = torch.from_numpy(rs.uniform(0, 0.5, (ei.shape[1], 50))).float()
    conv = _layer(torch, F_in, C)
    with torch.no_grad():
        got = conv(x.cuda(), ei.cuda(), w_mul.cuda())
    p = _params(conv, torch.float64, "cpu")
    with torch.no_grad():
        want = _ref_layer(x.double(), ei, w_mul.double(), p, n, oracle_softmax=True)
    assert got.shape == (n, C)
    err = float((got.cpu().double() - want).abs().max())
    assert err <= 1e-5 * float(want.abs().max()), (C, err, float(want.abs().max()))


# ---- 2. the softmax is grouped by SOURCE ------------------------------------------------------------------------------------------
def test_softmax_grouped_by_source_not_target():
    torch = _torch()
    n, F_in, C = 120, 16, 8
    rs = np.random.RandomState(5)
    # a directed graph whose out-degrees and in-degrees differ node by node
    src = np.concatenate([rs.randint(0, 20, 300), rs.randint(20, n, 100)])
    dst = rs.randint(0, n, 400)
    ei = torch.from_numpy(np.stack([src, dst]).astype(np.int64))
    x = torch.from_numpy(rs.randn(n, F_in)).float()
    w_mul = torch.from_numpy(rs.uniform(0, 1, (400, 50))).float()
    conv = _layer(torch, F_in, C, seed=1)
    with torch.no_grad():
        got = conv(x.cuda(), ei.cuda(), w_mul.cuda()).cpu().double()
        p = _params(conv, torch.float64, "cpu")
        by_src = _ref_layer(x.double(), ei, w_mul.double(), p, n, by="source")
        by_tgt = _ref_layer(x.double(), ei, w_mul.double(), p, n, by="target")
    assert float((by_src - by_tgt).abs().max()) > 1e-2
    assert float((got - by_src).abs().max()) <= 1e-5 * float(by_src.abs().max())


# ---- 3. edge cases ------------------------------------------------------------------------------------------------------------------
def test_edge_cases():
    torch = _torch()
    from tlc_gnn_amd import ops
    n, F_in, C = 10, 5, 4
    rs = np.random.RandomState(9)
    x = torch.from_numpy(rs.randn(n, F_in)).float()
    conv = _layer(torch, F_in, C, seed=2)
    p = _params(conv, torch.float64, "cpu")
    # E = 0: every row is zero
    e0 = torch.zeros((2, 0), dtype=torch.int64)
    with torch.no_grad():
        out0 = conv(x.cuda(), e0.cuda(), torch.zeros((0, 50)).cuda())
    assert out0.shape == (n, C) and bool((out0 == 0).all())
    # duplicates, a self loop, node 9 isolated, node 8 only out-edges, node 0 only in-edges
    ei = torch.tensor([[1, 1, 1, 2, 3, 8, 8, 5, 5], [0, 0, 2, 3, 3, 0, 4, 6, 0]], dtype=torch.int64)
    w_mul = torch.from_numpy(rs.uniform(0, 1, (ei.shape[1], 50))).float()
    with torch.no_grad():
        got = conv(x.cuda(), ei.cuda(), w_mul.cuda()).cpu().double()
        want = _ref_layer(x.double(), ei, w_mul.double(), p, n)
    assert float((got - want).abs().max()) <= 1e-5 * float(want.abs().max())
    for r in (1, 5, 7, 8, 9):                                   # no in-edges: zero rows
        assert bool((got[r] == 0).all()), r
    # the grouping keeps duplicates, in edge order
    g = ops.nc_group(ei.cuda(), n).cpu().numpy()
    src_ptr, src_eid = g[:n + 1], g[2 * (n + 1):2 * (n + 1) + ei.shape[1]]
    assert src_ptr.tolist() == [0, 0, 3, 4, 5, 5, 7, 7, 7, 9, 9]
    assert src_eid[:3].tolist() == [0, 1, 2]
    # ids outside [0, n) are refused
    with pytest.raises(ValueError):
        ops.nc_group(torch.tensor([[0, 1], [1, n]], dtype=torch.int64).cuda(), n)


# ---- 4. backward --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["plain", "skip_cat", "skip_sum"])
def test_layer_backward_matches_autograd(mode):
    torch = _torch()
    n, F_in, C = 300, 23, 64 if mode == "plain" else 7
    ei = torch.from_numpy(_graph(n, seed=3))
    rs = np.random.RandomState(11)
    x = torch.from_numpy(rs.randn(n, F_in)).float()
    w_mul = torch.from_numpy(rs.uniform(0, 0.5, (ei.shape[1], 50))).float()
    conv = _layer(torch, F_in, C, seed=4, skip_cat=mode == "skip_cat", skip_sum=mode == "skip_sum")
    C_out = 2 * C if mode == "skip_cat" else C
    gout = torch.from_numpy(rs.randn(n, C_out)).float()
    xg = x.cuda().requires_grad_(True)
    grads = []
    for _ in range(2):
        conv.zero_grad()
        xg.grad = None
        out = conv(xg, ei.cuda(), w_mul.cuda())
        out.backward(gout.cuda())
        grads.append({k: v.grad.detach().clone() for k, v in conv.named_parameters()} | {"x": xg.grad.detach().clone()})
    for k in grads[0]:                                           # deterministic: two backward calls, the same bits
        assert torch.equal(grads[0][k], grads[1][k]), k
    p = _params(conv, torch.float64, "cpu")
    if mode == "skip_cat":
        p["_cat"] = True
    xr = x.double().requires_grad_(True)
    wt = []
    _ref_layer(xr, ei, w_mul.double(), p, n, keep=wt).backward(gout.double())
    want = {k: v.grad for k, v in p.items() if k != "_cat"} | {"x": xr.grad}
    for k, w in want.items():
        got = grads[0][k].cpu().double()
        # element-wise rtol 1e-4; the atol only covers entries near zero: 2e-6 of the gradient's largest entry (observed: at most
        # 3.2e-7 of it).  d b2 = sum_e d wt[e] vanishes per source row (softmax): its scale is the size of the terms it sums.
        scale = float(wt[0].grad.abs().sum(0).max()) if k == "w_mlp_out.2.bias" else float(w.abs().max())
        bad = (got - w).abs() > 1e-4 * w.abs() + 2e-6 * scale
        assert not bool(bad.any()), (mode, k, float((got - w).abs().max()), scale)


# ---- 5. a whole PubMed-shaped step ------------------------------------------------------------------------------------------------
def _pubmed_like(torch, seed=0):
    from tlc_gnn_amd import synth
    from tlc_gnn_amd.data import Data
    n, edges, _, _, F_in = synth.shaped_graph("PubMed")
    und = torch.from_numpy(edges.T.copy()).long()
    loops = torch.arange(n)
    ei = torch.cat([und, und.flip(0), torch.stack([loops, loops])], dim=1)
    rs = np.random.RandomState(seed)
    x = torch.from_numpy(synth.synthetic_features(n, F_in)).float()
    y = torch.from_numpy(rs.randint(0, 3, n)).long()
    w_mul = torch.from_numpy(rs.uniform(0, 0.3, (ei.shape[1], 50)).astype(np.float32))
    w_mul[ei[0] == ei[1]] = 0
    data = Data(x=x, edge_index=ei, y=y).to("cuda")
    return data, w_mul.cuda(), F_in


def test_pubmed_shaped_step_matches_torch_restatement():
    torch = _torch()
    import torch.nn.functional as F
    from tlc_gnn_amd.Knowledge_Distillation import ConvCurv_GIN
    data, w_mul, F_in = _pubmed_like(torch)
    assert data.edge_index.shape[1] == 108365
    torch.manual_seed(0)
    model = ConvCurv_GIN.Net(data, "PubMed", F_in, 3, w_mul=w_mul).cuda()
    train_mask = torch.zeros(data.num_nodes, dtype=torch.bool, device="cuda")
    train_mask[:60] = True
    model.train()
    torch.manual_seed(123)
    logp = model(data)
    loss = F.nll_loss(logp[train_mask], data.y[train_mask])
    model.zero_grad()
    loss.backward()
    # the restatement, f32 on the GPU, the same dropout draws
    names = [k for k, v in model.named_parameters() if not k.startswith("modelGIN")]
    p = {k: v.detach().clone().requires_grad_(True) for k, v in model.named_parameters() if k in names}
    sub = lambda pre: {k[len(pre):]: v for k, v in p.items() if k.startswith(pre)}          # noqa: E731
    ei, n = data.edge_index, data.num_nodes
    torch.manual_seed(123)
    wt = []
    h = F.dropout(data.x, p=0.4, training=True)
    h = _ref_layer(h, ei, w_mul, sub("conv1."), n, keep=wt)
    h = F.dropout(F.elu(h), p=0.4, training=True)
    ref_logp = F.log_softmax(_ref_layer(h, ei, w_mul, sub("conv2."), n, keep=wt), dim=1)
    ref_loss = F.nll_loss(ref_logp[train_mask], data.y[train_mask])
    ref_loss.backward()
    assert _max_rel(logp.detach(), ref_logp.detach()) < 1e-5                 # (observed 5.4e-7)
    assert abs(float(loss.detach()) - float(ref_loss.detach())) <= 1e-5 * abs(float(ref_loss.detach()))
    for k in names:
        g = dict(model.named_parameters())[k].grad
        if k.startswith("linear"):
            assert g is None, k                                   # unused modules get no gradient
            continue
        want = p[k].grad
        scale = float(want.abs().max())
        if k.endswith("w_mlp_out.2.bias"):                      # (zero up to rounding: see test_layer_backward_matches_autograd)
            scale = float(wt[0 if k.startswith("conv1") else 1].grad.abs().sum(0).max())
        # f32 against f32: observed at most 1.2e-5 of the largest entry (conv1's W1; against an f64 restatement 8.7e-7)
        err = float((g - want).abs().max())
        assert err <= 1e-4 * scale, (k, err, scale)
    assert all(q.grad is None and not q.requires_grad for q in model.modelGIN.parameters())


# ---- 6. compute_PI against the per-node reference loop --------------------------------------------------------------------------
def test_compute_pi_matches_per_node_reference():
    torch = _torch()
    from tlc_gnn_amd import synth
    from tlc_gnn_amd.data import Data
    from tlc_gnn_amd.Knowledge_Distillation import ConvCurv_GIN
    from tlc_gnn_amd.Knowledge_Distillation.Teacher_model import Teacher_Model
    from tlc_gnn_amd.Knowledge_Distillation import data_utils_NC as nc
    from oracle import lp_forward_ref as ref
    from oracle import oracle
    n, edges, kappa, _, _ = synth.shaped_graph("Cora", scale=0.05)
    edges = np.concatenate([edges, [[n, n + 1]]]).astype(np.int64)          # + a component of two nodes
    kappa = np.concatenate([kappa, [0.3]])
    n = n + 2
    ricci = sorted([[int(a), int(b), float(k)] for (a, b), k in zip(edges.tolist(), kappa.tolist())] +
                   [[int(b), int(a), float(k)] for (a, b), k in zip(edges.tolist(), kappa.tolist())])
    und = torch.from_numpy(edges.T.copy())
    loops = torch.arange(n)
    ei = torch.cat([und, und.flip(0), torch.stack([loops, loops])], dim=1)
    data = Data(x=torch.zeros(n, 4), edge_index=ei, y=torch.zeros(n, dtype=torch.long)).to("cuda")
    torch.manual_seed(3)
    teacher = Teacher_Model(hidden_dim=32, type='GAT', num_models=1, dropout=0, new_node_feat=True, use_edge_attn=True).eval()
    params = {"prelu": torch.tensor(0.1)}
    for name in ("conv1", "conv2", "conv3", "conv4"):
        c = getattr(teacher.DIM0_Model, name)
        params[name] = {"lin_l": c.lin_l.weight.detach().clone(), "att_l": c.att_l.detach().reshape(-1).clone(),
                        "lin_ij": c.lin_ij.weight.detach().clone(), "bias": c.bias.detach().clone()}
    params.update(lin5_w=teacher.lin5.weight.detach().clone(), lin5_b=teacher.lin5.bias.detach().clone(),
                  lin6_w=teacher.lin6.weight.detach().clone(), lin6_b=teacher.lin6.bias.detach().clone())
    for name in ("Cora", "photo"):
        net = ConvCurv_GIN.Net(data, name, 4, 3, g=edges, teacher=teacher, ricci_curv=ricci, chunk=40).cuda()
        PI = net.PI.cpu().double()
        hop = 2 if name == "Cora" else 1
        for u in range(n):
            fv, e = nc.compute_persistence_image(edges, u, filt='ricci', hop=hop, ricci_curv=ricci, mode='filtration')
            if fv is None:
                assert bool((PI[u] == 0).all()), u                  # a ball without an edge: a zero row
                continue
            f = torch.tensor(fv, dtype=torch.float32).view(-1, 1)
            k = f.shape[0]
            e2 = torch.cat([e.long(), torch.stack([torch.arange(k), torch.arange(k)])], dim=1)
            _, pd = ref.teacher_forward(f, e2, params)
            row = oracle.pi_raster(np.array([0, pd.shape[0]]), pd.double().numpy(), 5)[0]
            row = torch.from_numpy(row).float()
            if name == "photo":
                row = torch.nn.functional.normalize(row, dim=0)
            row = row.double()
            assert float((PI[u] - row).abs().max()) <= 1e-5 * max(1.0, float(row.abs().max())), (name, u)
        wm = net.w_mul.cpu().double()
        s, t = ei[0], ei[1]
        off = s != t
        assert torch.equal(wm[off], torch.cat([PI[s[off]], PI[t[off]]], dim=1))
        assert bool((wm[~off] == 0).all())
        if name == "photo":
            nz = PI.abs().sum(1) > 0
            assert torch.allclose(PI[nz].norm(dim=1), torch.ones(int(nz.sum()), dtype=PI.dtype), atol=1e-5)


def test_call_computes_curvature_when_not_given():
    """The reference's call(data, name, F, C) path with the trained teacher handed in and no curvature: loaddatas.compute_ricci_curvature
    of the data's edges, then compute_PI -- the same images as a Net given that curvature.  Node 0 has no edge: a zero row.  Without
    a teacher (and without w_mul) Net refuses instead of imaging with an untrained one."""
    torch = _torch()
    from tlc_gnn_amd import synth, loaddatas
    from tlc_gnn_amd.data import Data
    from tlc_gnn_amd.Knowledge_Distillation import ConvCurv_GIN
    from tlc_gnn_amd.Knowledge_Distillation.Teacher_model import Teacher_Model
    n, edges = synth.shaped_graph("Cora", scale=0.05)[:2]
    edges, n = edges + 1, n + 1                                                  # node 0: isolated
    und = torch.from_numpy(edges.T.copy())
    data = Data(x=torch.randn(n, 4), edge_index=torch.cat([und, und.flip(0)], dim=1), y=torch.zeros(n, dtype=torch.long))
    torch.manual_seed(3)
    teacher = Teacher_Model(hidden_dim=32, type='GAT', num_models=1, dropout=0, new_node_feat=True, use_edge_attn=True).eval()
    model, data = ConvCurv_GIN.call(data, "Cora", 4, 3, teacher=teacher)
    ei = data.edge_index
    assert ei.shape[1] == 2 * len(edges) + n and model.w_mul.shape == (ei.shape[1], 50)
    ricci = loaddatas.compute_ricci_curvature(Data(edge_index=ei[:, ei[0] != ei[1]].cpu(), y=torch.zeros(n, dtype=torch.long)))
    ref = ConvCurv_GIN.Net(data, "Cora", 4, 3, teacher=teacher, ricci_curv=ricci)
    assert torch.allclose(model.PI, ref.PI, rtol=1e-6, atol=1e-7) and torch.allclose(model.w_mul, ref.w_mul, rtol=1e-6, atol=1e-7)
    assert bool((model.PI[0] == 0).all()) and int((model.PI.abs().sum(1) > 0).sum()) > 0
    model.eval()
    with torch.no_grad():
        assert bool(torch.isfinite(model(data)).all())
    with pytest.raises(ValueError):
        ConvCurv_GIN.Net(data, "Cora", 4, 3)


# ---- 7. pipelines_GIN.fit on a planted partition -----------------------------------------------------------------------------------
def _planted(torch, n=1200, k=3, seed=0):
    from tlc_gnn_amd.data import Data
    rs = np.random.RandomState(seed)
    y = rs.randint(0, k, n)
    src, dst = [], []
    for _ in range(6 * n):
        u = rs.randint(n)
        same = rs.rand() < 0.9
        cand = np.flatnonzero((y == y[u]) if same else (y != y[u]))
        v = cand[rs.randint(len(cand))]
        if u != v:
            src += [u, v]
            dst += [v, u]
    x = rs.randn(n, 32).astype(np.float32) * 1.0
    x[np.arange(n), y] += 0.6
    ei = torch.tensor([src, dst], dtype=torch.long)
    data = Data(x=torch.from_numpy(x), edge_index=ei, y=torch.from_numpy(y).long())
    return data


# Recorded on one MI355X (30 epochs, seed 0): test accuracy 0.98, best validation accuracy 0.9875 (chance: 1/3).  The bound leaves room for other boxes' rounding.
FIT_MIN_TEST_ACC = 0.80


def test_fit_learns_planted_partition_deterministically():
    torch = _torch()
    from tlc_gnn_amd import pipelines_GIN
    from tlc_gnn_amd.Knowledge_Distillation import ConvCurv_GIN
    results, states = [], []
    for _ in range(2):
        data = _planted(torch)
        E = data.edge_index.shape[1] + data.num_nodes
        w_mul = torch.from_numpy(np.random.RandomState(1).uniform(0, 0.3, (E, 50)).astype(np.float32)).cuda()
        torch.manual_seed(0)
        torch.cuda.manual_seed_all(0)
        model, data = ConvCurv_GIN.call(data, "Synth", 32, 3, w_mul=w_mul)
        masks = pipelines_GIN.split_masks(data, pipelines_GIN.loader_of("Synth"), rng=random.Random(0))
        opt = pipelines_GIN.optimizer_for(model)
        res = pipelines_GIN.fit(model, data, opt, *masks, total_epochs=30, wait_total=100)
        results.append(res)
        states.append({k: v.detach().clone() for k, v in model.state_dict().items()})
    print("fit:", results[0][:2])
    assert results[0][0] >= FIT_MIN_TEST_ACC, results[0]
    assert results[0][:2] == results[1][:2]
    for k in states[0]:
        assert torch.equal(states[0][k], states[1][k]), k


# ---- 8. state_dict ------------------------------------------------------------------------------------------------------------------
REF_KEYS = [
    "conv1.lin.weight", "conv1.lin.bias", "conv1.w_mlp_out.0.weight", "conv1.w_mlp_out.1.weight", "conv1.w_mlp_out.2.weight",
    "conv1.w_mlp_out.2.bias", "conv2.lin.weight", "conv2.lin.bias", "conv2.w_mlp_out.0.weight", "conv2.w_mlp_out.1.weight",
    "conv2.w_mlp_out.2.weight", "conv2.w_mlp_out.2.bias", "linear.weight", "linear.bias", "linear_1.weight", "linear_1.bias",
]


def test_state_dict_keys_and_round_trip(tmp_path):
    torch = _torch()
    from tlc_gnn_amd.Knowledge_Distillation import ConvCurv_GIN
    from tlc_gnn_amd.Knowledge_Distillation.Teacher_model import Teacher_Model
    data = _planted(torch, n=200)
    E = data.edge_index.shape[1] + 200
    w_mul = torch.zeros(E, 50).cuda()
    model, data = ConvCurv_GIN.call(data, "Cora", 32, 3, w_mul=w_mul)
    teacher_keys = ["modelGIN." + k for k in Teacher_Model(hidden_dim=32, type='GAT', num_models=1, dropout=0).state_dict()]
    keys = list(model.state_dict().keys())
    assert keys == REF_KEYS + teacher_keys
    assert tuple(model.conv1.lin.weight.shape) == (256, 32) and tuple(model.conv1.w_mlp_out[0].weight.shape) == (256, 50)
    path = tmp_path / "nc.pt"
    torch.save(model.state_dict(), path)
    torch.manual_seed(99)
    other, _ = ConvCurv_GIN.call(data, "Cora", 32, 3, w_mul=w_mul)
    other.load_state_dict(torch.load(path))
    for k, v in model.state_dict().items():
        assert torch.equal(v, other.state_dict()[k]), k
    model.eval()
    other.eval()
    with torch.no_grad():
        assert torch.equal(model(data), other(data))

"""GPU: the TLCGNN link-prediction training step (pipelines.py:10-18) -- pipelines.train / pipelines.fit over the HIP backward
(lp_backward.hip: tlc_gemm_tn_f32, tlc_lp_decode_bwd_f32; tlc_gcn_norm_csr_t) against a pure-torch restatement with autograd."""
import os
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def _gcn_operator(edge_index, n, device, dtype):
    """gcn_norm of oracle/lp_forward_ref (add_remaining_self_loops, deg^-1/2 at both ends) -> (source, target, norm) on `device`."""
    from oracle import lp_forward_ref as ref
    ei, norm = ref.gcn_norm(edge_index.cpu(), n)
    return ei[0].to(device), ei[1].to(device), norm.to(device=device, dtype=dtype)


def _conv(h, w, b, op):
    """GCNConv: x @ W, add-aggregate at the target (index_add), + bias."""
    import torch
    src, dst, norm = op
    xw = h @ w
    out = torch.zeros((h.shape[0], xw.shape[1]), dtype=xw.dtype, device=xw.device)
    return out.index_add(0, dst, norm[:, None] * xw[src]) + b


def _decode_ref(emb, pairs, pi, w1, b1, w2, b2, renorm=True):
    """TLCGNN.py:48-61 with autograd: renorm (the in-place renorm_ of a non-leaf has this gradient), gather, Linear, LeakyReLU,
    Linear, |.|, clamp, Fermi-Dirac."""
    import torch
    import torch.nn.functional as F
    if renorm:
        emb = emb.renorm(2, 0, 1)
    a, b = emb[pairs[:, 0].long()], emb[pairs[:, 1].long()]
    h = F.leaky_relu(F.linear(torch.cat(((a - b).pow(2), pi.to(emb.dtype)), dim=1), w1, b1), 0.2)
    d = torch.clamp(torch.abs(F.linear(h, w2, b2)).reshape(-1), min=0, max=40)
    return 1.0 / (torch.exp((d - 2.0) / 1.0) + 1.0)


def _ref_step(model, data, pairs_all, pi_all, y_all, seed_torch, seed_np):
    """One training step of the restatement (f32, on the GPU, so that F.dropout draws the masks the model draws) from the model's
    CURRENT parameters -> (predictions, {name: grad})."""
    import torch
    import torch.nn.functional as F
    names = ["conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "linear_1.weight", "linear_1.bias", "linear.weight", "linear.bias"]
    sd = dict(model.named_parameters())
    p = {k: sd[k].detach().clone().requires_grad_(True) for k in names}
    x, dev = data.x, data.x.device
    op = _gcn_operator(data.edge_index, x.shape[0], dev, torch.float32)
    torch.manual_seed(seed_torch)
    np.random.seed(seed_np)
    h = F.dropout(x, p=0.5, training=True)
    h = _conv(h, p["conv1.weight"], p["conv1.bias"], op)
    h = F.dropout(F.relu(h), p=0.5, training=True)
    emb = F.relu(_conv(h, p["conv2.weight"], p["conv2.bias"], op))
    tp, tn = data.train_pos, data.train_neg
    index = np.random.randint(0, tn, tp)
    idx = np.concatenate([np.arange(tp), tp + index])
    pairs = torch.from_numpy(np.asarray(pairs_all)[idx]).to(dev)
    pi = torch.from_numpy(np.asarray(pi_all)[idx]).to(dev)
    y = torch.as_tensor(np.asarray(y_all)[idx]).to(dev).float()
    prob = _decode_ref(emb, pairs, pi, p["linear_1.weight"], p["linear_1.bias"], p["linear.weight"], p["linear.bias"])
    F.binary_cross_entropy(prob, y).backward()
    return prob.detach(), {k: p[k].grad for k in names}


def _close(got, want, rtol, atol_frac):
    import torch
    atol = atol_frac * float(want.abs().max()) if want.numel() else 0.0
    ok = torch.allclose(got.to(want.dtype), want, rtol=rtol, atol=atol)
    return ok, float((got.to(want.dtype) - want).abs().max()) if want.numel() else 0.0


def _holme_kim_data(torch, F_=48):
    """The 300-node graph of test_gpu_dropins.test_pipelines_test_and_train_forward (random pairs and labels)."""
    from tlc_gnn_amd import synth
    from tlc_gnn_amd.data import Data
    n, m = 300, 900
    edges = synth.holme_kim_edges(n, m, triad_p=0.5, seed=5)
    ei = torch.from_numpy(np.concatenate([edges, edges[:, ::-1]]).T.copy()).long()
    x = torch.from_numpy(synth.synthetic_features(n, F_, seed=5))
    rs = np.random.RandomState(2)
    E = 1200
    pairs = rs.randint(0, n, size=(E, 2))
    PI = rs.uniform(0, 0.3, size=(E, 25))
    y = torch.from_numpy((rs.rand(E) < 0.5).astype(np.int64))
    data = Data(x=x, edge_index=ei, y=torch.zeros(n), total_edges=pairs, total_edges_y=y,
                train_pos=300, train_neg=400, val_pos=100, val_neg=100, test_pos=150, test_neg=150)
    return data, pairs, PI, y.numpy(), F_


def _pubmed_data(torch):
    """The PubMed-shaped graph and the 37 676 training positives of bench.py's LP leg, as many sampled negatives, random image rows."""
    import bench
    from tlc_gnn_amd.data import Data
    wl = bench.build_workload(0)
    n, te = wl["n"], wl["train_edges"]
    ei = torch.from_numpy(np.concatenate([te, te[:, ::-1]]).T.copy()).long()
    pos, neg = wl["pi_pairs"].astype(np.int64), wl["neg"]
    pairs = np.concatenate([pos, neg])
    PI = np.random.RandomState(7).uniform(0, 0.3, size=(len(pairs), 25))
    y = np.concatenate([np.ones(len(pos), np.int64), np.zeros(len(neg), np.int64)])
    data = Data(x=torch.from_numpy(wl["x"]), edge_index=ei, y=torch.zeros(n), total_edges=pairs, total_edges_y=torch.from_numpy(y),
                train_pos=len(pos), train_neg=len(neg), val_pos=0, val_neg=0, test_pos=0, test_neg=0)
    return data, pairs, PI, y, wl["n_feat"]


def _model(torch, data, F_, PI, seed=3):
    from tlc_gnn_amd import pipelines
    from tlc_gnn_amd.baselines import TLCGNN
    pipelines.setup_seed(seed)
    model = TLCGNN.Net(data, F_, 2, PI=PI)
    model.apply(pipelines.weights_init)
    return model.cuda()


# ---- 1. decoder backward ------------------------------------------------------------------------------------------------------------
def test_decode_backward_matches_autograd_f64():
    torch = _torch()
    from tlc_gnn_amd import ops
    rs = np.random.RandomState(11)
    n, E = 40, 700
    emb = rs.normal(0, 0.6, size=(n, 16)).astype(np.float32)
    emb[0] = 0.0
    emb[0, 0] = 1.0                                                  # norm exactly 1
    emb[1] = 0.0
    emb[1, 3] = -1.0
    emb[2:12] *= 0.2                                                 # norms below 1
    emb[12:] *= 3.0                                                  # norms above 1
    pairs = rs.randint(0, n, size=(E, 2)).astype(np.int32)
    pairs[:50] = pairs[50:100]                                      # repeated pairs
    pairs[100:130, 1] = pairs[100:130, 0]                           # u == v
    pi = rs.uniform(0, 0.3, size=(E, 25)).astype(np.float32)
    pi[100:110] = 0.0                                                # u == v and no image: in = 0, d = b2 + W2 . b1 = 0 exactly
    pi[200:260] *= 200.0                                             # |d| > 40
    w1 = (rs.normal(0, 1.0, size=(25, 41))).astype(np.float32)
    b1 = (rs.randint(0, 5, size=25) * 0.25).astype(np.float32)      # dyadic, >= 0: LeakyReLU(b1) = b1
    w2 = (rs.randint(-4, 5, size=(1, 25)) * 0.25).astype(np.float32)
    b2 = np.array([-(w2[0].astype(np.float64) @ b1.astype(np.float64))], dtype=np.float32)
    gprob = rs.normal(0, 1.0, size=E).astype(np.float32)
    dev = "cuda"
    t = {k: torch.from_numpy(v).to(dev) for k, v in dict(emb=emb, pairs=pairs, pi=pi, w1=w1, b1=b1, w2=w2, b2=b2, g=gprob).items()}
    post = ops.renorm_rows_(t["emb"].clone())
    got = ops.lp_decode_bwd(t["pairs"], t["emb"], post, t["pi"], t["w1"], t["b1"], t["w2"], t["b2"], t["g"])
    again = ops.lp_decode_bwd(t["pairs"], t["emb"], post, t["pi"], t["w1"], t["b1"], t["w2"], t["b2"], t["g"])
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    # the restatement, f64
    r = {k: v.double().requires_grad_(True) for k, v in t.items() if k not in ("pairs", "g")}
    # (forward values: the kernel's fp32 renormed rows -- the rounding of the forward is not under test; the gradient flows through
    # torch's renorm of the f64 rows, which is)
    e = r["emb"].renorm(2, 0, 1)
    e = e + (post.double() - e).detach()
    prob = _decode_ref(e, t["pairs"], r["pi"], r["w1"], r["b1"], r["w2"], r["b2"], renorm=False)
    with torch.no_grad():                                            # the cases the data is built to hold
        e = r["emb"].renorm(2, 0, 1)
        a, b = e[t["pairs"][:, 0].long()], e[t["pairs"][:, 1].long()]
        h = torch.cat(((a - b).pow(2), r["pi"]), 1) @ r["w1"].t() + r["b1"]
        d = torch.nn.functional.leaky_relu(h, 0.2) @ r["w2"].t() + r["b2"]
        assert bool((h < 0).any()) and bool((h > 0).any())
        assert bool((d.abs() > 40).any()) and int((d == 0).sum()) >= 10
    prob.backward(t["g"].double())
    names = ["emb", "w1", "b1", "w2", "b2"]
    for name, g in zip(names, got):
        want = r[name].grad
        ok, err = _close(g.double(), want, 1e-4, 2e-5)
        assert g.shape == want.shape and ok, (name, err, float(want.abs().max()))
    # an empty batch: zero weight gradients, zero d emb
    z = ops.lp_decode_bwd(t["pairs"][:0], t["emb"], post, t["pi"][:0], t["w1"], t["b1"], t["w2"], t["b2"], t["g"][:0])
    assert all(float(v.abs().max()) == 0.0 for v in z)


# ---- 2. A^T B and A^T G ---------------------------------------------------------------------------------------------------------------
def test_gemm_tn_odd_shapes_and_deterministic():
    torch = _torch()
    from tlc_gnn_amd import ops
    g = torch.Generator(device="cuda").manual_seed(5)
    for K in (0, 1, 65, 1000, 19717):
        for M in (1, 16, 100, 500):
            for N in (1, 16, 100, 500):
                a = torch.randn((K, M), device="cuda", generator=g)
                b = torch.randn((K, N), device="cuda", generator=g)
                c = ops.gemm_tn(a, b)
                want = a.double().t() @ b.double()
                ok, err = _close(c.double(), want, 1e-4, 1e-5)
                assert c.shape == (M, N) and ok, (K, M, N, err)
                assert torch.equal(c, ops.gemm_tn(a, b)), (K, M, N)
                if M == 1:
                    s = ops.colsum(b)
                    ok, err = _close(s.double(), b.double().sum(0), 1e-4, 1e-5)
                    assert ok and torch.equal(s, ops.colsum(b)), (K, N, err)
                if K == 0:
                    assert float(c.abs().max()) == 0.0


def test_transposed_operator_non_symmetric():
    torch = _torch()
    from tlc_gnn_amd import ops
    rs = np.random.RandomState(4)
    n = 157
    ei = rs.randint(0, n, size=(2, 900))
    ei[:, :20] = ei[:, 20:40]                                       # duplicate edges
    ei[1, 40:50] = ei[0, 40:50]                                     # self loops (dropped, one per node re-added)
    ei = torch.from_numpy(ei).long().cuda()
    rowptr, col, val = ops.gcn_norm_csr(ei, n)
    rowptr_t, col_t, val_t = ops.gcn_norm_csr_t(ei, n, rowptr)
    src, dst, norm = _gcn_operator(ei, n, "cuda", torch.float64)
    A = torch.zeros((n, n), dtype=torch.float64, device="cuda").index_put_((dst, src), norm, accumulate=True)
    assert not torch.equal(A, A.t())
    # the same entries as the forward's operator, transposed, with bit-equal values
    fwd = sorted(zip(np.repeat(np.arange(n), np.diff(rowptr.cpu().numpy())).tolist(), col.cpu().numpy().tolist(), val.cpu().numpy().tolist()))
    bwd = sorted(zip(col_t.cpu().numpy().tolist(), np.repeat(np.arange(n), np.diff(rowptr_t.cpu().numpy())).tolist(), val_t.cpu().numpy().tolist()))
    assert fwd == bwd
    for k in (1, 16, 100):
        G = torch.randn((n, k), device="cuda")
        y = ops.spmm(rowptr_t, col_t, val_t, G)
        ok, err = _close(y.double(), A.t() @ G.double(), 1e-4, 1e-6)
        assert ok, (k, err)
        assert torch.equal(y, ops.spmm(rowptr_t, col_t, val_t, G))


# ---- 3, 4. one step of the whole model ------------------------------------------------------------------------------------------------
def _step_against_restatement(torch, data, pairs, PI, y, F_, pi_table=None):
    from tlc_gnn_amd import pipelines
    model = _model(torch, data, F_, PI if pi_table is None else pi_table)
    data = data.to("cuda")
    opt = torch.optim.SGD(model.parameters(), lr=0.0)               # (lr 0: the parameters stay, the gradients are kept)
    pipelines.setup_seed(17)
    x_fwd, _, _ = pipelines.train_forward(model, data)
    pipelines.setup_seed(17)
    x = pipelines.train(model, data, opt)
    assert torch.equal(x, x_fwd)                                     # the training forward is the product forward
    grads = {k: p.grad.clone() for k, p in model.named_parameters()}
    pipelines.setup_seed(17)
    pipelines.train(model, data, opt)
    for k, p in model.named_parameters():                            # deterministic: bit-equal gradients
        assert torch.equal(p.grad, grads[k]), k
    prob_ref, gref = _ref_step(model, data, pairs, PI, y, 17, 17)
    assert torch.allclose(x, prob_ref, rtol=1e-4, atol=1e-5)
    for k, want in gref.items():
        ok, err = _close(grads[k], want, 1e-3, 1e-4)
        assert ok, (k, err, float(want.abs().max()))
    return model, data, grads


def test_train_step_holme_kim_matches_restatement():
    torch = _torch()
    data, pairs, PI, y, F_ = _holme_kim_data(torch)
    model, data, _ = _step_against_restatement(torch, data, pairs, PI, y, F_)
    # the public encode / decode keep refusing to record autograd, and now point at the training step
    model.train()
    with pytest.raises(RuntimeError, match="forward only.*pipelines.train"):
        model.encode(data)


def test_train_step_pubmed_shape_matches_restatement():
    torch = _torch()
    data, pairs, PI, y, F_ = _pubmed_data(torch)
    _step_against_restatement(torch, data, pairs, PI, y, F_, pi_table=torch.from_numpy(PI).cuda())


# ---- 5. several steps; fit -------------------------------------------------------------------------------------------------------------
def test_five_sgd_steps_match_restatement():
    torch = _torch()
    from tlc_gnn_amd import pipelines
    data, pairs, PI, y, F_ = _holme_kim_data(torch)
    model = _model(torch, data, F_, PI)
    data = data.to("cuda")
    names = [k for k, _ in model.named_parameters()]
    ref_params = {k: p.detach().clone() for k, p in model.named_parameters()}
    opt = torch.optim.SGD(model.parameters(), lr=0.5)
    for step in range(5):
        pipelines.setup_seed(100 + step)
        pipelines.train(model, data, opt)
        # the restatement from its own parameters, stepped by hand like SGD
        shadow = _Shadow(ref_params)
        _, g = _ref_step(shadow, data, pairs, PI, y, 100 + step, 100 + step)
        ref_params = {k: ref_params[k] - 0.5 * g[k] for k in names}
    moved = 0.0
    for k, p in model.named_parameters():
        assert torch.allclose(p.detach(), ref_params[k], rtol=1e-4, atol=1e-5), (k, float((p.detach() - ref_params[k]).abs().max()))
        moved = max(moved, float((p.detach() - dict(_model(torch, data, F_, PI).named_parameters())[k].detach()).abs().max()))
    assert moved > 1e-3


class _Shadow:
    def __init__(self, params):
        self._p = params

    def named_parameters(self):
        return list(self._p.items())


def _clustered_split(torch):
    from tlc_gnn_amd import synth
    from tlc_gnn_amd.data import Data
    n, m, F_ = 260, 700, 40
    edges = synth.holme_kim_edges(n, m, triad_p=0.5, seed=21)
    ei = torch.from_numpy(np.concatenate([edges, edges[:, ::-1]]).T.copy()).long()
    data = Data(x=torch.from_numpy(synth.synthetic_features(n, F_, seed=2)), edge_index=ei, y=torch.zeros(n, dtype=torch.long))
    data.ricci_list = synth.synthetic_curvature(edges, seed=21)
    return data, F_


def _call(torch, data, F_, streamed=None):
    from tlc_gnn_amd.baselines import TLCGNN
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            torch.manual_seed(3)
            np.random.seed(3)
            return TLCGNN.call(data, "Cora", F_, 2, 0, streamed=streamed)
        finally:
            os.chdir(cwd)


def test_fit_with_adam_learns_on_a_clustered_split():
    torch = _torch()
    from tlc_gnn_amd import pipelines
    data, F_ = _clustered_split(torch)
    model, data = _call(torch, data, F_)
    pipelines.setup_seed(5)
    model.apply(pipelines.weights_init)
    untrained = pipelines.test(model, data)
    pipelines.setup_seed(6)
    _, _, loss0 = pipelines.train_forward(model, data)
    opt = torch.optim.Adam(model.parameters(), lr=0.005, weight_decay=0)
    pipelines.setup_seed(7)
    test_acc, test_roc, best_val_acc, best_val_roc, best_val_loss = pipelines.fit(model, data, opt, total_epochs=50, wait_total=200)
    pipelines.setup_seed(6)
    _, _, loss1 = pipelines.train_forward(model, data)
    assert float(loss1) < float(loss0), (float(loss0), float(loss1))
    assert best_val_roc > untrained[1], (untrained, best_val_roc)
    assert 0.0 <= test_roc <= 1.0 and 0.0 <= test_acc <= 1.0 and np.isfinite(float(best_val_loss))


# ---- 6. streamed tables --------------------------------------------------------------------------------------------------------------
def test_streamed_tables_give_the_dense_gradients():
    torch = _torch()
    from tlc_gnn_amd import pipelines
    grads = {}
    state = None
    for streamed in (False, True):
        data, F_ = _clustered_split(torch)
        model, data = _call(torch, data, F_, streamed=streamed)
        if state is None:
            pipelines.setup_seed(5)
            model.apply(pipelines.weights_init)
            state = {k: v.clone() for k, v in model.state_dict().items()}
        else:
            model.load_state_dict(state)
        opt = torch.optim.SGD(model.parameters(), lr=0.1)
        pipelines.setup_seed(9)
        x = pipelines.train(model, data, opt)
        grads[streamed] = ({k: p.grad.clone() for k, p in model.named_parameters()}, x)
    assert torch.equal(grads[False][1], grads[True][1])
    for k, g in grads[False][0].items():
        assert torch.equal(g, grads[True][0][k]), k

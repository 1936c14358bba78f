"""torch restatement of the teacher's message-passing baselines (Knowledge_Distillation/Teacher_model.py:148-175,202-208,213-241 with
torch_geometric 1.6.1's GINConv / GCNConv / SAGEConv), straight from the formulas: index_add_ on the edge list as given, gcn_norm written
out from PD_conv.py:35-70.  TEST INFRASTRUCTURE ONLY; runs in the dtype of its inputs (float64 for the reference values, float32 on the
CPU to measure what float32 itself costs).  Shared by tests/test_cpu_gnn_baselines_host.py and tests/test_gpu_gnn_baselines.py.

PARITY UNPINNED against torch_geometric (not installed): the three layers are restated from its 1.6.1 sources as SURVEY.md 8(c) records
them, like oracle/lp_forward_ref.py's GCNConv.
"""
import numpy as np
import torch
import torch.nn.functional as F

KINDS = ("GIN", "GCN", "SAGE")
ORDER = ("conv1", "conv2", "conv4", "conv3")          # Base_Model.forward's order (:220-241)


def _act(z, act, slope):
    if act == "relu":
        return F.relu(z)
    if act == "prelu":
        return F.prelu(z, torch.tensor(slope, dtype=z.dtype))
    return z


def scatter_add(vals, index, n):
    return torch.zeros((n,) + vals.shape[1:], dtype=vals.dtype).index_add_(0, index, vals)


def gin_layer(x, ei, w, b, act=None, slope=0.0):
    """GINConv(nn = Linear [+ ReLU], eps = 0): nn((1 + eps) x_i + sum_{j -> i} x_j), the edge list as given."""
    agg = x + scatter_add(x[ei[0]], ei[1], x.shape[0])
    return _act(F.linear(agg, w, b), act, slope)


def gcn_norm(ei, n, dtype):
    """PD_conv.py:35-70, edge_index branch with unit weights: add_remaining_self_loops (every loop of the list dropped, one loop per node
    appended, its weight an existing loop's = 1), degrees summed at the target, D^-1/2 A D^-1/2."""
    mask = ei[0] != ei[1]
    loop = torch.arange(n, dtype=ei.dtype)
    ei = torch.cat([ei[:, mask], torch.stack([loop, loop])], dim=1)
    w = torch.ones(ei.shape[1], dtype=dtype)
    deg = scatter_add(w, ei[1], n)
    dis = deg.pow(-0.5)
    dis = dis.masked_fill(dis == float("inf"), 0.0)
    return ei, dis[ei[0]] * w * dis[ei[1]]


def gcn_layer(x, ei, weight, bias, act=None, slope=0.0):
    """GCNConv (PD_conv.py:179-188): x @ weight [in, out] first, propagate(add) at the target, + bias."""
    ei2, norm = gcn_norm(ei, x.shape[0], x.dtype)
    xw = x @ weight
    return _act(scatter_add(norm[:, None] * xw[ei2[0]], ei2[1], x.shape[0]) + bias, act, slope)


def sage_layer(x, ei, wl, bl, wr, act=None, slope=0.0):
    """SAGEConv of PyG 1.6.1: lin_l(mean_{j -> i} x_j) + lin_r(x_i); self loops untouched, an empty row's mean is 0."""
    n = x.shape[0]
    deg = scatter_add(torch.ones(ei.shape[1], dtype=x.dtype), ei[1], n)
    mean = scatter_add(x[ei[0]], ei[1], n) / deg.clamp(min=1)[:, None]
    return _act(F.linear(mean, wl, bl) + F.linear(x, wr), act, slope)


def layer(kind, x, ei, p, act=None, slope=0.0):
    """p: GIN {w, b}, GCN {weight [in, out], bias}, SAGE {wl, bl, wr}."""
    if kind == "GIN":
        return gin_layer(x, ei, p["w"], p["b"], act, slope)
    if kind == "GCN":
        return gcn_layer(x, ei, p["weight"], p["bias"], act, slope)
    return sage_layer(x, ei, p["wl"], p["bl"], p["wr"], act, slope)


def stack(kind, x, ei, params, masks=None):
    """Base_Model.forward :213-241: conv1 -> conv2 -> conv4 -> conv3; the GIN branch's layers carry their own ReLU (none on conv3) and
    no PReLU; the other types F.prelu(0.1) behind the first three.  masks: the four F.dropout masks in call order (in front of every
    layer), already scaled; None = eval mode."""
    for k, name in enumerate(ORDER):
        if masks is not None:
            x = x * masks[k]
        last = name == "conv3"
        act = (None if last else "relu") if kind == "GIN" else (None if last else "prelu")
        x = layer(kind, x, ei, params[name], act, 0.1)
    return x


def teacher_forward(kind, f, ei, params, masks=None):
    """Teacher_Model.forward :46-59 with a baseline: the stack on the edge_index as given (self loops LAST, the callers' convention,
    train_Teacher_Model.py:43-44), then the edge head on the edges without those loops.  masks: five, the last between lin5 and lin6."""
    n = f.shape[0]
    x = stack(kind, f, ei, params, None if masks is None else masks[:4])
    e = ei[:, :ei.shape[1] - n]
    h = F.prelu(F.linear(torch.cat((x[e[0]], x[e[1]]), dim=1), params["lin5_w"], params["lin5_b"]), torch.tensor(0.1, dtype=x.dtype))
    if masks is not None:
        h = h * masks[4]
    return x, F.linear(h, params["lin6_w"], params["lin6_b"])


# ---- parameters ---------------------------------------------------------------------------------------------------------------------
def random_layer_params(kind, c_in, c_out, gen, dtype=torch.float64):
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64).to(dtype)
    sc = 0.7 / np.sqrt(c_in)
    if kind == "GIN":
        return {"w": r(c_out, c_in) * sc, "b": r(c_out) * 0.2}
    if kind == "GCN":
        return {"weight": r(c_in, c_out) * sc, "bias": r(c_out) * 0.2}
    return {"wl": r(c_out, c_in) * sc, "bl": r(c_out) * 0.2, "wr": r(c_out, c_in) * sc}


def device_operands(kind, p):
    """(Wa, Ws, bias) of include/tlcgnn.h's layer form from a parameter dict (float32 CPU tensors)."""
    f = lambda t: t.detach().to(torch.float32)
    if kind == "GIN":
        return f(p["w"]), None, f(p["b"])
    if kind == "GCN":
        return f(p["weight"]).t().contiguous(), None, f(p["bias"])
    return f(p["wl"]), f(p["wr"]), f(p["bl"])


STATE_KEYS = {           # the parameter (and buffer) names of one conv, with their shapes for in -> out
    "GIN": lambda i, o: {"nn.0.weight": (o, i), "nn.0.bias": (o,), "eps": (1,)},
    "GCN": lambda i, o: {"weight": (i, o), "bias": (o,)},
    "SAGE": lambda i, o: {"lin_l.weight": (o, i), "lin_l.bias": (o,), "lin_r.weight": (o, i)},
}


def teacher_params(model, kind, dtype=torch.float64):
    """(params for `teacher_forward`, {state-dict name: leaf}) from a Teacher_Model of that type: detached copies that require grad."""
    leaf = lambda t: t.detach().cpu().to(dtype).clone().requires_grad_()
    names = {"GIN": {"w": "nn.0.weight", "b": "nn.0.bias"}, "GCN": {"weight": "weight", "bias": "bias"},
             "SAGE": {"wl": "lin_l.weight", "bl": "lin_l.bias", "wr": "lin_r.weight"}}[kind]
    sd = dict(model.named_parameters())
    params, leaves = {}, {}
    for conv in ORDER:
        params[conv] = {}
        for k, nm in names.items():
            full = "DIM0_Model.%s.%s" % (conv, nm)
            params[conv][k] = leaves[full] = leaf(sd[full])
    for k, full in (("lin5_w", "lin5.weight"), ("lin5_b", "lin5.bias"), ("lin6_w", "lin6.weight"), ("lin6_b", "lin6.bias")):
        params[k] = leaves[full] = leaf(sd[full])
    return params, leaves


# ---- graphs ---------------------------------------------------------------------------------------------------------------------------
def random_edges(rs, n, m, loops="some", repeats=True):
    """int64 [2, m'] directed edges on n nodes.  loops: 'some' (as drawn), 'none', 'double' (none drawn, then two loops on node 0),
    'all' (one on every node, appended LAST).  repeats=False: distinct pairs."""
    s, t = rs.randint(0, max(n, 1), size=m), rs.randint(0, max(n, 1), size=m)
    e = np.stack([s, t]).astype(np.int64)
    if loops != "some":
        e = e[:, e[0] != e[1]]
    if not repeats and e.shape[1]:
        e = e[:, np.sort(np.unique(e, axis=1, return_index=True)[1])]
    if loops == "double":
        e = np.concatenate([e, np.zeros((2, 2), dtype=np.int64)], axis=1)
    if loops == "all":
        e = np.concatenate([e, np.stack([np.arange(n), np.arange(n)])], axis=1)
    return torch.tensor(e, dtype=torch.int64).reshape(2, -1)


def connected_graph(rs, n, extra):
    """One orientation per edge (the teacher's own convention): the path 0 - 1 - ... - n-1 (so that no position inside the graph is free of
    crossing edges) and `extra` random chords, no loops, no repeats."""
    pairs = {(i, i + 1) for i in range(n - 1)}
    for _ in range(extra):
        a, b = int(rs.randint(0, n)), int(rs.randint(0, n))
        if a != b and (a, b) not in pairs and (b, a) not in pairs:
            pairs.add((a, b))
    e = np.array(sorted(pairs), dtype=np.int64).reshape(-1, 2).T
    flip = rs.rand(e.shape[1]) < 0.5
    e[:, flip] = e[::-1][:, flip]
    return torch.tensor(e, dtype=torch.int64).reshape(2, -1)


def batch_of(rs, sizes, extra=1.0):
    """A block-diagonal batch of connected graphs of the given node counts in the teacher's convention: the real edges graph by graph,
    then one self loop per node LAST.  -> (graphs [(n, e)], edge_index int64 [2, m + N], node_ptr, edge_ptr int64 numpy)."""
    graphs = [(int(n), connected_graph(rs, int(n), int(extra * n))) for n in sizes]
    gptr = np.concatenate([[0], np.cumsum([g[0] for g in graphs])]).astype(np.int64)
    eptr = np.concatenate([[0], np.cumsum([g[1].shape[1] for g in graphs])]).astype(np.int64)
    N = int(gptr[-1])
    ei = torch.cat([g[1] + int(gptr[b]) for b, g in enumerate(graphs)], dim=1)
    loops = torch.arange(N, dtype=torch.int64)
    return graphs, torch.cat([ei, torch.stack([loops, loops])], dim=1), gptr, eptr


def with_loops(n, e):
    lp = torch.arange(n, dtype=torch.int64)
    return torch.cat([e, torch.stack([lp, lp])], dim=1)


def rel(a, b):
    """max-abs difference over max-abs reference (tests/test_gpu_train.py:128-130)."""
    a = a.detach().cpu().double().reshape(-1)
    b = b.detach().cpu().double().reshape(-1)
    if a.numel() == 0:
        return 0.0
    return float((a - b).abs().max() / max(1e-12, float(b.abs().max())))

"""torch restatement of the PDGNN layer family (Knowledge_Distillation/gat_conv.py:113-216 with its new_node_feat / use_edge_attn switches,
PD_conv.py:179-219), straight from the formulas:

    x_l = X Wl^T                        alpha = x_l . att
    h_e = leaky_relu(Wij [x_l[i] || x_l[j]], 0.2)   (node_feat)   or   x_l[j]
    a_e = softmax over the in-edges of i of leaky_relu(alpha[j] + alpha[i], 0.2)   (edge_attn)   or   1
    m_e = a_e * h_e
    out_i = [ sum_e m_e || (min_e m_e + max_e m_e) ] + bias      ('sum_minmax')
    out_i = [ sum_e m_e ||  min_e m_e              ] + bias      ('sum_min')

gathered through edge_index after remove_self_loops + add_self_loops, scatter_reduce with amin / amax and include_self=False.  TEST
INFRASTRUCTURE ONLY; runs in the dtype of its inputs (float64 for the reference values).  Shared by tests/test_cpu_msg_layers_host.py and
tests/test_gpu_msg_layers.py.

Ties in min / max: a repeated edge (j -> i) gives two equal messages.  Torch's amin / amax backward splits the gradient evenly over the
tying entries; the kernel gives it to the first.  The copies share BOTH ends, so d m_e flows to the same x_l[i], x_l[j], alpha and weights
either way and every TENSOR gradient is equal -- the tests rely on that.  Everything else is generic random values, so no other tie occurs.
"""
import numpy as np
import torch
import torch.nn.functional as F

from gnn_baseline_cases import rel, random_edges, connected_graph, batch_of, with_loops   # noqa: F401  (shared helpers)

MODES = ((True, True), (True, False), (False, True), (False, False))      # (node_feat, edge_attn)
AGGS = ("sum_minmax", "sum_min")
ORDER = ("conv1", "conv2", "conv4", "conv3")                              # Base_Model.forward's order


def looped(ei, n):
    """remove_self_loops + add_self_loops (gat_conv.py:154-155): the kept edges in order, then one loop per node."""
    keep = ei[0] != ei[1]
    lp = torch.arange(n, dtype=ei.dtype)
    return torch.cat([ei[:, keep], torch.stack([lp, lp])], dim=1)


def softmax_by_target(logit, tgt, n):
    """PyG's softmax: minus the row maximum, exp, over (the row sum + 1e-16)."""
    mx = torch.full((n,), -float("inf"), dtype=logit.dtype).scatter_reduce(0, tgt, logit, "amax", include_self=False)
    ex = (logit - mx[tgt]).exp()
    den = torch.zeros(n, dtype=logit.dtype).index_add_(0, tgt, ex)
    return ex / (den[tgt] + 1e-16)


def layer(x, ei, p, node_feat, edge_attn, agg="sum_minmax", prelu_slope=-1.0, edges_as_given=False):
    """p: {wl [C, c_in], att [C], wij [C, 2C], bias [2C]} (att / wij unused when their switch is off).  edges_as_given: `ei` already is
    the final entry list (the C ABI takes any CSR, e.g. one with an empty row)."""
    n = x.shape[0]
    e = ei if edges_as_given else looped(ei, n)
    src, tgt = e[0], e[1]
    xl = x @ p["wl"].t()
    C = xl.shape[1]
    h = xl[src]
    if node_feat:
        h = F.leaky_relu(torch.cat((xl[tgt], xl[src]), dim=1) @ p["wij"].t(), 0.2)
    m = h
    if edge_attn:
        alpha = xl @ p["att"].reshape(-1)
        m = h * softmax_by_target(F.leaky_relu(alpha[src] + alpha[tgt], 0.2), tgt, n)[:, None]
    idx = tgt[:, None].expand(-1, C)
    zero = torch.zeros((n, C), dtype=x.dtype)
    s = zero.index_add(0, tgt, m)
    mn = zero.scatter_reduce(0, idx, m, "amin", include_self=False)            # (a row without entries keeps the 0)
    second = mn if agg == "sum_min" else mn + zero.scatter_reduce(0, idx, m, "amax", include_self=False)
    out = torch.cat((s, second), dim=1) + p["bias"]
    if prelu_slope >= 0:
        out = F.prelu(out, torch.tensor(prelu_slope, dtype=out.dtype))
    return out


def dense_layer(x, ei, p, node_feat, edge_attn, agg="sum_minmax"):
    """The same layer from dense [n, n, C] arrays with a multiplicity matrix: for tiny graphs only (the CPU test's second opinion)."""
    n = x.shape[0]
    e = looped(ei, n)
    mult = torch.zeros((n, n), dtype=x.dtype)                                    # mult[i, j] = number of entries j -> i
    for s, t in zip(e[0].tolist(), e[1].tolist()):
        mult[t, s] += 1
    xl = x @ p["wl"].t()
    C = xl.shape[1]
    H = xl[None, :, :].expand(n, n, C)
    if node_feat:
        H = F.leaky_relu((xl @ p["wij"][:, :C].t())[:, None, :] + (xl @ p["wij"][:, C:].t())[None, :, :], 0.2)      # H[i, j] = P_i + Q_j
    M = H
    if edge_attn:
        alpha = xl @ p["att"].reshape(-1)
        L = F.leaky_relu(alpha[None, :] + alpha[:, None], 0.2)                   # L[i, j]
        Lm = torch.where(mult > 0, L, torch.full_like(L, -float("inf")))
        ex = torch.exp(Lm - Lm.max(dim=1, keepdim=True).values) * mult
        A = ex / (ex.sum(dim=1, keepdim=True) + 1e-16) / mult.clamp(min=1)       # per entry
        M = H * A[:, :, None]
    present = (mult > 0)[:, :, None]
    s = (M * mult[:, :, None]).sum(dim=1)
    mn = torch.where(present, M, torch.full_like(M, float("inf"))).min(dim=1).values
    mx = torch.where(present, M, torch.full_like(M, -float("inf"))).max(dim=1).values
    return torch.cat((s, mn if agg == "sum_min" else mn + mx), dim=1) + p["bias"]


def random_layer_params(c_in, c_out, gen, dtype=torch.float64, att_scale=1.0):
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64).to(dtype)
    return {"wl": r(c_out, c_in) * (0.7 / np.sqrt(c_in)), "att": r(c_out) * (att_scale / np.sqrt(c_out)),
            "wij": r(c_out, 2 * c_out) * (0.7 / np.sqrt(2 * c_out)), "bias": r(2 * c_out) * 0.2}


# ---- stacks and the teacher ---------------------------------------------------------------------------------------------------------------
def stack(x, ei, params, node_feat, edge_attn, agg="sum_minmax"):
    """Base_Model.forward :213-229 (eval mode): conv1 -> conv2 -> conv4 -> conv3, F.prelu(0.1) behind the first three."""
    for name in ORDER:
        x = layer(x, ei, params[name], node_feat, edge_attn, agg, -1.0 if name == "conv3" else 0.1)
    return x


def teacher_forward(f, ei, params, node_feat, edge_attn):
    """Teacher_Model.forward :46-59 with type='GAT': the stack on the edge_index as given (self loops LAST), then the edge head on the edges
    without those loops."""
    n = f.shape[0]
    x = stack(f, ei, params, node_feat, edge_attn)
    e = ei[:, :ei.shape[1] - n]
    h = F.prelu(F.linear(torch.cat((x[e[0]], x[e[1]]), dim=1), params["lin5_w"], params["lin5_b"]), torch.tensor(0.1, dtype=x.dtype))
    return x, F.linear(h, params["lin6_w"], params["lin6_b"])


def gat_state_keys(c_in_total, c_out, node_feat):
    """The reference's parameter names and shapes of one GATConv (gat_conv.py:78-100; lin_r IS lin_l, so state_dict lists it too)."""
    keys = {"lin_l.weight": (c_out, c_in_total), "lin_r.weight": (c_out, c_in_total), "att_l": (1, 1, c_out), "att_r": (1, 1, c_out),
            "bias": (2 * c_out,)}
    if node_feat:
        keys["lin_ij.weight"] = (c_out, 2 * c_out)
    return keys


def pd_state_keys(c_in_total, c_out, node_feat):
    """PD_conv.py:129-142."""
    keys = {"weight": (c_in_total, c_out), "bias": (2 * c_out,)}
    if node_feat:
        keys["lin_ij.weight"] = (c_out, 2 * c_out)
    return keys


def teacher_params(model, node_feat, edge_attn, dtype=torch.float64):
    """(params for `teacher_forward`, {named_parameters name: leaf}) of a Teacher_Model(type='GAT'): detached copies that require grad.
    Only what the forward reads: no att_l without edge_attn, no lin_ij without node_feat."""
    leaf = lambda t: t.detach().cpu().to(dtype).clone().requires_grad_()
    sd = dict(model.named_parameters())
    params, leaves = {}, {}
    for conv in ORDER:
        names = {"wl": "lin_l.weight", "bias": "bias"}
        if edge_attn:
            names["att"] = "att_l"
        if node_feat:
            names["wij"] = "lin_ij.weight"
        params[conv] = {}
        for k, nm in names.items():
            full = "DIM0_Model.%s.%s" % (conv, nm)
            params[conv][k] = leaves[full] = leaf(sd[full])
    for k, full in (("lin5_w", "lin5.weight"), ("lin5_b", "lin5.bias"), ("lin6_w", "lin6.weight"), ("lin6_b", "lin6.bias")):
        params[k] = leaves[full] = leaf(sd[full])
    return params, leaves


# ---- special edge lists ---------------------------------------------------------------------------------------------------------------------
def hub_edges(n, hub, k):
    """k distinct nodes -> hub and hub -> the same k nodes (a row of k + 1 entries and a node with k + 1 out-entries), k <= n - 1."""
    others = torch.tensor([v for v in range(n) if v != hub][:k], dtype=torch.int64)
    h = torch.full_like(others, hub)
    return torch.cat([torch.stack([others, h]), torch.stack([h, others])], dim=1)


def rows_of(n, counts):
    """Node i gets counts[i] - 1 distinct in-neighbours (its row then has counts[i] entries with the loop), i < len(counts)."""
    src, tgt = [], []
    for i, c in enumerate(counts):
        nb = [v for v in range(n) if v != i][:c - 1]
        src += nb
        tgt += [i] * len(nb)
    return torch.tensor([src, tgt], dtype=torch.int64).reshape(2, -1)

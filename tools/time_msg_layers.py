"""What the PDGNN layer family costs (csrc/msg_layers.hip) -> profiles/msg_layers_timing.json.

One MI355X, device events around one call, the median of five windows, every route in the same run.  Parts, the JSON rewritten after each:
  hiv      the 41 127 HIV-shaped molecule graphs of synth.hiv_shaped_molecules() as one block-diagonal batch (both orientations, the
           self loops last), one hidden layer (64 -> 32, PReLU 0.1 fused): forward and backward (tlc_msg_layer_fwd / _bwd) of GATConv's three
           ablations (sum || min + max) and of PDConv with and without new_node_feat (sum || min); the FULL configuration through the new
           family against tlc_gat_layer_fwd / tlc_gat_layer_bwd (the atomic backward) -- the ratio that decides whether the default 'GAT'
           backward moves over; and the same layers written in torch ops (index_add_ / scatter_reduce, torch's autograd for the backward);
  amazon   the 4 096 hop-1 vicinities of the Photo-shaped graph, stacked (data_utils_LP.stacked): the same routes;
  train    one training step (forward, kernel='wasserstein' p = 2, backward) of Teacher_Model(type='GAT') on the first 4 096 HIV-shaped
           graphs, dropout 0, for the four flag combinations (the full one runs tlc_gat_layer_fwd / _bwd as before).

    python tools/time_msg_layers.py [--parts hiv,amazon,train] [--n-graphs 41127] [--out profiles/msg_layers_timing.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from time_gnn_baselines import windows, note, rel, hiv_batch, amazon_batch   # noqa: E402  (the batches and the timer of the baselines' tool)

C_IN, C_OUT, SLOPE = 64, 32, 0.1
CONFIGS = (("gat_no_node_feat", False, True, "sum_minmax"), ("gat_no_edge_attn", True, False, "sum_minmax"), ("gat_neither", False, False, "sum_minmax"),
           ("pdconv", True, False, "sum_min"), ("pdconv_no_node_feat", False, False, "sum_min"), ("gat_full", True, True, "sum_minmax"))


def frac_above(a, b, tol=1e-4):
    """The share of elements that differ by more than tol x the largest reference value: on a million rows float32 rounding decides a few
    near-ties of min / max (and signs at the PReLU) differently in two implementations, and each moves one element's gradient."""
    d = (a.double() - b.double()).abs()
    return float((d > tol * float(b.double().abs().max())).double().mean())


def torch_layer(torch, x, src, tgt, p, nf, ea, agg):
    """The layer in torch ops on the device (float32): the formulas of include/tlcgnn.h over the entry list."""
    import torch.nn.functional as F
    n, C = x.shape[0], p["wl"].shape[0]
    xl = x @ p["wl"].t()
    h = xl[src]
    if nf:
        h = F.leaky_relu(torch.cat((xl[tgt], h), dim=1) @ p["wij"].t(), 0.2)
    if ea:
        alpha = xl @ p["att"]
        lg = F.leaky_relu(alpha[src] + alpha[tgt], 0.2)
        mx = torch.full((n,), -float("inf"), device=x.device).scatter_reduce(0, tgt, lg, "amax", include_self=False)
        ex = (lg - mx[tgt]).exp()
        h = h * (ex / (torch.zeros(n, device=x.device).index_add_(0, tgt, ex)[tgt] + 1e-16))[:, None]
    idx = tgt[:, None].expand(-1, C)
    zero = torch.zeros((n, C), device=x.device)
    second = zero.scatter_reduce(0, idx, h, "amin", include_self=False)
    if agg == "sum_minmax":
        second = second + zero.scatter_reduce(0, idx, h, "amax", include_self=False)
    out = torch.cat((zero.index_add(0, tgt, h), second), dim=1) + p["bias"]
    return F.prelu(out, torch.tensor(SLOPE, device=x.device))


def measure_layers(torch, x0, ei, gptr, eptr):
    from tlc_gnn_amd import ops
    from tlc_gnn_amd.Knowledge_Distillation.gat_conv import GraphBatch
    n = x0.shape[0]
    gen = torch.Generator().manual_seed(1234)
    x = torch.randn(n, C_IN, generator=gen).cuda()
    G = torch.randn(n, 2 * C_OUT, generator=gen).cuda()
    p = {"wl": torch.randn(C_OUT, C_IN, generator=gen) * 0.09, "att": torch.randn(C_OUT, generator=gen) * 0.18,
         "wij": torch.randn(C_OUT, 2 * C_OUT, generator=gen) * 0.09, "bias": torch.randn(2 * C_OUT, generator=gen) * 0.2}
    p = {k: v.cuda() for k, v in p.items()}
    b = GraphBatch(ei, n, tiled=False)
    nnz = int(b.rowptr[n])
    out = dict(nodes=n, entries=nnz, graphs=int(gptr.numel()) - 1, c_in=C_IN, c_out=C_OUT)
    out["transpose_build_ms"], _, t = windows(torch, lambda: ops.csr_transpose_pos(b.rowptr, b.col, n), reps=3)
    keep = ei[0] != ei[1]
    loops = torch.arange(n, device=ei.device)
    src, tgt = torch.cat([ei[0][keep], loops]), torch.cat([ei[1][keep], loops])
    for name, nf, ea, agg in CONFIGS:
        mode = ops.msg_mode(nf, ea)
        r = {}
        r["fwd_ms"], r["fwd_ms_all"], o = windows(torch, lambda: ops.msg_layer(b.rowptr, b.col, x, p["wl"], p["att"], p["wij"], p["bias"], mode, agg, SLOPE))
        r["bwd_ms"], r["bwd_ms_all"], g = windows(torch, lambda: ops.msg_layer_bwd(b.rowptr, b.col, *t, x, p["wl"], p["att"], p["wij"], mode, agg, SLOPE, o, G))
        r["bwd_first_layer_ms"], _, _ = windows(torch, lambda: ops.msg_layer_bwd(b.rowptr, b.col, *t, x, p["wl"], p["att"], p["wij"], mode, agg, SLOPE, o, G,
                                                                                 need_gx=False))
        with torch.no_grad():
            r["torch_fwd_ms"], r["torch_fwd_ms_all"], ot = windows(torch, lambda: torch_layer(torch, x, src, tgt, p, nf, ea, agg))
        leaves = {k: v.clone().requires_grad_() for k, v in p.items()}
        xr = x.clone().requires_grad_()

        def torch_step():
            xr.grad = None
            for v in leaves.values():
                v.grad = None
            (torch_layer(torch, xr, src, tgt, leaves, nf, ea, agg) * G).sum().backward()
            return xr.grad
        r["torch_fwd_bwd_ms"], r["torch_fwd_bwd_ms_all"], gxt = windows(torch, torch_step)
        r["fwd_rel_diff_vs_torch"], r["gx_rel_diff_vs_torch"] = rel(o, ot), rel(g[0], gxt)
        r["gx_share_above_1e-4_vs_torch"] = frac_above(g[0], gxt)
        if name == "gat_full":
            r["gat_layer_fwd_ms"], r["gat_layer_fwd_ms_all"], oo = windows(torch, lambda: ops.gat_layer(b.rowptr, b.col, x, p["wl"], p["att"], p["wij"], p["bias"],
                                                                                                         prelu_slope=SLOPE))
            r["gat_layer_bwd_ms"], r["gat_layer_bwd_ms_all"], og = windows(torch, lambda: ops.gat_layer_bwd(b.rowptr, b.col, x, p["wl"], p["att"], p["wij"], SLOPE,
                                                                                                             oo, G))
            r["fwd_rel_diff_vs_gat_layer"], r["gx_rel_diff_vs_gat_layer"] = rel(o, oo), rel(g[0], og[0])
            r["gx_share_above_1e-4_vs_gat_layer"], r["gat_layer_gx_rel_diff_vs_torch"] = frac_above(g[0], og[0]), rel(og[0], gxt)
            r["bwd_over_atomic_bwd"] = r["bwd_ms"] / r["gat_layer_bwd_ms"]
            r["fwd_over_gat_layer_fwd"] = r["fwd_ms"] / r["gat_layer_fwd_ms"]
            note("full configuration: new family fwd %.3f / bwd %.3f ms; tlc_gat_layer fwd %.3f / bwd (atomics) %.3f ms"
                 % (r["fwd_ms"], r["bwd_ms"], r["gat_layer_fwd_ms"], r["gat_layer_bwd_ms"]))
        note("%s: fwd %.3f ms, bwd %.3f ms (first layer %.3f); torch ops fwd %.3f ms, fwd + bwd %.3f ms"
             % (name, r["fwd_ms"], r["bwd_ms"], r["bwd_first_layer_ms"], r["torch_fwd_ms"], r["torch_fwd_bwd_ms"]))
        out[name] = r
    return out


def measure_train(torch, x, ei, gptr, eptr):
    import numpy as np
    from tlc_gnn_amd.Knowledge_Distillation.Teacher_model import Teacher_Model
    n, m = x.shape[0], ei.shape[1] - x.shape[0]
    rs = np.random.RandomState(7)
    bb = rs.rand(m)
    PD = torch.tensor(np.stack([bb, bb + rs.uniform(0, 0.6, size=m)], 1), dtype=torch.float32).cuda()
    out = dict(nodes=n, edges=m, graphs=int(gptr.numel()) - 1)
    for nf, ea in ((True, True), (True, False), (False, True), (False, False)):
        torch.manual_seed(1234)
        model = Teacher_Model(type='GAT', dropout=0.0, new_node_feat=nf, use_edge_attn=ea).cuda().train()

        def step():
            model.zero_grad(set_to_none=True)
            loss = model(x, ei, PD, kernel='wasserstein', p=2, grad_PI=False, graph_ptr=gptr, edge_ptr=eptr)[2]
            loss.backward()
            return loss.detach()
        r = {}
        r["step_ms"], r["step_ms_all"], _ = windows(torch, step)
        note("training step, new_node_feat=%s use_edge_attn=%s: %.3f ms" % (nf, ea, r["step_ms"]))
        out["new_node_feat=%s,use_edge_attn=%s" % (nf, ea)] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="hiv,amazon,train")
    ap.add_argument("--n-graphs", type=int, default=41127)
    ap.add_argument("--train-graphs", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "msg_layers_timing.json"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "time_msg_layers.py measures on the GPU; there is no CPU fallback"
    res = {"tool": "time_msg_layers", "device": torch.cuda.get_device_name(0), "timer": "torch.cuda.Event around one call, median of five windows"}
    for part in a.parts.split(","):
        if part == "hiv":
            res[part] = measure_layers(torch, *hiv_batch(torch, a.n_graphs))
        elif part == "amazon":
            res[part] = measure_layers(torch, *amazon_batch(torch))
        else:
            res[part] = measure_train(torch, *hiv_batch(torch, a.train_graphs))
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())

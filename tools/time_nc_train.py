"""Milliseconds per node-classification training step and per test() (pipelines_GIN.train / .test: ConvCurv_GIN.Net, two curvGN
layers on the HIP kernels of nc_curv.hip) against the same step restated in f32 torch ops (index_add_ / scatter_reduce softmax,
autograd, the same Adam) on the same GPU.

Workloads from synth with planted labels and random w_mul rows: PubMed shape (19 717 nodes, 44 324 edges -> E = 108 365 with the self
loops, F = 500, hidden 256, 3 classes) and Photo shape (7 650 nodes, 119 081 edges -> E = 245 812, F = 745, hidden 256, 8 classes).
The two sides alternate in blocks (`--rounds` rounds of `--steps` steps each, after `--warmup` untimed steps of both), each block timed
with device events.  Also times Net.compute_PI at PubMed shape (--pi).  Prints one JSON line.  The kernel table comes from a separate
`rocprofv3 --kernel-trace --stats -- python tools/time_nc_train.py --only hip` run."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# the edge MLP's FLOPs per step at C = hidden (layer 1 dominates): forward 2 E (D C + C^2), backward twice that; the projection
# 2 N F C forward and the same for dW (the first layer needs no dx)
PEAK_F32_MFMA_TF = 157.3


def _workload(torch, shape, seed=0):
    from tlc_gnn_amd import synth
    from tlc_gnn_amd.data import Data
    n, edges, _, _, F_in = synth.shaped_graph(shape)
    k = {"PubMed": 3, "Photo": 8}[shape]
    rs = np.random.RandomState(seed)
    y = rs.randint(0, k, n)
    und = torch.from_numpy(edges.T.copy()).long()
    loops = torch.arange(n)
    ei = torch.cat([und, und.flip(0), torch.stack([loops, loops])], dim=1)
    x = synth.synthetic_features(n, F_in).astype(np.float32)
    x[np.arange(n), y] += 1.0                                      # planted labels
    w_mul = rs.uniform(0, 0.3, (ei.shape[1], 50)).astype(np.float32)
    w_mul[(ei[0] == ei[1]).numpy()] = 0
    data = Data(x=torch.from_numpy(x), edge_index=ei, y=torch.from_numpy(y).long()).to("cuda")
    return data, torch.from_numpy(w_mul).cuda(), F_in, k


def _flops(n, E, F_in, C, D=50):
    return 3 * 2 * E * (D * C + C * C) + 2 * 2 * n * F_in * C


def run_shape(torch, shape, args):
    import torch.nn.functional as F
    from tlc_gnn_amd import pipelines_GIN
    from tlc_gnn_amd.Knowledge_Distillation import ConvCurv_GIN
    name = {"PubMed": "PubMed", "Photo": "photo"}[shape]
    data, w_mul, F_in, k = _workload(torch, shape)
    n, E = data.num_nodes, data.edge_index.shape[1]
    torch.manual_seed(0)
    model = ConvCurv_GIN.Net(data, name, F_in, k, w_mul=w_mul).cuda()
    opt = pipelines_GIN.optimizer_for(model)
    masks = pipelines_GIN.split_masks(data, "Amazon")
    tp = {kk: torch.nn.Parameter(v.detach().clone()) for kk, v in model.named_parameters() if not kk.startswith("modelGIN")}
    topt = torch.optim.Adam(tp.values(), lr=0.005, weight_decay=0.0005)
    ei = data.edge_index
    p_drop = ConvCurv_GIN.dropout_of(name)

    def layer(h, pre):
        xl = F.linear(h, tp[pre + "lin.weight"], tp[pre + "lin.bias"])
        wt = F.linear(F.prelu(F.linear(w_mul, tp[pre + "w_mlp_out.0.weight"]), tp[pre + "w_mlp_out.1.weight"]), tp[pre + "w_mlp_out.2.weight"],
                      tp[pre + "w_mlp_out.2.bias"])
        idx = ei[0].view(-1, 1).expand_as(wt)
        mx = torch.full((n, wt.shape[1]), float("-inf"), device=wt.device).scatter_reduce(0, idx, wt, reduce="amax", include_self=True)
        ex = (wt - mx[ei[0]]).exp()
        den = torch.zeros((n, wt.shape[1]), device=wt.device).index_add_(0, ei[0], ex)
        alpha = ex / (den[ei[0]] + 1e-16)
        return torch.zeros((n, xl.shape[1]), device=xl.device).index_add_(0, ei[1], alpha * xl[ei[0]])

    def torch_forward(training):
        h = F.dropout(data.x, p=p_drop, training=training)
        h = F.dropout(F.elu(layer(h, "conv1.")), p=p_drop, training=training)
        return F.log_softmax(layer(h, "conv2."), dim=1)

    def torch_step():
        topt.zero_grad()
        F.nll_loss(torch_forward(True)[masks[0]], data.y[masks[0]]).backward()
        topt.step()

    def torch_test():
        with torch.no_grad():
            logits = torch_forward(False)
            accs = [logits[m].max(1)[1].eq(data.y[m]).sum().item() / m.sum().item() for m in masks]
            accs.append(F.nll_loss(logits[masks[1]], data.y[masks[1]]))
        return accs

    sides = {"hip": (lambda: pipelines_GIN.train(model, data, opt, masks[0]), lambda: pipelines_GIN.test(model, data, *masks)),
             "torch": (torch_step, torch_test)}
    if args.only:
        sides = {args.only: sides[args.only]}
    for _ in range(args.warmup):
        for st, te in sides.values():
            st()
            te()
    torch.cuda.synchronize()
    times = {s: {"step": [], "test": []} for s in sides}
    for _ in range(args.rounds):
        for s, fns in sides.items():
            for what, fn in zip(("step", "test"), fns):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.steps):
                    fn()
                e1.record()
                e1.synchronize()
                times[s][what].append(e0.elapsed_time(e1) / args.steps)
    out = {"shape": shape, "n": n, "E": E, "F": F_in, "hidden": ConvCurv_GIN.hidden_dim_of(name), "classes": k}
    for s in times:
        for what in ("step", "test"):
            out["%s_ms_per_%s" % (s, what)] = float(np.median(times[s][what]))
            out["%s_ms_per_%s_all" % (s, what)] = [round(t, 4) for t in times[s][what]]
    fl = _flops(n, E, F_in, ConvCurv_GIN.hidden_dim_of(name))
    out["gflop_per_step"] = fl / 1e9
    out["floor_ms"] = fl / (PEAK_F32_MFMA_TF * 1e12) * 1e3
    if "hip" in times:
        out["hip_step_fraction_of_floor"] = out["floor_ms"] / out["hip_ms_per_step"]
    if len(times) == 2:
        out["torch_over_hip_step"] = out["torch_ms_per_step"] / out["hip_ms_per_step"]
        out["torch_over_hip_test"] = out["torch_ms_per_test"] / out["hip_ms_per_test"]
    return out


def time_pi(torch):
    """Net.compute_PI at PubMed shape (synthetic curvature, a random-init teacher): seconds for the whole graph."""
    from tlc_gnn_amd import synth
    from tlc_gnn_amd.data import Data
    from tlc_gnn_amd.Knowledge_Distillation import ConvCurv_GIN
    n, edges, kappa, _, _ = synth.shaped_graph("PubMed")
    ricci = synth.synthetic_curvature(edges)
    und = torch.from_numpy(edges.T.copy()).long()
    loops = torch.arange(n)
    data = Data(x=torch.zeros(n, 1), edge_index=torch.cat([und, und.flip(0), torch.stack([loops, loops])], dim=1)).to("cuda")
    torch.manual_seed(3)
    net = ConvCurv_GIN.Net(data, "PubMed", 1, 3, g=edges, ricci_curv=ricci, w_mul=torch.zeros(1, 50))
    net.compute_NodeFeat(data, "PubMed", ricci)
    net.compute_PI(data, "PubMed")                                  # warm-up (kernels, allocator)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    net.compute_PI(data, "PubMed")
    torch.cuda.synchronize()
    return {"compute_PI_s": time.perf_counter() - t0, "nonzero_rows": int((net.PI.abs().sum(1) > 0).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", default="PubMed,Photo")
    ap.add_argument("--only", choices=["hip", "torch"], default=None, help="time one side only (profiling runs)")
    ap.add_argument("--pi", action="store_true", help="also time Net.compute_PI at PubMed shape")
    args = ap.parse_args()
    import torch
    res = {"shapes": [run_shape(torch, s, args) for s in args.shapes.split(",") if s]}
    if args.pi:
        res["pi_pubmed"] = time_pi(torch)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""Milliseconds per TLCGNN link-prediction training step at PubMed shape (pipelines.train: encode, decode('train'), BCE, backward,
Adam step) -- the HIP step against the same step restated in f32 torch ops (index_add_ aggregation, autograd) on the same GPU.

The two alternate inside one run: `--rounds` rounds of `--steps` steps each, the HIP block and the torch block back to back, each
block timed with device events after `--warmup` untimed steps of both.  Prints one JSON line: the median block time per step of
each and their ratio.  The graph, the 37 676 training positives and the negatives are bench.py's LP leg (build_workload); the
image rows are random (their values do not change the work)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", choices=["hip", "torch"], default=None, help="time one side only (profiling runs)")
    args = ap.parse_args()

    import torch
    import torch.nn.functional as F
    import bench
    from tlc_gnn_amd import pipelines
    from tlc_gnn_amd.baselines import TLCGNN
    from tlc_gnn_amd.data import Data
    from oracle import lp_forward_ref as ref

    dev = torch.device("cuda", 0)
    wl = bench.build_workload(0)
    n, te = wl["n"], wl["train_edges"]
    ei = torch.from_numpy(np.concatenate([te, te[:, ::-1]]).T.copy()).long()
    pos, neg = wl["pi_pairs"].astype(np.int64), wl["neg"]
    pairs = np.concatenate([pos, neg])
    PI = torch.from_numpy(np.random.RandomState(7).uniform(0, 0.3, size=(len(pairs), 25))).to(dev)
    y = torch.cat([torch.ones(len(pos)), torch.zeros(len(neg))]).long()
    data = Data(x=torch.from_numpy(wl["x"]), edge_index=ei, y=torch.zeros(n), total_edges=pairs, total_edges_y=y,
                train_pos=len(pos), train_neg=len(neg), val_pos=0, val_neg=0, test_pos=0, test_neg=0).to(dev)
    pipelines.setup_seed(1)
    model = TLCGNN.Net(data, wl["n_feat"], 2, PI=PI)
    model.apply(pipelines.weights_init)
    model = model.to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=0.005)

    # the restatement: its own copy of the parameters, its own Adam
    tp = {k: torch.nn.Parameter(v.detach().clone()) for k, v in model.named_parameters()}
    topt = torch.optim.Adam(tp.values(), lr=0.005)
    e2, norm = ref.gcn_norm(ei, n)
    src, dst, norm = e2[0].to(dev), e2[1].to(dev), norm.to(dev)
    pairs_d = torch.from_numpy(pairs).to(dev)
    pi32 = PI.float()
    y_d = y.to(dev).float()
    x = data.x

    def conv(h, w, b):
        xw = h @ w
        return torch.zeros((n, xw.shape[1]), device=dev).index_add_(0, dst, norm[:, None] * xw[src]) + b

    def torch_step():
        topt.zero_grad()
        h = F.dropout(x, p=0.5, training=True)
        h = F.dropout(F.relu(conv(h, tp["conv1.weight"], tp["conv1.bias"])), p=0.5, training=True)
        emb = F.relu(conv(h, tp["conv2.weight"], tp["conv2.bias"])).renorm(2, 0, 1)
        index = np.random.randint(0, len(neg), len(pos))
        idx = torch.cat((torch.arange(len(pos), device=dev), len(pos) + torch.from_numpy(index).to(dev)))
        pr = pairs_d[idx]
        a, b = emb[pr[:, 0]], emb[pr[:, 1]]
        hh = F.leaky_relu(F.linear(torch.cat(((a - b).pow(2), pi32[idx]), 1), tp["linear_1.weight"], tp["linear_1.bias"]), 0.2)
        d = torch.clamp(torch.abs(F.linear(hh, tp["linear.weight"], tp["linear.bias"])).reshape(-1), min=0, max=40)
        prob = 1.0 / (torch.exp((d - 2.0) / 1.0) + 1.0)
        F.binary_cross_entropy(prob, y_d[idx]).backward()
        topt.step()

    def hip_step():
        pipelines.train(model, data, opt)

    sides = {"hip": hip_step, "torch": torch_step}
    if args.only:
        sides = {args.only: sides[args.only]}
    for _ in range(args.warmup):
        for fn in sides.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in sides}
    for _ in range(args.rounds):
        for k, fn in sides.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / args.steps)
    out = {"shape": "PubMed", "steps": args.steps, "rounds": args.rounds, "pairs_per_step": 2 * len(pos)}
    for k, v in times.items():
        out["%s_ms_per_step" % k] = float(np.median(v))
        out["%s_ms_per_step_all" % k] = [round(t, 4) for t in v]
    if len(times) == 2:
        out["torch_over_hip"] = out["torch_ms_per_step"] / out["hip_ms_per_step"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()

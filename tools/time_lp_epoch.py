"""Milliseconds per TLCGNN link-prediction evaluation (pipelines.test) and per epoch (pipelines.train + test, the body of
pipelines.fit) at PubMed shape, scoring with sklearn on the host (the default) against scoring on the device (metrics="device"),
plus the device time of the metrics kernels (tlc_binary_rank_metrics) for one segment of 4 k, 64 k, 1 M and 16 M scores.

The graph, the training positives and negatives are bench.py's LP leg (build_workload); the val / test positives are the 5 % / 10 %
of the positives build_workload holds out (the reference's get_adj_split), each with as many negatives (non-adjacent pairs, seeded).
The image rows are random (their values do not change the work).  The two sides alternate inside one run: `--rounds` rounds of
`--steps` calls each, wall time on the host around a block (test() returns host numbers, so every call ends synchronised).
Kernel time: one call captured into a graph (ops.capture) and replayed `--replays` times between device events.  Prints one JSON
line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _negatives(n, adj, k, rs):
    out = []
    while len(out) < k:
        for x, y in zip(rs.randint(0, n, 2 * k).tolist(), rs.randint(0, n, 2 * k).tolist()):
            if x != y and (min(x, y), max(x, y)) not in adj:
                out.append((x, y))
                if len(out) == k:
                    break
    return np.array(out, dtype=np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--replays", type=int, default=20)
    args = ap.parse_args()

    import torch
    import bench
    from tlc_gnn_amd import pipelines, ops
    from tlc_gnn_amd.baselines import TLCGNN
    from tlc_gnn_amd.data import Data

    dev = torch.device("cuda", 0)
    wl = bench.build_workload(0)
    n, te, allpos = wl["n"], wl["train_edges"], wl["all_pos"]
    n_val, n_test = int(len(allpos) * 0.05), int(len(allpos) * 0.1)
    val_pos, test_pos = allpos[:n_val].astype(np.int64), allpos[n_val:n_val + n_test].astype(np.int64)
    adj = set(map(tuple, np.sort(allpos, axis=1).tolist()))
    rs = np.random.RandomState(99)
    val_neg, test_neg = _negatives(n, adj, n_val, rs), _negatives(n, adj, n_test, rs)
    tr_pos, tr_neg = wl["pi_pairs"].astype(np.int64), wl["neg"]
    pairs = np.concatenate([tr_pos, tr_neg, val_pos, val_neg, test_pos, test_neg])
    y = np.concatenate([np.ones(len(tr_pos)), np.zeros(len(tr_neg)), np.ones(n_val), np.zeros(n_val), np.ones(n_test),
                        np.zeros(n_test)]).astype(np.int64)
    ei = torch.from_numpy(np.concatenate([te, te[:, ::-1]]).T.copy()).long()
    PI = torch.from_numpy(np.random.RandomState(7).uniform(0, 0.3, size=(len(pairs), 25))).to(dev)
    data = Data(x=torch.from_numpy(wl["x"]), edge_index=ei, y=torch.zeros(n), total_edges=pairs, total_edges_y=torch.from_numpy(y),
                train_pos=len(tr_pos), train_neg=len(tr_neg), val_pos=n_val, val_neg=n_val, test_pos=n_test, test_neg=n_test).to(dev)
    pipelines.setup_seed(1)
    model = TLCGNN.Net(data, wl["n_feat"], 2, PI=PI)
    model.apply(pipelines.weights_init)
    model = model.to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=0.005)

    blocks = {
        "test_sklearn": lambda: pipelines.test(model, data),
        "test_device": lambda: pipelines.test(model, data, metrics="device"),
        "epoch_sklearn": lambda: (pipelines.train(model, data, opt), pipelines.test(model, data)),
        "epoch_device": lambda: (pipelines.train(model, data, opt), pipelines.test(model, data, metrics="device")),
    }
    for _ in range(args.warmup):
        for fn in blocks.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in blocks}
    for _ in range(args.rounds):
        for k, fn in blocks.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3 / args.steps)
    out = {"shape": "PubMed", "val_pairs": 2 * n_val, "test_pairs": 2 * n_test, "steps": args.steps, "rounds": args.rounds}
    for k, v in times.items():
        out["%s_ms" % k] = round(float(np.median(v)), 4)
        out["%s_ms_all" % k] = [round(t, 4) for t in v]
    out["test_sklearn_over_device"] = round(out["test_sklearn_ms"] / out["test_device_ms"], 3)
    out["epoch_sklearn_over_device"] = round(out["epoch_sklearn_ms"] / out["epoch_device_ms"], 3)

    # device time of the metrics kernels: one segment, f32 scores (what Net.decode returns), float labels
    kern = {}
    g = torch.Generator(device=dev).manual_seed(3)
    for size in (4096, 65536, 1 << 20, 1 << 24):
        s = torch.rand(size, device=dev, generator=g)
        lab = (torch.rand(size, device=dev, generator=g) < 0.5).float()
        graph = ops.capture(lambda: ops.binary_rank_metrics(s, lab))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        graph.replay()
        e0.record()
        for _ in range(args.replays):
            graph.replay()
        e1.record()
        e1.synchronize()
        kern[str(size)] = round(e0.elapsed_time(e1) / args.replays, 4)
        del graph
    out["metrics_kernel_ms"] = kern
    print(json.dumps(out))


if __name__ == "__main__":
    main()

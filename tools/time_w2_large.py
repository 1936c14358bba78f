"""What the workspace tier of the matching loss costs (csrc/w2_large.hip) -> profiles/w2_large_timing.json.

One MI355X, device events.  Every case runs in a child process of its own under a time limit (`--limit` seconds), the largest last; a
case that fails or runs out of time ends the run, and what was measured until then is written.  Per case: milliseconds (the median of
`reps` runs: 5 where a run takes under 2 s, 3 under 20 s, else the one run), the steps and augmentations its workgroup counted (the
first int64 words of a workspace slot), and scipy.optimize.linear_sum_assignment on the host in the same process where its dense
matrix is at most 8 192 square -- first of all its optimum is compared with the cost of the device's matching.

    python tools/time_w2_large.py [--out profiles/w2_large_timing.json] [--limit 900] [--only NAME ...] [--reps K]
    python tools/time_w2_large.py --case NAME          (one case, one JSON line; what the parent starts)
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCIPY_NMAX = 8192
# name: (form, n, m, problems)
CASES = {}
for order in (2, 1):
    CASES["train_4096x3000_wide_p%d" % order] = ("wide", 4096, 3000, 1, order)        # the parent's LDS kernel at the cut
    CASES["train_4096x3000_p%d" % order] = ("train", 4096, 3000, 1, order)
    CASES["train_4097x3000_p%d" % order] = ("train", 4097, 3000, 1, order)
    CASES["eval_2049+2048_p%d" % order] = ("eval", 2049, 2048, 1, order)
    CASES["eval_4100+50_p%d" % order] = ("eval", 4100, 50, 1, order)
for order in (2, 1):
    CASES["train_8192x6000_p%d" % order] = ("train", 8192, 6000, 1, order)
CASES["batch64_train_5000x3700_p2"] = ("train", 5000, 3700, 64, 2)
for order in (2, 1):
    CASES["eval_8192+8192_p%d" % order] = ("eval", 8192, 8192, 1, order)
for order in (2, 1):
    CASES["train_16384x12000_p%d" % order] = ("train", 16384, 12000, 1, order)
for order in (2, 1):
    CASES["train_30000x22000_p%d" % order] = ("train", 30000, 22000, 1, order)


def pair(rs, n, m):
    """the `random` style of tests/test_gpu_train.py: continuous coordinates, a few predicted points below the diagonal"""
    b0 = rs.rand(n)
    X = np.stack([b0, b0 + rs.uniform(-0.1, 0.6, size=n)], 1)
    b1 = rs.rand(m)
    Y = np.stack([b1, b1 + rs.uniform(0.0, 0.7, size=m)], 1)
    return X, Y


def host_cost(X, Y, order, infer, ax, ay=None):
    n, m = len(X), len(Y)
    on = ax >= 0
    cxd = ((X[:, 1] - X[:, 0]) * 0.5) ** order
    cost = float((np.abs(Y[ax[on]] - X[on]).max(axis=1) ** order).sum() + cxd[~on].sum())
    if infer:
        cost += float((((Y[:, 1] - Y[:, 0]) * 0.5) ** order)[ay < 0].sum())
    return cost


def host_optimum(X, Y, order, infer):
    from scipy.optimize import linear_sum_assignment
    n, m = len(X), len(Y)
    N = n + m if infer else n
    big = np.zeros((N, N))
    big[:n, :m] = np.abs(X[:, None, :] - Y[None, :, :]).max(axis=2) ** order
    big[:n, m:] = (((X[:, 1] - X[:, 0]) * 0.5) ** order)[:, None]
    if infer:
        big[n:, :m] = (((Y[:, 1] - Y[:, 0]) * 0.5) ** order)[None, :]
    t = time.time()
    rows, cols = linear_sum_assignment(big)
    ms = (time.time() - t) * 1e3
    return float(big[rows, cols].sum()), ms


def run_case(name, reps=None):
    import torch
    from tlc_gnn_amd import _lib, ops
    form, n, m, B, order = CASES[name]
    infer = form == "eval"
    rs = np.random.RandomState(n + m + order)
    pairs = [pair(rs, n, m) for _ in range(B)]
    xoff = torch.as_tensor(np.arange(B + 1, dtype=np.int64) * n).cuda()
    yoff = torch.as_tensor(np.arange(B + 1, dtype=np.int64) * m).cuda()
    X = torch.as_tensor(np.concatenate([p[0] for p in pairs])).cuda()
    Y = torch.as_tensor(np.concatenate([p[1] for p in pairs])).cuda()
    if form == "wide":
        call = lambda: ops.w2_partial_matching(xoff, X, yoff, Y, order=order, want_grad=True, max_points=n)
    else:
        call = lambda: ops.w2_large_matching(xoff, X, yoff, Y, order=order, infer=infer, want_grad=True)

    def timed():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = call()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), r

    first, r = timed()
    out = dict(case=name, form=form, n=n, m=m, rows=n + m if infer else n, problems=B, order=order, first_ms=first)
    assert bool((r["status"] == 0).all()), r["status"].tolist()
    ax = (r["assign"] if form == "wide" else r["assign_x"]).cpu().numpy()
    ay = r["assign_y"].cpu().numpy() if infer else None
    out["device_cost"] = host_cost(pairs[0][0], pairs[0][1], order, infer, ax[:n], None if ay is None else ay[:m])
    if out["rows"] <= SCIPY_NMAX:
        out["scipy_cost"], out["scipy_ms"] = host_optimum(pairs[0][0], pairs[0][1], order, infer)
        out["cost_rel_diff"] = abs(out["device_cost"] - out["scipy_cost"]) / max(1.0, abs(out["scipy_cost"]))
        assert out["cost_rel_diff"] <= 1e-9, out
    if form != "wide":
        stride = int(_lib.lib().tlc_w2_large_work_bytes(out["rows"], 1))
        w = r["work"]
        ctr = np.stack([w[k * stride:k * stride + 8 * _lib.W2_LARGE_COUNTERS].view(torch.int64).cpu().numpy() for k in range(w.numel() // stride)])
        out.update(slots=int(len(ctr)), steps=int(ctr[:, 0].sum()), augmentations=int(ctr[:, 1].sum()), rows_start_assigned=int(ctr[:, 2].sum()))
    reps = reps or (5 if first < 2e3 else (3 if first < 2e4 else 1))
    ms = [first] if reps == 1 else [timed()[0] for _ in range(reps)]
    out.update(reps=reps, ms=float(np.median(ms)), ms_all=[float(v) for v in ms])
    if "steps" in out and out["steps"]:
        out["us_per_step"] = out["ms"] * 1e3 / (out["steps"] / max(1, min(B, out.get("slots", 1))))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "w2_large_timing.json"))
    ap.add_argument("--limit", type=int, default=900)
    ap.add_argument("--case")
    ap.add_argument("--only", nargs="*")
    ap.add_argument("--reps", type=int, help="runs per case instead of 5 / 3 / 1 by the first run's time")
    a = ap.parse_args()
    if a.case:
        print("RESULT " + json.dumps(run_case(a.case, a.reps)))
        return 0
    results, ended = [], None
    for name in (a.only or CASES):
        t = time.time()
        try:
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name] + (["--reps", str(a.reps)] if a.reps else []), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                                 text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            ended = "%s: no result within %d s" % (name, a.limit)
            break
        line = [l for l in res.stdout.splitlines() if l.startswith("RESULT ")]
        if res.returncode != 0 or not line:
            ended = "%s: exit status %d\n%s" % (name, res.returncode, res.stdout[-2000:])
            break
        results.append(json.loads(line[-1][7:]))
        print("%-32s %10.1f ms  %s  (%.0f s in all)" % (name, results[-1]["ms"], {k: results[-1].get(k) for k in ("steps", "augmentations", "scipy_ms")},
                                                     time.time() - t), flush=True)
        with open(a.out, "w") as f:
            json.dump(dict(device="MI355X", timer="device events", cases=results), f, indent=1)
    if ended:
        print("ended early: " + ended, flush=True)
        with open(a.out, "w") as f:
            json.dump(dict(device="MI355X", timer="device events", cases=results, ended_early=ended), f, indent=1)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())

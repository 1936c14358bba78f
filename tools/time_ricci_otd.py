"""Ollivier-Ricci curvature of every edge of the PubMed-shaped (44 324 edges) and Photo-shaped graphs with both transport methods,
tlc_ollivier_ricci_sinkhorn and tlc_ollivier_ricci_otd (exact), on the same edges in the same process: median of --reps runs after a
warm-up (host clock around a call that ends in a synchronise, uploads included) for all edges, for the edges the exact method's
wavefront kernel takes ("small") and for those it leaves to the workgroup kernel ("hub") separately, and for the slowest single hub
edge among the --singles largest supports.  As the host comparison scipy's HiGHS LP solves a fixed sample of 200 small edges (its
time per edge, and its integers against the device's).  Every graph is measured in a child process of its own under --step-timeout
seconds; a child that fails or runs out of time ends the tool: nothing else is started on the GPU.
Prints ONE JSON line.

  python tools/time_ricci_otd.py [--graphs PubMed,Photo] [--reps 5] [--singles 8] [--step-timeout 420] [--out profiles/ricci_otd_timing.json]
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


def lp_wd(rowptr, col, s, t, num=1, den=2):
    """(W, D) of one edge by scipy's LP on the scaled integer problem (hop distances by a three-level search from each source)"""
    import scipy.sparse as sp
    from scipy.optimize import linprog
    nbr = lambda v: col[rowptr[v]:rowptr[v + 1]]
    xs, ys = np.concatenate([nbr(s), [s]]), np.concatenate([nbr(t), [t]])
    ds, dt = len(xs) - 1, len(ys) - 1
    pos = {int(y): j for j, y in enumerate(ys)}
    cost = np.full((len(xs), len(ys)), 3.0)
    for i, a in enumerate(xs):
        for y in nbr(a):
            for z in nbr(y):
                if int(z) in pos:
                    cost[i, pos[int(z)]] = 2.0
        for y in nbr(a):
            if int(y) in pos:
                cost[i, pos[int(y)]] = 1.0
        if int(a) in pos:
            cost[i, pos[int(a)]] = 0.0
    a = np.array([(den - num) * dt] * ds + [num * ds * dt], dtype=np.float64)
    b = np.array([(den - num) * ds] * dt + [num * ds * dt], dtype=np.float64)
    A = sp.vstack([sp.kron(sp.eye(len(xs)), np.ones((1, len(ys)))), sp.kron(np.ones((1, len(xs))), sp.eye(len(ys)))]).tocsr()
    res = linprog(cost.ravel(), A_eq=A, b_eq=np.concatenate([a, b]), method="highs")
    assert res.status == 0 and abs(res.fun - round(res.fun)) < 1e-6
    return int(round(res.fun)), den * ds * dt


def median_s(fn, reps):
    import torch
    fn()                                                              # warm-up
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), [round(x, 5) for x in ts]


def measure(name, reps, singles):
    import torch
    from tlc_gnn_amd import _lib, engine, synth
    assert torch.cuda.is_available(), "time_ricci_otd.py measures on the GPU; there is no CPU fallback"
    n, edges = synth.shaped_graph(name)[:2]
    edges = np.unique(np.sort(np.asarray(edges, dtype=np.int64), axis=1), axis=0)
    rowptr, col, _ = synth.edges_to_csr(n, edges)
    deg = np.diff(rowptr).astype(np.int64)
    na, nb = deg[edges[:, 0]] + 1, deg[edges[:, 1]] + 1
    hub = (na * nb > _lib.OTD_WAVE_PRODUCT) | (na + nb > _lib.OTD_WAVE_SUPPORT) | (2 * (na - 1) * (nb - 1) > _lib.OTD_WAVE_DENOM)
    r = {"nodes": int(n), "edges": int(len(edges)), "small_edges": int((~hub).sum()), "hub_edges": int(hub.sum()), "max_degree": int(deg.max()),
         "max_support_product": int((na * nb).max()), "device": torch.cuda.get_device_name(0)}
    sets = {"all": edges, "small": edges[~hub], "hub": edges[hub]}
    for key, e in sets.items():
        if len(e) == 0:
            continue
        q = {}
        for method, fn in (("otd", lambda: engine.ollivier_ricci_otd(rowptr, col, e)), ("sinkhorn", lambda: engine.ollivier_ricci_sinkhorn(rowptr, col, e))):
            q[method + "_s"], q[method + "_s_all"] = median_s(fn, reps)
        q["otd_over_sinkhorn"] = q["otd_s"] / q["sinkhorn_s"]
        r[key] = q
        print("# %s %s (%d edges): otd %.4f s, sinkhorn %.4f s, ratio %.2f" % (name, key, len(e), q["otd_s"], q["sinkhorn_s"], q["otd_over_sinkhorn"]),
              file=sys.stderr, flush=True)
    if hub.any():
        order = np.argsort(-(na * nb)[hub], kind="stable")[:singles]
        worst = None
        for k in order.tolist():
            e = sets["hub"][k:k + 1]
            q = {"edge": e[0].tolist(), "support": [int(deg[e[0, 0]]) + 1, int(deg[e[0, 1]]) + 1]}
            q["otd_s"], _ = median_s(lambda: engine.ollivier_ricci_otd(rowptr, col, e), reps)
            q["sinkhorn_s"], _ = median_s(lambda: engine.ollivier_ricci_sinkhorn(rowptr, col, e), reps)
            if worst is None or q["otd_s"] > worst["otd_s"]:
                worst = q
        r["slowest_single_hub_edge"] = worst
        print("# %s slowest single hub edge: %s" % (name, worst), file=sys.stderr, flush=True)
    # the host comparison: a fixed sample of 200 small edges through scipy's LP
    small = sets["small"]
    sample = small[np.random.RandomState(0).permutation(len(small))[:200]]
    _, w, d = engine.ollivier_ricci_otd(rowptr, col, sample, want_cost=True)
    t0 = time.perf_counter()
    ref = [lp_wd(rowptr, col, int(s), int(t)) for s, t in sample.tolist()]
    lp_s = time.perf_counter() - t0
    dev_s, _ = median_s(lambda: engine.ollivier_ricci_otd(rowptr, col, sample), reps)
    r["lp_sample"] = {"edges": int(len(sample)), "scipy_highs_s": lp_s, "scipy_highs_s_per_edge": lp_s / max(1, len(sample)), "device_s": dev_s,
                      "equal": bool(w.tolist() == [x for x, _ in ref] and d.tolist() == [x for _, x in ref])}
    print("# %s LP sample: %s" % (name, r["lp_sample"]), file=sys.stderr, flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="PubMed,Photo")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--singles", type=int, default=8)
    ap.add_argument("--step-timeout", type=int, default=420)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(measure(a.child, a.reps, a.singles)))
        return 0
    res = {"tool": "time_ricci_otd", "reps": a.reps}
    for name in a.graphs.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(a.reps), "--singles", str(a.singles)]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.step_timeout)
        except subprocess.TimeoutExpired:
            print("time_ricci_otd: %s did not finish within %d s; stopping" % (name, a.step_timeout), file=sys.stderr)
            return 124
        if p.returncode != 0:
            print("time_ricci_otd: %s failed with status %d; stopping" % (name, p.returncode), file=sys.stderr)
            return p.returncode or 1
        res[name] = json.loads(p.stdout.strip().splitlines()[-1])
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

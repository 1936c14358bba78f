"""The large HKS tier (tlc_hks_large_batch) against the host fallback (scipy's eigh per graph) on README's third HKS workload: the
node-centred hop-2 vicinities of 4 096 PubMed-shaped nodes through NodeVicinities.batch(filt='hks', hks_backend='device'), times 0.1
and 10.  Per time, each in a child process of its own under its own time limit (a step that fails or runs out of time ends the run;
nothing is started after it):
  pipeline  hks_large='host' against hks_large='device', end to end (extraction included), median of --reps runs after a warm-up each;
  kernel    the graphs above TLC_HKS_NMAX alone: tlc_hks_large_batch (device events, median of --reps) against `hks_signature` for the
            same graphs (host clock, one run), their count and largest size;
  small     one 200-node and one 256-node random connected graph through tlc_hks_batch and through tlc_hks_large_batch (device
            events, median of --reps): the numbers a later change needs to decide whether the Jacobi tier's 97 .. 256 range should move.
Prints ONE JSON line and writes it to --out.

  python tools/time_hks_large.py [--reps 5] [--n-queries 4096] [--limit 600] [--out profiles/hks_large_timing.json]
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
TIMES = (0.1, 10.0)


def wall(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def events_median_ms(fn, reps):
    import torch
    fn()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


def pubmed_vicinities(n_queries):
    from tlc_gnn_amd import synth
    from tlc_gnn_amd.Knowledge_Distillation import data_utils_NC as kd_nc
    _, edges, _, _, _ = synth.shaped_graph("PubMed")
    return kd_nc.NodeVicinities(edges, None), np.random.RandomState(0).permutation(np.unique(edges))[:n_queries], 2


def random_connected(n, seed):
    rs = np.random.RandomState(seed)
    es = {(int(rs.randint(i)), i) for i in range(1, n)}
    for _ in range(2 * n):
        a, b = (int(x) for x in rs.randint(n, size=2))
        if a != b:
            es.add((min(a, b), max(a, b)))
    return np.array(sorted(es), dtype=np.int64)


def step_pipeline(a, t):
    from tlc_gnn_amd.Knowledge_Distillation import data_utils_LP as kd_lp
    vic, query, hop = pubmed_vicinities(a.n_queries)
    r = {}
    for large in ("host", "device"):
        run = lambda: vic.batch(query, hop, filt='hks', hks_time=t, hks_backend='device', hks_large=large)
        run()
        s = [wall(run)[0] for _ in range(a.reps)]
        r["hks_large_%s_s" % large] = float(np.median(s))
        r["hks_large_%s_s_all" % large] = [round(x, 4) for x in s]
        r["hks_large_%s_host_fallback" % large] = int(kd_lp.hks_host_fallback)
        r["hks_large_%s_large_tier" % large] = int(kd_lp.hks_large_device)
    r["host_over_device"] = r["hks_large_host_s"] / r["hks_large_device_s"]
    return r


def step_kernel(a, t):
    from tlc_gnn_amd import engine, _lib
    from tlc_gnn_amd.Knowledge_Distillation.data_utils_LP import hks_signature
    vic, query, hop = pubmed_vicinities(a.n_queries)
    b = vic.batch(query, hop, filt='degree')
    node_ptr, edge_ptr, edges = b["node_ptr"], b["edge_ptr"], b["edges"].contiguous()
    nptr, eptr, e = node_ptr.cpu().numpy(), edge_ptr.cpu().numpy(), edges.cpu().numpy()
    sizes = np.diff(nptr)
    sel = np.nonzero((sizes > _lib.HKS_NMAX) & (sizes <= _lib.HKS_LARGE_NMAX))[0]
    tot = int(nptr[-1])
    run = lambda: engine.hks_large_batch(node_ptr, edge_ptr, edges, sel.tolist(), sizes[sel].tolist(), [t], total_nodes=tot)
    r = dict(graphs=int(len(sel)), of=int((sizes > 0).sum()), n_max=int(sizes[sel].max()) if len(sel) else 0,
             n_median=float(np.median(sizes[sel])) if len(sel) else 0.0, above_large_cap=int((sizes > _lib.HKS_LARGE_NMAX).sum()),
             work_bytes=list(engine.hks_large_work_bytes(sizes[sel].tolist())))
    r["hks_large_batch_ms"] = events_median_ms(run, a.reps)
    f, st = run()
    assert int(st[sel.tolist()].sum()) == 0
    f = f[0].cpu().numpy()
    t0 = time.perf_counter()
    ref = [hks_signature(int(sizes[k]), e[int(eptr[k]):int(eptr[k + 1])], t) for k in sel]
    r["hks_signature_host_s"] = time.perf_counter() - t0
    r["host_over_device"] = r["hks_signature_host_s"] * 1e3 / r["hks_large_batch_ms"]
    r["worst_abs_diff"] = float(max(np.abs(f[nptr[k]:nptr[k + 1]] - v / (max(v) + 1e-10)).max() for k, v in zip(sel, ref))) if len(sel) else 0.0
    return r


def step_small(a, t):
    import torch
    from tlc_gnn_amd import engine
    r = {}
    for n in (200, 256):
        e = random_connected(n, 100 + n)
        node_ptr = torch.tensor([0, n], dtype=torch.int64, device="cuda")
        edge_ptr = torch.tensor([0, len(e)], dtype=torch.int64, device="cuda")
        edges = torch.from_numpy(e.astype(np.int32)).cuda()
        r["n%d_hks_batch_ms" % n] = events_median_ms(lambda: engine.hks_batch(node_ptr, edge_ptr, edges, [t], total_nodes=n), a.reps)
        r["n%d_hks_large_batch_ms" % n] = events_median_ms(lambda: engine.hks_large_batch(node_ptr, edge_ptr, edges, [0], [n], [t], total_nodes=n), a.reps)
        x, _ = engine.hks_batch(node_ptr, edge_ptr, edges, [t], total_nodes=n)
        y, _ = engine.hks_large_batch(node_ptr, edge_ptr, edges, [0], [n], [t], total_nodes=n)
        r["n%d_abs_diff" % n] = float((x - y).abs().max())
    return r


STEPS = {"pipeline": step_pipeline, "kernel": step_kernel, "small": step_small}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n-queries", type=int, default=4096)
    ap.add_argument("--limit", type=float, default=600.0, help="seconds each step may take")
    ap.add_argument("--steps", default="pipeline,kernel,small")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hks_large_timing.json"))
    ap.add_argument("--step", default=None, help="(internal) run one step in this process and print its JSON")
    ap.add_argument("--time", type=float, default=None, help="(internal) the step's HKS time")
    a = ap.parse_args()
    if a.step:
        import torch
        assert torch.cuda.is_available(), "time_hks_large.py measures on the GPU; there is no CPU fallback"
        r = STEPS[a.step](a, a.time)
        r["device"] = torch.cuda.get_device_name(0)
        print("RESULT " + json.dumps(r), flush=True)
        return 0
    res = {"tool": "time_hks_large", "reps": a.reps, "n_queries": a.n_queries, "times": list(TIMES)}
    for t in TIMES:
        per = res.setdefault("t=%g" % t, {})
        for step in a.steps.split(","):
            cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--time", repr(t), "--reps", str(a.reps), "--n-queries", str(a.n_queries)]
            t0 = time.perf_counter()
            try:
                p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.limit)
            except subprocess.TimeoutExpired:
                print("# step %s at t=%g ran out of its %g s: stopping" % (step, t, a.limit), file=sys.stderr)
                return 124
            if p.returncode != 0:
                print("# step %s at t=%g ended with status %d: stopping" % (step, t, p.returncode), file=sys.stderr)
                return p.returncode if p.returncode > 0 else 1
            line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
            r = json.loads(line[len("RESULT "):])
            res["device"] = r.pop("device")
            per[step] = r
            print("# t=%g %s (%.1f s): %s" % (t, step, time.perf_counter() - t0, r), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

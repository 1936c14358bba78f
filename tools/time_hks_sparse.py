"""The sparse HKS tier (tlc_hks_sparse_batch) timed, with its baselines in the same run.  Steps, each in a child process of its own under
its own time limit (a step that fails or runs out of time ends the run; nothing is started after it):
  pubmed     the largest component of the PubMed-shaped graph at times 0.1 and 10: the entry alone (device events), and end to end through
             `ground_truth_packed(filt='hks', hks_sparse='device', pd_large='device')` (host clock around a synchronise) beside
             filt='degree' on the same route;
  wide       one random connected graph of 200 000 nodes and 300 000 edges at time 0.1, the entry alone;
  host       `hks_signature` (scipy's eigh) on sparse random graphs of growing size, one run each, up to the first that takes more than
             --host-limit seconds -- the host route this tier replaces above 4 096 nodes;
  crossover  sparse random graphs of 512, 1 024, 2 048 and 4 096 nodes at times 0.1 and 10 through tlc_hks_sparse_batch and through
             tlc_hks_large_batch (device events), their largest difference, and the smallest size from which the sparse tier is the
             faster one.
Device events are medians of --reps windows after a warm-up.  Prints ONE JSON line and writes it to --out.

  python tools/time_hks_sparse.py [--reps 5] [--limit 500] [--out profiles/hks_sparse_timing.json]
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


def random_connected(n, m, seed):
    """a random tree plus random edges up to about m: simple, connected, each edge once"""
    rs = np.random.RandomState(seed)
    tree = np.stack([(rs.random_sample(n - 1) * np.arange(1, n)).astype(np.int64), np.arange(1, n)], 1)
    more = rs.randint(n, size=(max(m - (n - 1), 0), 2)).astype(np.int64)
    more = np.stack([more.min(1), more.max(1)], 1)
    e = np.unique(np.concatenate([tree, more[more[:, 0] != more[:, 1]]]), axis=0)
    return e


def cuda_graph(n, e):
    import torch
    return (torch.tensor([0, n], dtype=torch.int64, device="cuda"), torch.tensor([0, len(e)], dtype=torch.int64, device="cuda"),
            torch.from_numpy(np.ascontiguousarray(e, dtype=np.int32)).cuda())


def entry_ms(n, e, t, reps, work_bytes=None):
    from tlc_gnn_amd import engine
    node_ptr, edge_ptr, edges = cuda_graph(n, e)
    run = lambda: engine.hks_sparse_batch(node_ptr, edge_ptr, edges, [0], [n], [len(e)], [t], total_nodes=n, work_bytes=work_bytes)
    ms = events_median_ms(run, reps)
    f, st = run()
    assert int(st[0]) == 0
    return ms, f[0]


def step_pubmed(a):
    import scipy.sparse as sp
    from scipy.sparse import csgraph
    from tlc_gnn_amd import engine, synth, _lib
    from tlc_gnn_amd.Knowledge_Distillation import data_utils_GC as kd, data_utils_LP as kd_lp
    n, edges, _, _, _ = synth.shaped_graph("PubMed")
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    e = np.unique(np.stack([e.min(1), e.max(1)], 1), axis=0)
    e = e[e[:, 0] != e[:, 1]]
    _, lab = csgraph.connected_components(sp.csr_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(n, n)), directed=False)
    keep = lab == np.bincount(lab).argmax()
    new = np.cumsum(keep) - 1
    ce = new[e[keep[e[:, 0]]]]
    cn = int(keep.sum())
    r = dict(nodes=cn, edges=int(len(ce)), max_degree=int(np.bincount(ce.reshape(-1)).max()), work_bytes=list(engine.hks_sparse_work_bytes([cn], [len(ce)])),
             work_cap=engine.HKS_SPARSE_WORK_CAP)
    packed = kd.pack_dataset([(int(n), np.concatenate([e, e[:, ::-1]]))])
    for t in TIMES:
        per = r.setdefault("t=%g" % t, {})
        per["terms"] = _lib.hks_sparse_terms(t)
        per["entry_ms"], _ = entry_ms(cn, ce, t, a.reps)
        per["multiply_adds"] = cn * per["terms"] * 2 * len(ce)
        run = lambda: kd.ground_truth_packed(*packed, filt='hks', hks_time=t, hks_sparse='device', pd_large='device')
        gt = run()
        assert bool(gt.ok[0]) and kd_lp.hks_sparse_device == 1 and kd_lp.hks_host_fallback == 0
        per["ground_truth_packed_hks_s"] = float(np.median([wall(run)[0] for _ in range(a.reps)]))
    run = lambda: kd.ground_truth_packed(*packed, filt='degree', pd_large='device')
    run()
    r["ground_truth_packed_degree_s"] = float(np.median([wall(run)[0] for _ in range(a.reps)]))
    return r


def step_wide(a):
    from tlc_gnn_amd import engine, _lib
    n = 200000
    e = random_connected(n, 300000, 9)
    ms, f = entry_ms(n, e, 0.1, a.reps)
    return dict(nodes=n, edges=int(len(e)), time=0.1, terms=_lib.hks_sparse_terms(0.1), entry_ms=ms, work_bytes=list(engine.hks_sparse_work_bytes([n], [len(e)])),
                work_cap=engine.HKS_SPARSE_WORK_CAP, finite=bool(f.isfinite().all()))


def step_host(a):
    from tlc_gnn_amd.Knowledge_Distillation.data_utils_LP import hks_signature
    r = {}
    for n in (1024, 2048, 4096, 8192, 12288, 16384):
        e = random_connected(n, 2 * n, 100 + n)
        t0 = time.perf_counter()
        hks_signature(n, e, 0.1)
        r["n%d_hks_signature_s" % n] = time.perf_counter() - t0
        r["largest_n"] = n
        if r["n%d_hks_signature_s" % n] > a.host_limit:
            break
    return r


def step_crossover(a):
    from tlc_gnn_amd import engine
    r = {}
    for t in TIMES:
        per, first = r.setdefault("t=%g" % t, {}), None
        for n in (512, 1024, 2048, 4096):
            e = random_connected(n, 2 * n, 100 + n)
            node_ptr, edge_ptr, edges = cuda_graph(n, e)
            ms_s, f = entry_ms(n, e, t, a.reps)
            run = lambda: engine.hks_large_batch(node_ptr, edge_ptr, edges, [0], [n], [t], total_nodes=n)
            ms_l = events_median_ms(run, a.reps)
            per["n%d" % n] = dict(edges=int(len(e)), sparse_ms=ms_s, large_ms=ms_l, abs_diff=float((run()[0][0] - f).abs().max()))
            if first is None and ms_s < ms_l:
                first = n
        per["sparse_faster_from_n"] = first
    return r


STEPS = {"pubmed": step_pubmed, "wide": step_wide, "host": step_host, "crossover": step_crossover}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=float, default=500.0, help="seconds each step may take")
    ap.add_argument("--host-limit", type=float, default=60.0, help="the host step stops after the first size that takes longer")
    ap.add_argument("--steps", default="pubmed,wide,crossover,host")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hks_sparse_timing.json"))
    ap.add_argument("--step", default=None, help="(internal) run one step in this process and print its JSON")
    a = ap.parse_args()
    if a.step:
        import torch
        assert torch.cuda.is_available(), "time_hks_sparse.py measures on the GPU; there is no CPU fallback"
        r = STEPS[a.step](a)
        r["device"] = torch.cuda.get_device_name(0)
        print("RESULT " + json.dumps(r), flush=True)
        return 0
    res = {"tool": "time_hks_sparse", "reps": a.reps, "times": list(TIMES)}
    for step in a.steps.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(a.reps), "--host-limit", str(a.host_limit)]
        t0 = time.perf_counter()
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print("# step %s ran out of its %g s: stopping" % (step, a.limit), file=sys.stderr)
            return 124
        if p.returncode != 0:
            print("# step %s ended with status %d: stopping" % (step, p.returncode), file=sys.stderr)
            return p.returncode if p.returncode > 0 else 1
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
        r = json.loads(line[len("RESULT "):])
        res["device"] = r.pop("device")
        res[step] = r
        print("# %s (%.1f s): %s" % (step, time.perf_counter() - t0, r), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""What the packed distance filtration costs (engine.dist_filtration / dist_filtration_vjp: tlc_dist_filtration and its VJP), against
the two routes a user has without it, in the same run.  Each step runs in a child process of its own under its own time limit (a step
that fails or runs out of time ends the run; nothing is started after it):
  hiv         the 41 127 HIV-shaped molecule graphs, root 0, weights U(0.5, 1.9): forward and VJP;
  vicinities  4 096 PubMed-shaped hop-2 node vicinities packed by NodeVicinities.batch: forward and VJP on the packed batch, against
              NodeVicinities.batch itself (tlc_vicinity_filtration: it also EXTRACTS the vicinities, so it is not the same work);
  lcc         the largest component of the PubMed-shaped graph, root 0, with the generic weights kappa + 1 and with tie-heavy weights
              (multiples of 0.1): forward and VJP, and the share of sources that took the per-source fallback search.
Host baseline in each step: scipy.sparse.csgraph.dijkstra per graph (wall clock; on the first --baseline-graphs graphs of the batches)
and a torch formulation of the VJP on the GPU: f = (path-incidence matrix built from scipy's predecessors) @ w / max, autograd through
it -- the build on the host (wall clock) and the forward + backward (device events) are reported apart.
Device events around each window of --calls calls, the median of --reps windows after a warm-up window, per call.
Prints ONE JSON line and writes it to --out.

  python tools/time_dist_filt.py [--reps 5] [--calls 3] [--limit 300] [--out profiles/dist_filt_timing.json]
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


def windows_median_ms(fn, reps, calls):
    """median over `reps` windows of (device time of `calls` calls) / calls, after one warm-up window"""
    import torch
    ms = []
    for w in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        if w:
            ms.append(e0.elapsed_time(e1) / calls)
    return float(np.median(ms)), [round(x, 4) for x in ms]


def fallbacks_of(work):
    from tlc_gnn_amd import _lib
    off = (-work.data_ptr()) % 256 + _lib.DIST_WORK_FALLBACKS_OFF
    return int(work[off:off + 8].cpu().numpy().view(np.uint64)[0])


def device_figures(a, no, eo, E, W, R, opts, tot_n):
    """forward and VJP of one packed batch, and the fallback share of one forward"""
    import torch
    from tlc_gnn_amd import engine
    need = engine.dist_filtration_work_bytes(no.numel() - 1, tot_n, E.shape[0])
    work = torch.empty(need + 255 + min(255 * (8 * tot_n + 256), 1 << 28), dtype=torch.uint8, device="cuda")
    f, st, P = engine.dist_filtration(no, eo, E, W, R, work=work, total_nodes=tot_n, **opts)
    r = dict(graphs=no.numel() - 1, nodes=tot_n, edges=int(E.shape[0]), fallback_sources=fallbacks_of(work))
    r["fallback_share"] = r["fallback_sources"] / max(tot_n, 1)
    g = torch.ones(tot_n, dtype=torch.float64, device="cuda")
    r["forward_ms"], r["forward_ms_all"] = windows_median_ms(
        lambda: engine.dist_filtration(no, eo, E, W, R, work=work, total_nodes=tot_n, check=False, **opts), a.reps, a.calls)
    r["vjp_ms"], r["vjp_ms_all"] = windows_median_ms(
        lambda: engine.dist_filtration_vjp(no, eo, E, W, R, P, g, total_nodes=tot_n, check=False, **opts), a.reps, a.calls)
    return r, f


def host_baseline(a, nptr, eptr, edges, w, f_dev, eps):
    """scipy's dijkstra from node 0 per graph on the first graphs of the batch, the path-incidence entries from its predecessors, and
    the torch forward + backward through them"""
    import torch
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import dijkstra
    B = min(a.baseline_graphs, len(nptr) - 1)
    t0 = time.perf_counter()
    preds = []
    for g in range(B):
        n, e, wg = int(nptr[g + 1] - nptr[g]), edges[eptr[g]:eptr[g + 1]], w[eptr[g]:eptr[g + 1]]
        A = csr_matrix((np.concatenate([wg, wg]), (np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]]))), shape=(n, n))
        d, p = dijkstra(A, directed=False, indices=0, return_predecessors=True)
        preds.append((d, p, A))
    t_dij = time.perf_counter() - t0
    t0 = time.perf_counter()
    rows, cols = [], []
    for g in range(B):
        d, p, A = preds[g]
        n, e = len(p), edges[eptr[g]:eptr[g + 1]]
        eid = csr_matrix((np.concatenate([np.arange(len(e)), np.arange(len(e))]) + 1,
                          (np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]]))), shape=(n, n))
        start, cur = np.arange(n), np.arange(n)
        for _ in range(n):
            live = p[cur] >= 0
            if not live.any():
                break
            start, cur = start[live], cur[live]
            rows.append(start + nptr[g])
            cols.append(np.asarray(eid[cur, p[cur]]).ravel() - 1 + eptr[g])
            cur = p[cur]
    t_build = time.perf_counter() - t0
    tot_n, tot_m = int(nptr[B]), int(eptr[B])
    row = torch.from_numpy(np.concatenate(rows).astype(np.int64)).cuda()
    col = torch.from_numpy(np.concatenate(cols).astype(np.int64)).cuda()
    owner = torch.from_numpy(np.repeat(np.arange(B), np.diff(nptr[:B + 1]))).cuda()
    wt = torch.from_numpy(w[:tot_m]).cuda().requires_grad_(True)

    def torch_route():
        wt.grad = None
        q = torch.zeros(tot_n, dtype=torch.float64, device="cuda").index_add(0, row, wt[col])
        mx = torch.zeros(B, dtype=torch.float64, device="cuda").scatter_reduce(0, owner, q, "amax")
        f = q / (mx[owner] + eps)
        f.sum().backward()
        return f

    fa = torch_route()
    r = dict(graphs=B, nodes=tot_n, scipy_dijkstra_host_ms=1e3 * t_dij, path_incidence_build_host_ms=1e3 * t_build, incidence_entries=int(row.numel()),
             worst_abs_diff_to_device=float((fa.detach() - f_dev[:tot_n]).abs().max()))
    r["torch_fwd_bwd_ms"], r["torch_fwd_bwd_ms_all"] = windows_median_ms(torch_route, a.reps, a.calls)
    return r


def one_root(B):
    import torch
    return torch.stack([torch.zeros(B, dtype=torch.int32, device="cuda"), torch.full((B,), -1, dtype=torch.int32, device="cuda")], 1).contiguous()


OPTS = dict(descriptor="sum", norm="max_eps", unreachable_100=True)


def step_hiv(a):
    import torch
    from tlc_gnn_amd import synth
    edges, _, nptr, eptr = synth.hiv_shaped_molecules(41127)
    w = np.random.RandomState(1).uniform(0.5, 1.9, len(edges))
    no, eo, E, W = (torch.from_numpy(x).cuda() for x in (nptr, eptr, edges, w))
    r, f = device_figures(a, no, eo, E, W, one_root(len(nptr) - 1), OPTS, int(nptr[-1]))
    r["baseline"] = host_baseline(a, nptr, eptr, edges.astype(np.int64), w, f, 1e-10)
    return r


def step_vicinities(a):
    import torch
    from tlc_gnn_amd import synth
    from tlc_gnn_amd.Knowledge_Distillation import data_utils_NC as kd_nc
    n, edges, kappa, _, _ = synth.shaped_graph("PubMed")
    curv = np.concatenate([np.concatenate([edges, edges[:, ::-1]]).astype(np.float64), np.concatenate([kappa, kappa])[:, None]], axis=1)
    vic = kd_nc.NodeVicinities(edges, curv)
    nodes = np.random.RandomState(0).permutation(np.unique(edges))[:a.n_queries]
    b = vic.batch(nodes, 2)
    no, eo, ids, E = (b[k].cpu().numpy() for k in ("node_ptr", "edge_ptr", "ids", "edges"))
    key = edges.min(1).astype(np.int64) * n + edges.max(1)
    order = np.argsort(key)
    owner = np.repeat(np.arange(len(nodes)), np.diff(eo))
    ga, gb = ids[no[owner] + E[:, 0]], ids[no[owner] + E[:, 1]]
    w = kappa[order[np.searchsorted(key[order], np.minimum(ga, gb) * n + np.maximum(ga, gb))]] + 1.0
    roots = np.stack([[np.searchsorted(ids[no[k]:no[k + 1]], nodes[k]) for k in range(len(nodes))], np.full(len(nodes), -1)], 1).astype(np.int32)
    r, f = device_figures(a, b["node_ptr"], b["edge_ptr"], b["edges"].contiguous(), torch.from_numpy(w).cuda(), torch.from_numpy(roots).cuda(),
                          dict(OPTS, include_roots=True), int(no[-1]))
    sizes = np.diff(no)
    r.update(n_max=int(sizes.max()), n_median=float(np.median(sizes)), equal_to_vicinity_pipeline=bool(torch.equal(f, b["f"])))
    r["vicinity_batch_extract_and_filtration_ms"], r["vicinity_batch_extract_and_filtration_ms_all"] = windows_median_ms(
        lambda: vic.batch(nodes, 2), a.reps, 1)
    return r


def step_lcc(a):
    import torch
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    from tlc_gnn_amd import synth
    n, edges, kappa, _, _ = synth.shaped_graph("PubMed")
    _, lab = connected_components(csr_matrix((np.ones(len(edges)), (edges[:, 0], edges[:, 1])), shape=(n, n)), directed=False)
    big = np.argmax(np.bincount(lab))
    new = np.cumsum(lab == big) - 1
    keep = lab[edges[:, 0]] == big
    e = new[edges[keep]].astype(np.int32)
    k = int((lab == big).sum())
    nptr, eptr = np.array([0, k], np.int64), np.array([0, len(e)], np.int64)
    r = dict(nodes=k, edges=int(len(e)))
    for name, w in (("generic", kappa[keep] + 1.0), ("ties", np.round((kappa[keep] + 1.0) * 10.0) * 0.1)):
        no, eo, E, W = (torch.from_numpy(x).cuda() for x in (nptr, eptr, e, np.ascontiguousarray(w)))
        r[name], f = device_figures(a, no, eo, E, W, one_root(1), OPTS, k)
        r[name]["baseline"] = host_baseline(a, nptr, eptr, e.astype(np.int64), w, f, 1e-10)
    return r


STEPS = {"hiv": step_hiv, "vicinities": step_vicinities, "lcc": step_lcc}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="windows per figure")
    ap.add_argument("--calls", type=int, default=3, help="calls per window")
    ap.add_argument("--n-queries", type=int, default=4096)
    ap.add_argument("--baseline-graphs", type=int, default=4096)
    ap.add_argument("--limit", type=float, default=300.0, help="seconds each step may take")
    ap.add_argument("--steps", default="hiv,vicinities,lcc")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dist_filt_timing.json"))
    ap.add_argument("--step", default=None, help="(internal) run one step in this process and print its JSON")
    a = ap.parse_args()
    if a.step:
        import torch
        assert torch.cuda.is_available(), "time_dist_filt.py measures on the GPU; there is no CPU fallback"
        r = STEPS[a.step](a)
        r["device"] = torch.cuda.get_device_name(0)
        print("RESULT " + json.dumps(r), flush=True)
        return 0
    res = {"tool": "time_dist_filt", "reps": a.reps, "calls_per_window": a.calls}
    for step in a.steps.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(a.reps), "--calls", str(a.calls),
               "--n-queries", str(a.n_queries), "--baseline-graphs", str(a.baseline_graphs)]
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

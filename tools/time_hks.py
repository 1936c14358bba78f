"""The HKS filtration, host backend (scipy's eigh per graph) against device backend (tlc_hks_batch), end to end on three batches:
  hiv     the 41 127 HIV-shaped molecule graphs of synth.hiv_shaped_molecules(), times 0.1 and 10:
          data_utils_GC.compute_persistence_image_batch(filt='hks'), diagrams and images included;
  photo   the edge-centred vicinities of 4 096 Photo-shaped positive pairs, hop 1: Vicinities.batch(filt='hks'), extraction included;
  pubmed  the node-centred vicinities of 4 096 PubMed-shaped nodes, hop 2: NodeVicinities.batch(filt='hks'), extraction included.
Prints ONE JSON line: per batch the size histogram (share of graphs per tier and above TLC_HKS_NMAX), the host time (one run: it is
a Python loop of up to a minute), the device time (median of --reps runs after a warm-up; host clock around work that ends in a
synchronise), their ratio, the graphs that fell back to the host, and the median time of tlc_hks_batch alone (device events).

  python tools/time_hks.py [--batches hiv,photo,pubmed] [--reps 5] [--n-graphs 41127] [--n-queries 4096] [--out profiles/hks_timing.json]
  python tools/time_hks.py --kernels-only      # tlc_hks_batch alone on the three batches: run it under rocprofv3 --kernel-trace --stats
  python tools/time_hks.py --sizes-only        # the size histograms alone (how many vicinities lie above the cap decides how long the rest takes)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def size_histogram(node_ptr):
    from tlc_gnn_amd import _lib
    n = np.diff(np.asarray(node_ptr))
    n = n[n > 0]
    cuts = [("n<=32", 0, 32), ("n<=64", 32, 64), ("n<=%d" % _lib.HKS_LDS_NMAX, 64, _lib.HKS_LDS_NMAX),
            ("n<=%d" % _lib.HKS_NMAX, _lib.HKS_LDS_NMAX, _lib.HKS_NMAX), ("above_cap", _lib.HKS_NMAX, 1 << 62)]
    h = {name: round(float(((n > lo) & (n <= hi)).mean()), 5) for name, lo, hi in cuts} if len(n) else {}
    h.update(graphs=int(len(n)), n_median=float(np.median(n)) if len(n) else 0.0, n_max=int(n.max()) if len(n) else 0)
    return h


def wall(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def kernel_median_ms(node_ptr, edge_ptr, edges, times, reps):
    import torch
    from tlc_gnn_amd import engine
    tot = int(node_ptr[-1])
    engine.hks_batch(node_ptr, edge_ptr, edges, times, total_nodes=tot)
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        engine.hks_batch(node_ptr, edge_ptr, edges, times, total_nodes=tot)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


def packed_hiv(n_graphs):
    import torch
    from tlc_gnn_amd import synth
    edges, _, node_offs, edge_offs = synth.hiv_shaped_molecules(n_graphs)
    graphs = [(int(node_offs[k + 1] - node_offs[k]), edges[edge_offs[k]:edge_offs[k + 1]].astype(np.int64)) for k in range(n_graphs)]
    packed = (torch.from_numpy(node_offs).cuda(), torch.from_numpy(edge_offs).cuda(), torch.from_numpy(edges).cuda())
    return graphs, packed


def vicinity_setup(which, n_queries):
    from tlc_gnn_amd import synth
    from tlc_gnn_amd.Knowledge_Distillation import data_utils_LP as kd_lp, data_utils_NC as kd_nc
    rs = np.random.RandomState(0)
    if which == "photo":
        _, edges, _, _, _ = synth.shaped_graph("Photo")
        return kd_lp.Vicinities(edges, None), edges[rs.permutation(len(edges))[:n_queries]], 1
    n, edges, _, _, _ = synth.shaped_graph("PubMed")
    return kd_nc.NodeVicinities(edges, None), rs.permutation(np.unique(edges))[:n_queries], 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="hiv,photo,pubmed")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n-graphs", type=int, default=41127)
    ap.add_argument("--n-queries", type=int, default=4096)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--sizes-only", action="store_true")
    ap.add_argument("--skip-host", action="store_true", help="device side only (the host loop is the long part)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from tlc_gnn_amd.Knowledge_Distillation import data_utils_LP as kd_lp, data_utils_GC as kd_gc
    assert torch.cuda.is_available(), "time_hks.py measures on the GPU; there is no CPU fallback"
    res = {"tool": "time_hks", "device": torch.cuda.get_device_name(0), "reps": a.reps, "times": [0.1, 10.0]}
    for which in a.batches.split(","):
        r = {}
        if which == "hiv":
            graphs, packed = packed_hiv(a.n_graphs)
            run = lambda backend: [kd_gc.compute_persistence_image_batch(graphs, filt='hks', hks_time=t, hks_backend=backend) for t in (0.1, 10.0)]
            times = [0.1, 10.0]
        else:
            vic, query, hop = vicinity_setup(which, a.n_queries)
            run = lambda backend: vic.batch(query, hop, filt='hks', hks_time=0.1, hks_backend=backend)
            b = vic.batch(query, hop, filt='degree')
            packed = (b["node_ptr"], b["edge_ptr"], b["edges"].contiguous())
            times = [0.1]
        r["sizes"] = size_histogram(packed[0].cpu().numpy())
        if a.sizes_only:
            res[which] = r
            continue
        r["hks_batch_alone_ms"] = kernel_median_ms(*packed, times, a.reps)
        print("# %s: sizes %s, tlc_hks_batch alone %.3f ms" % (which, r["sizes"], r["hks_batch_alone_ms"]), file=sys.stderr, flush=True)
        if not a.kernels_only:
            run('device')                                                       # warm-up
            dev = []
            for _ in range(a.reps):
                dev.append(wall(lambda: run('device'))[0])
                r["host_fallback_graphs"] = int(kd_lp.hks_host_fallback)
            r["device_s"] = float(np.median(dev))
            r["device_s_all"] = [round(x, 4) for x in dev]
            print("# %s: device %.3f s" % (which, r["device_s"]), file=sys.stderr, flush=True)
            if not a.skip_host:
                r["host_s"] = wall(lambda: run('host'))[0]
                r["host_over_device"] = r["host_s"] / r["device_s"]
                print("# %s: host %.3f s" % (which, r["host_s"]), file=sys.stderr, flush=True)
        res[which] = r
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

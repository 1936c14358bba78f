"""The degree / centrality / clustering filtrations, host backend (`structural_filtration`: numpy + scipy on copies of offsets and edges)
against device backend (tlc_struct_batch on the extracted tensors), end to end on three batches, filt 'clustering' and 'centrality':
  photo   the edge-centred vicinities of 4 096 Photo-shaped positive pairs, hop 1: Vicinities.batch(filt=...), extraction included;
  pubmed  the node-centred vicinities of 4 096 PubMed-shaped nodes, hop 2: NodeVicinities.batch(filt=...), extraction included;
  hiv     the 41 127 HIV-shaped molecule graphs of synth.hiv_shaped_molecules(): data_utils_GC.compute_persistence_image_batch, diagrams
          and images included.  The host backend refuses 'centrality' and 'clustering' there, so its run is what a caller does today:
          `structural_filtration` on the packed list, then the batch call with `filtrations=`.
Prints ONE JSON line: per batch the size histogram (share of graphs per tier), per filtration the host and device times (median of --reps
runs each after a warm-up, same process; host clock around work that ends in a synchronise), their ratio, and the median time of
tlc_struct_batch alone (device events).

  python tools/time_struct.py [--batches photo,pubmed,hiv] [--reps 5] [--n-graphs 41127] [--n-queries 4096] [--out profiles/struct_timing.json]
  python tools/time_struct.py --kernels-only     # tlc_struct_batch alone on the three batches: run it under rocprofv3 --kernel-trace --stats
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FILTS = ("clustering", "centrality")


def size_histogram(node_ptr):
    from tlc_gnn_amd import _lib
    n = np.diff(np.asarray(node_ptr))
    n = n[n > 0]
    cuts = [("n<=%d" % _lib.STRUCT_WAVE_NMAX, 0, _lib.STRUCT_WAVE_NMAX), ("n<=%d" % _lib.STRUCT_LDS_SMALL_NMAX, _lib.STRUCT_WAVE_NMAX, _lib.STRUCT_LDS_SMALL_NMAX),
            ("n<=%d" % _lib.STRUCT_LDS_NMAX, _lib.STRUCT_LDS_SMALL_NMAX, _lib.STRUCT_LDS_NMAX), ("larger", _lib.STRUCT_LDS_NMAX, 1 << 62)]
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


def kernel_median_ms(node_ptr, edge_ptr, edges, kind, reps):
    import torch
    from tlc_gnn_amd import engine
    tot = int(node_ptr[-1])
    engine.struct_batch(node_ptr, edge_ptr, edges, kind, total_nodes=tot)
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        engine.struct_batch(node_ptr, edge_ptr, edges, kind, total_nodes=tot)
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
    return graphs, packed, (node_offs, edge_offs, edges)


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
    ap.add_argument("--batches", default="photo,pubmed,hiv")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n-graphs", type=int, default=41127)
    ap.add_argument("--n-queries", type=int, default=4096)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from tlc_gnn_amd.Knowledge_Distillation import data_utils_LP as kd_lp, data_utils_GC as kd_gc
    assert torch.cuda.is_available(), "time_struct.py measures on the GPU; there is no CPU fallback"
    res = {"tool": "time_struct", "device": torch.cuda.get_device_name(0), "reps": a.reps, "filts": list(FILTS)}
    for which in a.batches.split(","):
        r = {}
        if which == "hiv":
            graphs, packed, host_packed = packed_hiv(a.n_graphs)

            def run(backend, filt):
                if backend == 'device':
                    return kd_gc.compute_persistence_image_batch(graphs, filt=filt, struct_backend='device')
                f = kd_lp.structural_filtration(filt, *host_packed)
                return kd_gc.compute_persistence_image_batch(graphs, filt=filt, filtrations=[f[host_packed[0][k]:host_packed[0][k + 1]] for k in range(len(graphs))])
        else:
            vic, query, hop = vicinity_setup(which, a.n_queries)
            run = lambda backend, filt: vic.batch(query, hop, filt=filt, struct_backend=backend)
            b = vic.batch(query, hop, filt='ricci')
            packed = (b["node_ptr"], b["edge_ptr"], b["edges"].contiguous())
        r["sizes"] = size_histogram(packed[0].cpu().numpy())
        for filt in FILTS:
            q = {"struct_batch_alone_ms": kernel_median_ms(*packed, filt, a.reps)}
            print("# %s %s: sizes %s, tlc_struct_batch alone %.3f ms" % (which, filt, r["sizes"], q["struct_batch_alone_ms"]), file=sys.stderr, flush=True)
            if not a.kernels_only:
                for backend in ('device', 'host'):
                    run(backend, filt)                                          # warm-up
                    ts = [wall(lambda: run(backend, filt))[0] for _ in range(a.reps)]
                    q[backend + "_s"] = float(np.median(ts))
                    q[backend + "_s_all"] = [round(x, 4) for x in ts]
                q["host_over_device"] = q["host_s"] / q["device_s"]
                print("# %s %s: device %.4f s, host %.4f s, host / device %.2f" % (which, filt, q["device_s"], q["host_s"], q["host_over_device"]),
                      file=sys.stderr, flush=True)
            r[filt] = q
        res[which] = r
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

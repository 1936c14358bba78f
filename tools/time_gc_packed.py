"""The packed graph-classification ground truth (`data_utils_GC.ground_truth_packed` on `tlc_graph_components`) against today's route
(`largest_component` per graph, then `compute_persistence_image_batch` with the device backends), everything in one run:
  hiv     the 41 127 HIV-shaped molecule graphs of synth.hiv_shaped_molecules(), edges handed over RAW (both orientations):
          filt 'degree' and filt 'hks' at time 10, end to end; today's route split into its scipy loop and its batch call; and
          tlc_graph_components alone between device events;
  mid     4 096 random graphs of 65 .. 1 024 nodes, raw: the WIDE class as a batch -- tlc_graph_components alone against the scipy loop
          (what an LDS class for these sizes would have to beat);
  pubmed  the PubMed-shaped graph, raw, filt 'degree', pd_large='device' on both routes.
Medians of --reps runs each after a warm-up, same process; a host clock around work that ends in a synchronise, device events for the
entry alone.  The outputs of the two routes are compared (d0, d1, f, edge_index, the images: equal) before anything is timed.
Prints ONE JSON line.

  python tools/time_gc_packed.py [--parts hiv,mid,pubmed] [--reps 5] [--n-graphs 41127] [--out profiles/gc_packed_timing.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def wall(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def med(ts):
    return {"s": float(np.median(ts)), "s_all": [round(float(x), 4) for x in ts]}


def both_orientations(graphs):
    return [(n, np.concatenate([e, e[:, ::-1]])) for n, e in graphs]


def hiv_graphs(n_graphs):
    from tlc_gnn_amd import synth
    edges, _, node_offs, edge_offs = synth.hiv_shaped_molecules(n_graphs)
    return both_orientations([(int(node_offs[k + 1] - node_offs[k]), edges[edge_offs[k]:edge_offs[k + 1]].astype(np.int64)) for k in range(n_graphs)])


def mid_graphs(n_graphs=4096, seed=7):
    rs = np.random.RandomState(seed)
    out = []
    for n in rs.randint(65, 1025, size=n_graphs):
        par = (rs.random_sample(n - 1) * np.arange(1, n)).astype(np.int64)
        e = np.concatenate([np.stack([par, np.arange(1, n)], 1)[rs.random_sample(n - 1) < 0.9], rs.randint(0, n, size=(n // 4, 2))])
        out.append((int(n), rs.permutation(n)[e]))
    return both_orientations(out)


def same(a, b):
    if len(a) != len(b):
        return False
    for x, y in zip(a, b):
        if len(x) != len(y) or (len(x) == 2) != (len(y) == 2):
            return False
        if len(x) > 2 and not (all(np.array_equal(np.asarray(x[j]), np.asarray(y[j])) for j in (0, 1, 2, 5, 6)) and x[3] == y[3]
                               and np.array_equal(x[4].numpy(), y[4].numpy())):
            return False
    return True


def entry_alone_ms(packed, reps):
    """tlc_graph_components between device events (its workspace and outputs allocated outside the window)"""
    import torch
    from tlc_gnn_amd import engine
    B, tot_n, tot_m = packed[0].numel() - 1, int(packed[0][-1]), int(packed[2].shape[0])
    max_n = int((packed[0][1:] - packed[0][:-1]).max())
    work = torch.empty(engine.graph_components_work_bytes(B, tot_n, tot_m), dtype=torch.uint8, device="cuda")
    run = lambda: engine.graph_components(*packed, work=work, total_nodes=tot_n, max_nodes=max_n)
    run()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"ms": float(np.median(ms)), "ms_all": [round(x, 4) for x in ms]}


def scipy_loop(graphs):
    from tlc_gnn_amd.Knowledge_Distillation.data_utils_GC import largest_component
    return [largest_component(n, e) for n, e in graphs]


def routes(graphs, packed, reps, **kw):
    """the packed route and today's route end to end, today's split into its two parts; checks that they agree first"""
    from tlc_gnn_amd.Knowledge_Distillation import data_utils_GC as kd
    new = lambda: kd.ground_truth_packed(*packed, component='largest', **kw)
    old_batch = lambda comps: kd.compute_persistence_image_batch(comps, struct_backend='device', hks_backend='device', **kw)
    ref = old_batch(scipy_loop(graphs))                                   # warm-up of both, and the check
    got = new()
    q = {"equal": same(got.tuples(), ref), "graphs": len(graphs), "with_ground_truth": int(got.ok.sum())}
    t_new, t_loop, t_batch, t_tuples = [], [], [], []
    for _ in range(reps):
        t, gt = wall(new)
        t_new.append(t)
        t_tuples.append(wall(gt.tuples)[0])
        t, comps = wall(lambda: scipy_loop(graphs))
        t_loop.append(t)
        t_batch.append(wall(lambda: old_batch(comps))[0])
    q.update(packed=med(t_new), packed_tuples=med(t_tuples), today_scipy_loop=med(t_loop), today_batch_call=med(t_batch),
             today=med([a + b for a, b in zip(t_loop, t_batch)]))
    q["today_over_packed"] = q["today"]["s"] / q["packed"]["s"]
    q["today_batch_call_over_packed"] = q["today_batch_call"]["s"] / q["packed"]["s"]
    return q


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="hiv,mid,pubmed")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n-graphs", type=int, default=41127)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from tlc_gnn_amd import synth
    from tlc_gnn_amd.Knowledge_Distillation import data_utils_GC as kd
    assert torch.cuda.is_available(), "time_gc_packed.py measures on the GPU; there is no CPU fallback"
    res = {"tool": "time_gc_packed", "device": torch.cuda.get_device_name(0), "reps": a.reps}
    say = lambda *x: print("#", *x, file=sys.stderr, flush=True)
    for part in a.parts.split(","):
        r = {}
        if part == "hiv":
            graphs = hiv_graphs(a.n_graphs)
            packed = kd.pack_dataset(graphs)
            r["pack_dataset"] = med([wall(lambda: kd.pack_dataset(graphs))[0] for _ in range(a.reps)])
            r["graph_components_alone"] = entry_alone_ms(packed, a.reps)
            say(part, "tlc_graph_components alone", r["graph_components_alone"])
            for name, kw in (("degree", dict(filt='degree')), ("hks10", dict(filt='hks', hks_time=10))):
                r[name] = routes(graphs, packed, a.reps, **kw)
                say(part, name, r[name])
        elif part == "mid":
            graphs = mid_graphs()
            packed = kd.pack_dataset(graphs)
            r["graphs"], r["nodes"], r["raw_edges"] = len(graphs), int(packed[0][-1]), int(packed[2].shape[0])
            r["graph_components_alone"] = entry_alone_ms(packed, a.reps)
            r["scipy_loop"] = med([wall(lambda: scipy_loop(graphs))[0] for _ in range(a.reps)])
            r["ms_per_graph"] = r["graph_components_alone"]["ms"] / len(graphs)
            say(part, r)
        elif part == "pubmed":
            n, edges, _, _, _ = synth.shaped_graph("PubMed")
            graphs = both_orientations([(int(n), edges.astype(np.int64))])
            packed = kd.pack_dataset(graphs)
            r["nodes"], r["raw_edges"] = int(n), int(packed[2].shape[0])
            r["graph_components_alone"] = entry_alone_ms(packed, a.reps)
            r["degree"] = routes(graphs, packed, a.reps, filt='degree', pd_large='device')
            say(part, r)
        else:
            raise SystemExit("unknown part %r" % part)
        res[part] = r
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

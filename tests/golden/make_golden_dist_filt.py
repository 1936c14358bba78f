#!/usr/bin/env python3
"""Generate tests/golden/dist_filt_ref.npz by IMPORTING the reference (build container only; the shadow package and the stubs of
make_golden.py).  Run from the repo root:  python tests/golden/make_golden_dist_filt.py

About 60 connected graphs of 2 .. 200 nodes with weights kappa + 1 -- generic (U(0.5, 1.9)), tie-heavy (multiples of 0.1), an even
cycle and a grid with equal weights -- and for each
  one root:   Knowledge_Distillation/data_utils_NC.py ricci_filtration(g, r0, hop, curv).build_fv(weight_graph=True, norm=True)  -> f_one
  two roots:  sg2dgm/riccidist2dgm.py filtration(g, r0, r1, hop, curv).build_fv(weight_graph=True, norm=True)   -> f_sum, f_min, f_max
              (a ZeroDivisionError -- the graph is its two roots -- is recorded as status 3 and NaN values).
Only data is written: the packed inputs (node_offs, edge_offs, edges, w, roots) and the expected values."""
import os
import sys

import networkx as nx
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden  # noqa: E402
import dist_filt_cases as dc  # noqa: E402


def main():
    mods = make_golden.import_reference()
    r2d, nc = mods["r2d"], mods["kd_nc"]
    rng = np.random.default_rng(20260)
    graphs = []
    sizes = [2, 3, 4, 5, 7, 9, 12, 16, 20, 25, 31, 40, 50, 63, 64, 65, 80, 100, 130, 160, 200]
    for kind in ("generic", "ties"):
        for n in sizes:
            m = min(n * (n - 1) // 2, n - 1 + int(rng.integers(0, n + 1)))
            e = dc.random_connected(rng, n, m)
            graphs.append((n, e, kind))
    for n in sizes[::3]:                                      # denser ones: more alternative paths
        e = dc.random_connected(rng, n, min(n * (n - 1) // 2, 3 * n))
        graphs.append((n, e, "ties"))
    graphs += [(10, dc.cycle(10), "unit"), (64, dc.cycle(64), "unit"), (42, dc.grid(6, 7), "unit"), (36, dc.grid(6, 6), "ties"),
               (30, dc.star(30), "generic"), (33, dc.path(33), "generic")]
    packed, out = [], dict(f_one=[], f_sum=[], f_min=[], f_max=[], st_one=[], st_two=[])
    for n, e, kind in graphs:
        m = len(e)
        w = dc.generic_weights(rng, m) if kind == "generic" else (dc.tie_weights(rng, m) if kind == "ties" else np.ones(m))
        kappa = w - 1.0
        w = kappa + 1.0                                       # the weight the reference sums is kappa + 1, whatever w - 1 rounded to
        r0, r1 = (int(v) for v in rng.choice(n, 2, replace=False))
        g = nx.Graph()
        g.add_nodes_from(range(n))
        curv = {}
        for (a, b), k, wt in zip(e.tolist(), kappa.tolist(), w.tolist()):
            g.add_edge(a, b, weight=wt)
            curv[(a, b)] = k
            curv[(b, a)] = k
        one = nc.ricci_filtration(g.copy(), r0, 2, curv).build_fv(weight_graph=True, norm=True)
        out["f_one"].append(np.array([one.nodes[x]["sum"] for x in range(n)], np.float64))
        out["st_one"].append(0)
        try:
            two = r2d.filtration(g.copy(), r0, r1, 2, curv).build_fv(weight_graph=True, norm=True)
            for d in ("sum", "min", "max"):
                out["f_" + d].append(np.array([two.nodes[x][d] for x in range(n)], np.float64))
            out["st_two"].append(0)
        except ZeroDivisionError:
            for d in ("sum", "min", "max"):
                out["f_" + d].append(np.full(n, np.nan))
            out["st_two"].append(3)
        packed.append((n, e, w, r0, r1))
    no, eo, E, W, R = dc.pack(packed)
    path = os.path.join(HERE, "dist_filt_ref.npz")
    np.savez_compressed(path, node_offs=no, edge_offs=eo, edges=E, w=W, roots=R,
                        st_one=np.array(out["st_one"], np.uint8), st_two=np.array(out["st_two"], np.uint8),
                        **{k: np.concatenate(out[k]) for k in ("f_one", "f_sum", "f_min", "f_max")})
    print("wrote %s: %d graphs, %d nodes, %d edges, %d bytes" % (path, len(graphs), no[-1], eo[-1], os.path.getsize(path)))


if __name__ == "__main__":
    main()

"""The device-wide persistence tier (tlc_pd_wide) against tlc_pd_from_filtration's one-workgroup HUGE tier and the C oracle, in one
process, each figure the median of --reps runs after a warm-up (host clock around a synchronised call; all runs kept):
  pubmed   the largest component of the PubMed-shaped synthetic graph (synth.shaped_graph), degree filtration and a random one:
           HUGE tier, wide tier, oracle (one CPU thread);
  sweep    random connected graphs (a random recursive tree plus n / 2 chords, random values) from 2 049 to 65 535 nodes: both tiers
           and the oracle -- the crossover, if there is one;
  big      200 000 nodes and 300 000 edges: wide tier and oracle (the HUGE tier refuses it), checked against the oracle here.
Each wide figure comes with the same call under TLC_NO_EXT1 (everything but the cycle swap), so the swap's share is their difference.
Every wide result is compared with the oracle's (counts, sorted points).  Prints ONE JSON line and writes it to --out.

  python tools/time_pd_wide.py [--reps 5] [--out profiles/pd_wide_timing.json] [--no-huge-above N]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def rrt(n, chords, seed):
    rs = np.random.RandomState(seed)
    par = (rs.random_sample(n - 1) * np.arange(1, n)).astype(np.int64)
    a, b = rs.randint(0, n, size=2 * chords), rs.randint(0, n, size=2 * chords)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    key = np.unique((lo * n + hi)[lo != hi])
    key = np.setdiff1d(key, par * n + np.arange(1, n))
    key = key[rs.permutation(len(key))[:chords]]
    return np.concatenate([np.stack([par, np.arange(1, n)], 1), np.stack([key // n, key % n], 1)]).astype(np.int32)


def largest_component(n, edges):
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    e = np.unique(np.sort(edges[edges[:, 0] != edges[:, 1]], 1), axis=0)
    a = sp.coo_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(n, n))
    _, lab = connected_components(a, directed=False)
    keep = lab == np.bincount(lab).argmax()
    new = np.cumsum(keep) - 1
    e = e[keep[e[:, 0]]]
    return int(keep.sum()), new[e].astype(np.int32)


def degree_f(n, e):
    deg = np.bincount(e.reshape(-1), minlength=n).astype(np.float64)
    return deg / (deg.max() + 1e-10)


def timed(fn, reps):
    import torch
    fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return dict(median_s=float(np.median(out)), all_s=[round(x, 5) for x in out])


def sorted_pts(p):
    p = np.asarray(p).reshape(-1, 2)
    return p[np.lexsort((p[:, 1], p[:, 0]))]


def measure(n, e, f, reps, huge=True):
    import torch
    from oracle import oracle
    from tlc_gnn_amd import engine, _lib
    no, eo = np.array([0, n], dtype=np.int64), np.array([0, len(e)], dtype=np.int64)
    d = [torch.from_numpy(x).cuda() for x in (no, eo, np.ascontiguousarray(e, dtype=np.int32), np.ascontiguousarray(f, dtype=np.float64))]
    flags = _lib.KEEP_ZERO_PERS
    r = dict(n=int(n), m=int(len(e)))
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        ref = oracle.pd_from_filtration(no, eo, e, f, flags)
        t.append(time.perf_counter() - t0)
    r["oracle"] = dict(median_s=float(np.median(t)), all_s=[round(x, 5) for x in t])
    r["n_pos"] = int((ref["edge_rank"] >= 0).sum())
    work = torch.empty(engine.pd_wide_work_bytes([n], [len(e)]), dtype=torch.uint8, device="cuda")
    r["work_bytes"] = int(work.numel())
    r["wide"] = timed(lambda: engine.pd_wide(*d, flags, work=work), reps)
    # the stages before the cycle swap alone (keys, sorts, the two forests, the two serial passes): TLC_NO_EXT1 ends there
    r["wide_no_ext1"] = timed(lambda: engine.pd_wide(*d, flags | _lib.NO_EXT1, work=work), reps)
    r["swap_share"] = 1.0 - r["wide_no_ext1"]["median_s"] / r["wide"]["median_s"]
    got = engine.pd_wide(*d, flags, work=work)
    r["stats"] = dict(zip(("levels", "boruvka_rounds", "launches", "fallback", "status"), (int(v) for v in got["stats"])))
    c = got["counts"][0].cpu().numpy()
    same = bool(np.array_equal(c, ref["counts"][0]))
    for key, k in (("up", c[0]), ("down", c[1]), ("one", c[2])):
        same = same and np.array_equal(sorted_pts(got[key][:k].cpu().numpy()), sorted_pts(ref[key][:k]))
    r["wide_matches_oracle"] = same
    if huge:
        r["huge_tier"] = timed(lambda: engine.pd_from_filtration(*d, flags, want_rank=False), reps)
        r["huge_over_wide"] = r["huge_tier"]["median_s"] / r["wide"]["median_s"]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-huge-above", type=int, default=65535, help="skip the one-workgroup tier above this many nodes")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pd_wide_timing.json"))
    a = ap.parse_args()
    import torch
    from tlc_gnn_amd import synth
    assert torch.cuda.is_available(), "time_pd_wide.py measures on the GPU; there is no CPU fallback"
    res = {"tool": "time_pd_wide", "reps": a.reps, "device": torch.cuda.get_device_name(0), "flags": "TLC_KEEP_ZERO_PERS"}
    def dump():
        line = json.dumps(res)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return line

    def note(key, r):
        print("# %s: %s" % (key, r), file=sys.stderr, flush=True)
        dump()
    n0, e0 = synth.shaped_graph("PubMed")[:2]
    n, e = largest_component(n0, np.asarray(e0))
    res["pubmed_degree"] = measure(n, e, degree_f(n, e), a.reps)
    note("pubmed degree", res["pubmed_degree"])
    res["pubmed_random"] = measure(n, e, np.random.RandomState(1).rand(n), a.reps)
    note("pubmed random", res["pubmed_random"])
    g = rrt(200000, 100001, seed=200000)
    res["big"] = measure(200000, g, np.random.RandomState(2).rand(200000), a.reps, huge=False)
    note("big", res["big"])
    res["sweep"] = []
    for k in (2049, 4096, 8192, 16384, 32768, 65535):
        g = rrt(k, k // 2, seed=k)
        res["sweep"].append(measure(k, g, np.random.RandomState(k + 1).rand(k), a.reps, huge=k <= a.no_huge_above))
        note("sweep", res["sweep"][-1])
    ok = all(r["wide_matches_oracle"] for r in [res["pubmed_degree"], res["pubmed_random"], res["big"]] + res["sweep"])
    res["all_match_oracle"] = ok
    print(dump())
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

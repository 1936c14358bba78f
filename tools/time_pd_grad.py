"""What the gradient of the exact extended persistence costs (csrc/pd_grad.hip), next to the forward it differentiates and to the
same vertices and gradient from torch ops, in one process.  Each figure is the median of --reps windows after a warm-up; a window is
--inner calls between two device events (hipEvent through torch.cuda.Event) with no synchronisation of the tool's inside it, and the
figure is the window over --inner.  (tlc_pd_point_vertices and tlc_pd_filtration_grad read the offsets back themselves: that wait is
part of their price and is inside their figures; `offsets_readback` times the same two copies and the wait alone, through torch.)
  hiv      the 41 127 HIV-shaped molecule graphs of synth.hiv_shaped_molecules() with random distinct values, TLC_KEEP_ZERO_PERS:
           tlc_pd_from_filtration alone, tlc_pd_point_vertices alone, tlc_pd_filtration_grad alone, autograd.extended_persistence
           forward + backward end to end;
  pubmed   the largest component of the PubMed-shaped synthetic graph through pd_large='device' (tlc_pd_wide), the same four;
  torch    for both, the baseline a user would write today: ranks from torch.unique, a stable sort of (graph, rank) per node,
           searchsorted per coordinate, index_add_ of the point gradients -- which also checks the ids (==) and the gradient (the
           baseline's sum is atomic, so to 1e-12).
Prints ONE JSON line and writes it to --out.

  python tools/time_pd_grad.py [--reps 5] [--inner 10] [--n-graphs 41127] [--out profiles/pd_grad_timing.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KEYS = ("up", "down", "one", "ext0")


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


def timed(fn, reps, inner):
    import torch
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / 1e3 / inner)
    return dict(median_s=float(np.median(out)), all_s=[round(x, 6) for x in out])


class TorchBaseline:
    """the vertices and the gradient from torch ops; the row -> graph maps depend on the offsets alone and are built once"""

    def __init__(self, torch, no, eo, B):
        dev = no.device
        g = torch.arange(B, device=dev)
        self.torch, self.no, self.B = torch, no, B
        self.seg_n = torch.repeat_interleave(g, no[1:] - no[:-1])
        self.seg_m = torch.repeat_interleave(g, eo[1:] - eo[:-1])
        self.row_n = torch.arange(self.seg_n.numel(), device=dev) - no[:-1][self.seg_n]
        self.row_m = torch.arange(self.seg_m.numel(), device=dev) - eo[:-1][self.seg_m]
        self.slots = (("up", self.seg_n, self.row_n, 0), ("down", self.seg_n, self.row_n, 1), ("one", self.seg_m, self.row_m, 2))

    def vertices(self, f, pd):
        torch = self.torch
        vals, rank = torch.unique(f, return_inverse=True)                        # exact ranks: every coordinate is a copy of one f[v]
        U = vals.numel() + 1
        key = self.seg_n * U + rank
        skey, order = torch.sort(key, stable=True)                               # (graph, value, id): the first equal entry has the lowest id
        out = {}
        for name, seg, row, col in self.slots:
            R = seg.numel()
            c = pd[name][:R]
            ckey = (seg * U).unsqueeze(1) + torch.searchsorted(vals, c.contiguous())
            pos = torch.searchsorted(skey, ckey.contiguous()).clamp_(max=skey.numel() - 1)
            ids = order[pos] - self.no[:-1][seg].unsqueeze(1)
            is_point = (row < pd["counts"][:, col].to(torch.int64)[seg]).unsqueeze(1)
            out[name] = torch.where(is_point & (skey[pos] == ckey), ids, torch.full_like(ids, -1)).to(torch.int32)
        g = torch.arange(self.B, device=f.device)
        ckey = (g * U).unsqueeze(1) + torch.searchsorted(vals, pd["ext0"].contiguous())
        pos = torch.searchsorted(skey, ckey.contiguous()).clamp_(max=skey.numel() - 1)
        out["ext0"] = (order[pos] - self.no[:-1].unsqueeze(1)).to(torch.int32)
        return out

    def grad(self, ids, grads, n_total):
        torch = self.torch
        out = torch.zeros(n_total, dtype=torch.float64, device=self.no.device)
        for name, seg, _, _ in self.slots:
            R = seg.numel()
            v = ids[name][:R].to(torch.int64)
            at = (v + self.no[:-1][seg].unsqueeze(1)).reshape(-1)
            ok = (v >= 0).reshape(-1)
            out.index_add_(0, at[ok], grads[name][:R].reshape(-1)[ok])
        at = (ids["ext0"].to(torch.int64) + self.no[:-1].unsqueeze(1)).reshape(-1)
        out.index_add_(0, at, grads["ext0"][:self.B].reshape(-1))
        return out


def measure(torch, no, eo, e, f, pd_large, reps, inner):
    from tlc_gnn_amd import _lib, autograd, engine
    d_no, d_eo = torch.from_numpy(no).cuda(), torch.from_numpy(eo).cuda()
    d_e = torch.from_numpy(np.ascontiguousarray(e, dtype=np.int32)).cuda()
    d_f = torch.from_numpy(np.ascontiguousarray(f, dtype=np.float64)).cuda()
    B, flags = len(no) - 1, _lib.KEEP_ZERO_PERS
    r = dict(graphs=B, nodes=int(no[-1]), edges=int(eo[-1]), pd_large=pd_large)
    forward = lambda: engine.pd_from_filtration(d_no, d_eo, d_e, d_f, flags, want_rank=False, pd_large=pd_large)
    pd = forward()
    work_bytes = engine.pd_grad_work_bytes(int(np.diff(no).max()), int(np.diff(eo).max()))
    work = torch.empty(work_bytes, dtype=torch.uint8, device="cuda")        # (empty: the entries alone, without the wrapper's size query)
    r["work_bytes"] = work_bytes
    verts = engine.pd_point_vertices(d_no, d_eo, d_f, pd, work=work)
    r["status_ok"] = bool((verts["status"] == 0).all())
    gen = torch.Generator(device="cuda").manual_seed(1)
    grads = {k: torch.randn(pd[k].shape, dtype=torch.float64, device="cuda", generator=gen) for k in KEYS}
    out = torch.zeros(max(int(no[-1]), 1), dtype=torch.float64, device="cuda")
    r["forward"] = timed(forward, reps, inner)
    r["vertices"] = timed(lambda: engine.pd_point_vertices(d_no, d_eo, d_f, pd, work=work), reps, inner)
    r["grad"] = timed(lambda: engine.pd_filtration_grad(d_no, d_eo, pd["counts"], verts, *[grads[k] for k in KEYS], work=work, out=out), reps, inner)
    # what both entries do before they launch: the two offset arrays to pageable host memory, then a wait
    r["offsets_readback"] = timed(lambda: (d_no.cpu(), d_eo.cpu()), reps, inner)
    x = d_f.clone().requires_grad_(True)

    def end_to_end():
        x.grad = None
        res = autograd.extended_persistence(x, d_no, d_eo, d_e, flags, pd_large)
        sum((res[i] * grads[k]).sum() for i, k in enumerate(KEYS)).backward()
    r["autograd_fwd_bwd"] = timed(end_to_end, reps, inner)
    base = TorchBaseline(torch, d_no, d_eo, B)
    r["torch_vertices"] = timed(lambda: base.vertices(d_f, pd), reps, inner)
    t_ids = base.vertices(d_f, pd)
    r["torch_grad"] = timed(lambda: base.grad(t_ids, grads, int(no[-1])), reps, inner)
    r["ids_match_torch"] = bool(all(torch.equal(t_ids[k], verts[k][:t_ids[k].shape[0]]) for k in KEYS))
    mine = engine.pd_filtration_grad(d_no, d_eo, pd["counts"], verts, *[grads[k] for k in KEYS], work=work)[:int(no[-1])]
    r["grad_max_abs_diff_torch"] = float((mine - base.grad(t_ids, grads, int(no[-1]))).abs().max())
    end_to_end()
    r["autograd_equals_entry"] = bool(torch.equal(x.grad, mine))
    s = lambda k: r[k]["median_s"]
    r["ratios"] = dict(vertices_over_forward=s("vertices") / s("forward"), grad_over_forward=s("grad") / s("forward"),
                       vertices_plus_grad_over_forward=(s("vertices") + s("grad")) / s("forward"),
                       autograd_over_forward=s("autograd_fwd_bwd") / s("forward"), readback_over_vertices=s("offsets_readback") / s("vertices"),
                       torch_vertices_over_vertices=s("torch_vertices") / s("vertices"), torch_grad_over_grad=s("torch_grad") / s("grad"))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--n-graphs", type=int, default=41127)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pd_grad_timing.json"))
    a = ap.parse_args()
    import torch
    from tlc_gnn_amd import synth
    assert torch.cuda.is_available(), "time_pd_grad.py measures on the GPU; there is no CPU fallback"
    res = {"tool": "time_pd_grad", "reps": a.reps, "inner": a.inner, "device": torch.cuda.get_device_name(0), "flags": "TLC_KEEP_ZERO_PERS",
           "timer": "torch.cuda.Event around `inner` calls"}
    e, _, no, eo = synth.hiv_shaped_molecules(a.n_graphs)
    res["hiv"] = measure(torch, no, eo, e, np.random.RandomState(1).rand(int(no[-1])), "host", a.reps, a.inner)
    print("# hiv: %s" % res["hiv"], file=sys.stderr, flush=True)
    n0, e0 = synth.shaped_graph("PubMed")[:2]
    n, e = largest_component(n0, np.asarray(e0))
    res["pubmed"] = measure(torch, np.array([0, n], dtype=np.int64), np.array([0, len(e)], dtype=np.int64), e,
                            np.random.RandomState(2).rand(n), "device", a.reps, a.inner)
    ok = all(res[k]["status_ok"] and res[k]["ids_match_torch"] and res[k]["autograd_equals_entry"] and res[k]["grad_max_abs_diff_torch"] < 1e-12
             for k in ("hiv", "pubmed"))
    res["all_checks_pass"] = ok
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    print(line)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

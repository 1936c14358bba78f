"""What the sliced Wasserstein diagram loss costs (csrc/sliced_w.hip), next to the matching loss it stands beside and to the same loss
and gradient from torch ops, in one process.  Each figure is the median of --reps windows after a warm-up; a window is --inner calls
between two device events (hipEvent through torch.cuda.Event) with no synchronisation of the tool's inside it, and the figure is the
window over --inner.  (tlc_sliced_wasserstein reads the offsets back itself: that wait is part of its price and is inside its figures.)
  hiv      one (predicted, target) diagram pair per HIV-shaped molecule of synth.hiv_shaped_molecules(): as many points on each side
           as the molecule has edges (Ord0 + Ext1 with zero persistence kept), random coordinates, M = 50 reference directions:
           tlc_sliced_wasserstein with the gradient of the predicted side; tlc_w2_inference_matching with its gradient on the same
           pairs; and the formulation a user would write today -- per direction one batched torch.sort of the padded lists, the L1
           distance, autograd through the sorts (a gather) -- whose loss and gradient are checked against the kernel's here;
  pubmed   ONE pair of the size of the PubMed-shaped largest component (about 44 000 points a side, which the matching kernels refuse)
           through topo.sliced_wasserstein_to(pd_large='device'), forward and backward, and its split: the diagrams (tlc_pd_wide +
           tlc_pd_point_vertices), the loss with gradient (the device-wide class), the gradient through tlc_pd_filtration_grad.
Prints ONE JSON line and writes it to --out.

  python tools/time_sliced_w.py [--reps 5] [--inner 10] [--n-graphs 41127] [--M 50] [--out profiles/sliced_w_timing.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.time_pd_grad import largest_component, timed  # noqa: E402

PAD = 1e300          # what the torch formulation fills the lists of the shorter problems with: equal in both lists, so it adds 0


class TorchSliced:
    """the loss and, through autograd, its gradient from torch ops; the index maps depend on the offsets alone and are built once"""

    def __init__(self, torch, xoff, yoff):
        dev = xoff.device
        n, m = xoff[1:] - xoff[:-1], yoff[1:] - yoff[:-1]
        B, W = n.numel(), int((n + m).max())
        col = torch.arange(W, device=dev).unsqueeze(0).expand(B, W)
        nx = int(xoff[-1])
        self.torch, self.nx = torch, nx
        # list 1: X's points then Y's (as diagonal projections); list 2: Y's points then X's.  Rows of cat([X, Y]).
        in1x, in1 = col < n.unsqueeze(1), col < (n + m).unsqueeze(1)
        in2y = col < m.unsqueeze(1)
        self.row1 = torch.where(in1x, xoff[:-1].unsqueeze(1) + col, nx + yoff[:-1].unsqueeze(1) + col - n.unsqueeze(1)).clamp_(min=0) * in1
        self.row2 = torch.where(in2y, nx + yoff[:-1].unsqueeze(1) + col, xoff[:-1].unsqueeze(1) + col - m.unsqueeze(1)).clamp_(min=0) * in1
        self.proj1, self.proj2, self.valid = in1x, in2y, in1

    def loss(self, X, Y, dirs, scale):
        torch = self.torch
        P = torch.cat([X, Y])
        b, d = P[:, 0], P[:, 1]
        c = (b + d).abs() * 0.5
        total = 0.0
        for l0, l1 in dirs:
            pr, dg = l0 * b + l1 * d, (l0 + l1) * c
            v1 = torch.where(self.valid, torch.where(self.proj1, pr[self.row1], dg[self.row1]), PAD)
            v2 = torch.where(self.valid, torch.where(self.proj2, pr[self.row2], dg[self.row2]), PAD)
            s1, s2 = torch.sort(v1, dim=1, stable=True)[0], torch.sort(v2, dim=1, stable=True)[0]
            total = total + scale * (s1 - s2).abs().sum(1)
        return total


def hiv(torch, n_graphs, M, reps, inner):
    from tlc_gnn_amd import ops, synth
    _, _, _, eo = synth.hiv_shaped_molecules(n_graphs)
    rs = np.random.RandomState(1)

    def dgm(k):
        b = rs.random_sample(k)
        return np.stack([b, b + rs.random_sample(k)], 1)
    offs = torch.from_numpy(np.ascontiguousarray(eo, dtype=np.int64)).cuda()
    X, Y = torch.from_numpy(dgm(int(eo[-1]))).cuda(), torch.from_numpy(dgm(int(eo[-1]))).cuda()
    sizes = 2 * np.diff(eo)
    r = dict(pairs=len(eo) - 1, points_per_side=int(eo[-1]), largest_pair=int(sizes.max()), median_pair=float(np.median(sizes)), M=M,
             pairs_above_64_points=int((sizes > 64).sum()))
    d_np, scale = ops.sliced_directions(M)
    dirs = torch.from_numpy(d_np).cuda()
    mine = ops.sliced_wasserstein(offs, X, offs, Y, dirs=dirs, scale=scale, want_grad=("x",))
    r["status_ok"] = bool((mine["status"] == 0).all())
    r["sliced"] = timed(lambda: ops.sliced_wasserstein(offs, X, offs, Y, dirs=dirs, scale=scale, want_grad=("x",)), reps, inner)
    r["sliced_no_grad"] = timed(lambda: ops.sliced_wasserstein(offs, X, offs, Y, dirs=dirs, scale=scale, want_grad=()), reps, inner)
    r["w2_inference_matching"] = timed(lambda: ops.w2_inference_matching(offs, X, offs, Y, order=2, want_grad=True), reps, max(inner // 5, 1))
    base = TorchSliced(torch, offs, offs)
    dl = d_np.tolist()
    x = X.clone().requires_grad_(True)

    def torch_fwd_bwd():
        x.grad = None
        base.loss(x, Y, dl, scale).sum().backward()
    r["torch_sort_fwd_bwd"] = timed(torch_fwd_bwd, reps, max(inner // 5, 1))
    with torch.no_grad():
        tl = base.loss(X, Y, dl, scale)
    r["torch_sort_fwd"] = timed(lambda: base.loss(X.detach(), Y, dl, scale), reps, max(inner // 5, 1))
    torch_fwd_bwd()
    r["loss_max_rel_diff_torch"] = float(((mine["loss"] - tl).abs() / tl.abs().clamp_min(1e-300)).max())
    r["grad_max_abs_diff_torch"] = float((mine["grad_x"] - x.grad).abs().max())
    s = lambda k: r[k]["median_s"]
    r["ratios"] = dict(w2_over_sliced=s("w2_inference_matching") / s("sliced"), torch_over_sliced=s("torch_sort_fwd_bwd") / s("sliced"),
                       torch_fwd_over_sliced_no_grad=s("torch_sort_fwd") / s("sliced_no_grad"))
    r["checks_pass"] = bool(r["status_ok"] and r["loss_max_rel_diff_torch"] < 1e-10 and r["grad_max_abs_diff_torch"] < 1e-10)
    return r


def pubmed(torch, M, reps, inner):
    from tlc_gnn_amd import _lib, ops, synth, topo
    n0, e0 = synth.shaped_graph("PubMed")[:2]
    n, e = largest_component(n0, np.asarray(e0))
    no = torch.tensor([0, n], dtype=torch.int64, device="cuda")
    eo = torch.tensor([0, len(e)], dtype=torch.int64, device="cuda")
    E = torch.from_numpy(np.ascontiguousarray(e, dtype=np.int32)).cuda()
    f = torch.from_numpy(np.random.RandomState(2).rand(n)).cuda()
    with torch.no_grad():
        target, toffs = topo._select(torch.from_numpy(np.random.RandomState(3).rand(n)).cuda(), no, eo, E, "ord0+ext1", "device")
    target, toffs = target.contiguous(), toffs.contiguous()
    x = f.clone().requires_grad_(True)
    pts, offs = topo._select(x, no, eo, E, "ord0+ext1", "device")
    N = int(offs[-1]) + int(toffs[-1])
    r = dict(nodes=n, edges=int(len(e)), points_predicted=int(offs[-1]), points_target=int(toffs[-1]), M=M,
             work_bytes=ops.sliced_w_work_bytes(1, N, N, M), work_bytes_one_direction=ops.sliced_w_work_bytes(1, N, N, 1))
    # csrc/sliced_w.hip, sw_run_wide: the coordinate check once, and per group of directions the keys, 9 radix passes of 3 kernels, the
    # signs, the loss and the point sums; the default workspace (capped at ops.SLICED_W_WORK_CAP) decides the groups
    r["default_work_bytes"] = min(r["work_bytes"], max(ops.SLICED_W_WORK_CAP, r["work_bytes_one_direction"]))
    r["one_group_at_default_workspace"] = bool(r["default_work_bytes"] == r["work_bytes"])
    r["device_wide_kernel_launches_one_group"] = 1 + (1 + 27 + 2 + 1)
    r["matching_status"] = int(ops.w2_inference_matching(offs, pts.detach(), toffs, target, order=2)["status"][0])     # 2: too many points
    d_np, scale = ops.sliced_directions(M)
    dirs = torch.from_numpy(d_np).cuda()
    p0 = pts.detach()
    res = ops.sliced_wasserstein(offs, p0, toffs, target, dirs=dirs, scale=scale, want_grad=("x",))
    r["status_ok"] = int(res["status"][0]) == 0
    r["loss"] = float(res["loss"][0])

    def end_to_end():
        x.grad = None
        topo.sliced_wasserstein_to(x, no, eo, E, target, toffs, M=M, pd_large="device").sum().backward()
    r["fwd_bwd"] = timed(end_to_end, reps, inner)
    with torch.no_grad():
        r["diagrams"] = timed(lambda: topo._select(f, no, eo, E, "ord0+ext1", "device"), reps, inner)
    r["loss_with_grad"] = timed(lambda: ops.sliced_wasserstein(offs, p0, toffs, target, dirs=dirs, scale=scale, want_grad=("x",)), reps, inner)
    r["loss_no_grad"] = timed(lambda: ops.sliced_wasserstein(offs, p0, toffs, target, dirs=dirs, scale=scale, want_grad=()), reps, inner)
    least = r["work_bytes_one_direction"]
    r["loss_with_grad_least_workspace"] = timed(lambda: ops.sliced_wasserstein(offs, p0, toffs, target, dirs=dirs, scale=scale, want_grad=("x",),
                                                                               work_bytes=least), 3, 1)
    g = res["grad_x"]

    def back():
        x.grad = None
        pts.backward(g, retain_graph=True)
    r["grad_through_pd_grad"] = timed(back, reps, inner)
    end_to_end()
    whole = x.grad.clone()
    back()
    r["autograd_equals_parts"] = bool(torch.equal(whole, x.grad))
    r["checks_pass"] = bool(r["status_ok"] and r["autograd_equals_parts"] and np.isfinite(r["loss"]) and N > 4096 and N > _lib.SW_LDS_NMAX)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--n-graphs", type=int, default=41127)
    ap.add_argument("--M", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sliced_w_timing.json"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "time_sliced_w.py measures on the GPU; there is no CPU fallback"
    res = {"tool": "time_sliced_w", "reps": a.reps, "inner": a.inner, "device": torch.cuda.get_device_name(0),
           "timer": "torch.cuda.Event around `inner` calls"}
    res["hiv"] = hiv(torch, a.n_graphs, a.M, a.reps, a.inner)
    print("# hiv: %s" % res["hiv"], file=sys.stderr, flush=True)
    res["pubmed"] = pubmed(torch, a.M, a.reps, a.inner)
    ok = bool(res["hiv"]["checks_pass"] and res["pubmed"]["checks_pass"])
    res["all_checks_pass"] = ok
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    print(line)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

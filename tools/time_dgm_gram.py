"""What the Gram matrix of a diagram kernel costs (csrc/dgm_gram.hip), forward and VJP, next to the formulation a user would write today in
torch ops -- the padded diagrams [B, n_max, 2], torch.cdist -> exp -> masked sum, autograd through it -- on the same GPU, in one
process.  Each figure is the median of --reps windows after a warm-up; a window is --inner calls between two device events (hipEvent
through torch.cuda.Event) with no synchronisation of the tool's inside it, and the figure is the window over --inner.  (The entries
read the offsets back themselves: that wait is part of their price and is inside their figures.)  The kernel is the PSS kernel
(mirror term, no weights) at sigma = 0.1 throughout.
  gram       the symmetric Gram matrix of the first --gram-dgms (4 096) diagrams of synth.hiv_shaped_molecules(): as many points as the
             molecule has edges, random coordinates.  The torch baseline materialises 8 B x Bx x By x n_max^2 per tensor: it runs on the
             first diagrams that pad to --baseline-points points a side (the figure says how many), as does the kernel's "same_diagrams" figure beside it.
  paired     the squared PSS distance k(X,X) + k(Y,Y) - 2 k(X,Y) between all --n-graphs (41 127) molecule diagrams and as many targets,
             forward and forward + backward (three PAIRED calls and three VJPs); the baseline on the same diagrams in blocks.
  medium     256 diagrams of about 400 points, symmetric Gram, forward and VJP; the baseline likewise.
  large      one 70 000 x 70 000 pair (slices, groups and the merge), with the full and with the least workspace, and its VJP.  No baseline:
             the 70 000 x 70 000 distance matrix is 39 GB.
Also writes profiles/dgm_gram_resource_usage.txt (hipcc's remarks per instantiation: VGPRs, LDS, scratch; needs hipcc, no GPU:
--only-resource-usage).  Prints ONE JSON line and writes it to --out.

  python tools/time_dgm_gram.py [--reps 5] [--inner 3] [--n-graphs 41127] [--out profiles/dgm_gram_timing.json]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.time_pd_grad import timed  # noqa: E402

HIPCC = "/opt/rocm/bin/hipcc"
SRC = os.path.join("tlc-gnn_amd", "csrc", "dgm_gram.hip")
SIGMA = 0.1
CDIST_CELLS = 1 << 22                         # distances per torch.cdist call of the ALL-mode baseline
EXACT = "donot_use_mm_for_euclid_dist"        # cdist from differences: the matrix-product form cancels to 1e-8 in fp64


def resource_usage(path):
    """hipcc's kernel-resource-usage remarks of csrc/dgm_gram.hip -> path; True when no kernel uses scratch"""
    cmd = [HIPCC, "-O3", "-fPIC", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
           "-Rpass-analysis=kernel-resource-usage", "-c", SRC, "-o", os.devnull]
    err = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT).stderr
    keep = ("Function Name", "TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize", "Occupancy", "SGPRs Spill", "LDS Size")
    lines, scratch = [], []
    for l in err.splitlines():
        if "remark:" not in l:
            continue
        t = l.split("remark:", 1)[1].split("[-Rpass")[0].strip()
        if t.startswith(keep):
            lines.append(t if t.startswith("Function Name") else "    " + t)
        if t.startswith("ScratchSize"):
            scratch.append(int(t.rsplit(":", 1)[1]))
    head = ("hipcc -O3 --offload-arch=gfx950 -ffp-contract=off -fno-fast-math -Rpass-analysis=kernel-resource-usage -c %s\n"
            "(dg_status_kernel: a wavefront per diagram; dg_unit_kernel<MIRROR, WEIGHTS>: a wavefront per (slice of X_i, group of Y_j), the\n"
            " slice's points as readlanes; dg_merge_kernel: a thread per pair; dg_vjp_all_kernel / dg_vjp_paired_kernel<MIRROR, WEIGHTS>: a lane\n"
            " per point of X.  256-thread workgroups, no LDS, no scratch in any instantiation)\n" % SRC)
    with open(path, "w") as fh:
        fh.write(head + "\n".join(lines) + "\n")
    return bool(scratch) and not any(scratch)


def random_points(rs, k):
    b = rs.random_sample(k)
    return np.stack([b, b + rs.random_sample(k)], 1)


class Padded:
    """a packed batch as the padded tensors of the torch formulation; the index maps depend on the offsets alone and are built once"""

    def __init__(self, torch, offs, n_points):
        n = offs[1:] - offs[:-1]
        W = max(int(n.max()), 1)
        col = torch.arange(W, device=offs.device).unsqueeze(0)
        self.mask = (col < n.unsqueeze(1)).to(torch.float64)                # [B, W]
        self.row = (offs[:-1].unsqueeze(1) + col).clamp_(max=max(n_points - 1, 0))
        self.W = W

    def __call__(self, pts):
        return pts[self.row]                                                 # [B, W, 2]


def torch_gram(torch, px, mx, py, my, gamma, scale):
    """[Bx, By]: sum over the valid point pairs of e1 - e2 from torch.cdist on the padded points (the mirror image swaps the columns)"""
    Bx, Wx, By, Wy = px.shape[0], px.shape[1], py.shape[0], py.shape[1]
    b = py.reshape(1, By * Wy, 2)
    # in blocks of X's diagrams of at most CDIST_CELLS distances: one cdist call over 16 384 x 16 384 points returned wrong distances
    # on this stack (its launch has one workgroup per distance), and the batched calls of torch_paired, 4.5 M distances each, did not
    step = max(1, CDIST_CELLS // (Wx * By * Wy))
    rows = []
    for i0 in range(0, Bx, step):
        a = px[i0:i0 + step].reshape(1, -1, 2)
        d1 = torch.cdist(a, b, compute_mode=EXACT)[0]
        d2 = torch.cdist(a, b.flip(-1), compute_mode=EXACT)[0]
        e = torch.exp(-gamma * d1 * d1) - torch.exp(-gamma * d2 * d2)
        e = e * mx[i0:i0 + step].reshape(-1, 1) * my.reshape(1, -1)
        rows.append(e.reshape(-1, Wx, By, Wy).sum(dim=(1, 3)))
    return scale * torch.cat(rows)


def torch_paired(torch, px, mx, py, my, gamma, scale):
    """[B]: the same for diagram i against diagram i (batched cdist)"""
    d1, d2 = torch.cdist(px, py, compute_mode=EXACT), torch.cdist(px, py.flip(-1), compute_mode=EXACT)
    e = (torch.exp(-gamma * d1 * d1) - torch.exp(-gamma * d2 * d2)) * mx.unsqueeze(2) * my.unsqueeze(1)
    return scale * e.sum(dim=(1, 2))


def batch(torch, sizes, seed):
    rs = np.random.RandomState(seed)
    offs_h = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return offs_h, torch.from_numpy(offs_h).cuda(), torch.from_numpy(random_points(rs, int(offs_h[-1]))).cuda()


def gram_workload(torch, sizes, n_base, reps, inner, seed):
    """the symmetric Gram matrix and its VJP; the torch formulation on as many of the first diagrams as pad to n_base points"""
    from tlc_gnn_amd import engine, ops
    gamma, scale, mirror = ops.dgm_kernel_params("pss", SIGMA)
    offs_h, offs, pts = batch(torch, sizes, seed)
    B = len(sizes)
    r = dict(diagrams=B, points=int(offs_h[-1]), largest=int(max(sizes)), median=float(np.median(sizes)),
             point_pairs=int(np.sum(sizes)) ** 2)
    call = lambda: engine.dgm_gram(pts, offs, None, pts, offs, None, gamma, scale, mirror, symmetric=True)      # noqa: E731
    out, sx, _ = call()
    r["status_ok"] = bool((sx == 0).all())
    G = torch.from_numpy(np.random.RandomState(seed + 1).standard_normal((B, B))).cuda()
    Gs = (G + G.t()).contiguous()
    vj = lambda: engine.dgm_gram_vjp(pts, offs, None, pts, offs, None, gamma, scale, mirror, sx, sx, Gs)       # noqa: E731
    grad, _ = vj()
    r["forward_symmetric"] = timed(call, reps, inner)
    r["forward_general"] = timed(lambda: engine.dgm_gram(pts, offs, None, pts, offs, None, gamma, scale, mirror), reps, inner)
    r["vjp"] = timed(vj, reps, inner)
    nb = max(1, min(B, n_base // max(int(max(sizes)), 1)))           # n_base padded points a side: the distance matrix is 8 n_base^2 bytes
    boffs, bpts = offs[:nb + 1].contiguous(), pts[:int(offs_h[nb])].clone().requires_grad_(True)
    pad = Padded(torch, boffs, int(offs_h[nb]))
    r["baseline"] = dict(diagrams=nb, points=int(offs_h[nb]), distance_matrix_bytes=8 * (nb * pad.W) ** 2)
    with torch.no_grad():
        bo = torch_gram(torch, pad(bpts), pad.mask, pad(bpts), pad.mask, gamma, scale)
    r["baseline"]["value_max_rel_diff"] = float(((bo - out[:nb, :nb]).abs() / out[:nb, :nb].abs().clamp_min(1e-300)).max())
    r["baseline"]["value_max_abs_diff"] = float((bo - out[:nb, :nb]).abs().max())

    def base_fwd():
        with torch.no_grad():
            torch_gram(torch, pad(bpts), pad.mask, pad(bpts), pad.mask, gamma, scale)

    def base_both():
        bpts.grad = None
        p = pad(bpts)
        (torch_gram(torch, p, pad.mask, p, pad.mask, gamma, scale) * G[:nb, :nb]).sum().backward()
    base_both()
    bsx = sx[:nb].contiguous()
    Gb = (G[:nb, :nb] + G[:nb, :nb].t()).contiguous()
    sub = bpts.detach()
    gsub, _ = engine.dgm_gram_vjp(sub, boffs, None, sub, boffs, None, gamma, scale, mirror, bsx, bsx, Gb)
    r["baseline"]["grad_max_abs_diff"] = float((bpts.grad - gsub).abs().max()) if gsub.numel() else 0.0
    r["baseline"]["grad_max_abs"] = float(gsub.abs().max()) if gsub.numel() else 0.0
    r["baseline"]["forward"] = timed(base_fwd, reps, inner)
    r["baseline"]["forward_backward"] = timed(base_both, reps, inner)
    mine_fwd = lambda: engine.dgm_gram(sub, boffs, None, sub, boffs, None, gamma, scale, mirror, symmetric=True)   # noqa: E731

    def mine_both():
        mine_fwd()
        engine.dgm_gram_vjp(sub, boffs, None, sub, boffs, None, gamma, scale, mirror, bsx, bsx, Gb)
    r["same_diagrams"] = dict(forward=timed(mine_fwd, reps, inner), forward_vjp=timed(mine_both, reps, inner))
    r["speedup_forward"] = r["baseline"]["forward"]["median_s"] / r["same_diagrams"]["forward"]["median_s"]
    r["speedup_forward_backward"] = r["baseline"]["forward_backward"]["median_s"] / r["same_diagrams"]["forward_vjp"]["median_s"]
    r["checks_pass"] = bool(r["status_ok"] and r["baseline"]["value_max_abs_diff"] <= 1e-9 * float(out.abs().max())
                            and r["baseline"]["grad_max_abs_diff"] <= 1e-9 * max(r["baseline"]["grad_max_abs"], 1.0))
    return r


def paired_workload(torch, sizes, reps, inner, seed, block=2048):
    """the squared PSS distance between every diagram and a target of the same size, forward and with the backward"""
    from tlc_gnn_amd import autograd
    offs_h, offs, pts = batch(torch, sizes, seed)
    _, _, tgt = batch(torch, sizes, seed + 1)
    B = len(sizes)
    r = dict(diagrams=B, points=int(offs_h[-1]), largest=int(max(sizes)), point_pairs=int(3 * np.sum(np.asarray(sizes, dtype=np.int64) ** 2)))
    x = pts.clone().requires_grad_(True)

    def mine_fwd():
        with torch.no_grad():
            return autograd.diagram_kernel_distance(x, offs, tgt, offs, sigma=SIGMA)

    def mine_both():
        x.grad = None
        autograd.diagram_kernel_distance(x, offs, tgt, offs, sigma=SIGMA).sum().backward()
    d = mine_fwd()
    mine_both()
    g = x.grad.clone()
    r["forward"] = timed(mine_fwd, reps, inner)
    r["forward_backward"] = timed(mine_both, reps, inner)
    from tlc_gnn_amd import ops
    gamma, scale, _ = ops.dgm_kernel_params("pss", SIGMA)
    pads = []
    for b0 in range(0, B, block):
        b1 = min(B, b0 + block)
        bo = (offs[b0:b1 + 1] - offs[b0]).contiguous()
        lo, hi = int(offs_h[b0]), int(offs_h[b1])
        pads.append((lo, hi, Padded(torch, bo, hi - lo)))
    y = pts.clone().requires_grad_(True)

    def base(p):
        outs = []
        for lo, hi, pad in pads:
            a, b = pad(p[lo:hi]), pad(tgt[lo:hi])
            outs.append(torch_paired(torch, a, pad.mask, a, pad.mask, gamma, scale) + torch_paired(torch, b, pad.mask, b, pad.mask, gamma, scale)
                        - 2.0 * torch_paired(torch, a, pad.mask, b, pad.mask, gamma, scale))
        return torch.cat(outs)

    def base_fwd():
        with torch.no_grad():
            return base(y)

    def base_both():
        y.grad = None
        base(y).sum().backward()
    bd = base_fwd()
    base_both()
    r["baseline"] = dict(diagrams=B, blocks=len(pads), value_max_abs_diff=float((bd - d).abs().max()), grad_max_abs_diff=float((y.grad - g).abs().max()),
                         forward=timed(base_fwd, reps, inner), forward_backward=timed(base_both, reps, inner))
    r["speedup_forward"] = r["baseline"]["forward"]["median_s"] / r["forward"]["median_s"]
    r["speedup_forward_backward"] = r["baseline"]["forward_backward"]["median_s"] / r["forward_backward"]["median_s"]
    r["checks_pass"] = bool(r["baseline"]["value_max_abs_diff"] <= 1e-9 * max(float(d.abs().max()), 1.0)
                            and r["baseline"]["grad_max_abs_diff"] <= 1e-9 * max(float(g.abs().max()), 1.0))
    return r


def large_workload(torch, n, reps, inner, seed):
    from tlc_gnn_amd import engine, ops
    gamma, scale, mirror = ops.dgm_kernel_params("pss", SIGMA)
    _, xo, x = batch(torch, [n], seed)
    _, yo, y = batch(torch, [n], seed + 1)
    flags = engine.dgm_gram_flags(mirror, False)
    full, least = engine.dgm_gram_work_bytes(1, 1, n, n, flags)
    r = dict(points=n, point_pairs=n * n, work_bytes=full, work_bytes_least=least)
    wf = torch.empty(full, dtype=torch.uint8, device="cuda")
    call = lambda w: engine.dgm_gram(x, xo, None, y, yo, None, gamma, scale, mirror, work=w)                    # noqa: E731
    out, sx, sy = call(wf)
    r["value"] = float(out[0, 0])
    r["forward"] = timed(lambda: call(wf), reps, inner)
    if least < full:
        wl = torch.empty(least, dtype=torch.uint8, device="cuda")
        r["least_workspace_same_bits"] = bool(torch.equal(call(wl)[0], out))
        r["forward_least_workspace"] = timed(lambda: call(wl), reps, inner)
    G = torch.ones((1, 1), dtype=torch.float64, device="cuda")
    r["vjp"] = timed(lambda: engine.dgm_gram_vjp(x, xo, None, y, yo, None, gamma, scale, mirror, sx, sy, G, work=wf), reps, inner)
    r["checks_pass"] = bool(np.isfinite(r["value"]) and r.get("least_workspace_same_bits", True))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--n-graphs", type=int, default=41127)
    ap.add_argument("--gram-dgms", type=int, default=4096)
    ap.add_argument("--baseline-points", type=int, default=16384, help="padded points a side of the torch baseline")
    ap.add_argument("--large", type=int, default=70000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dgm_gram_timing.json"))
    ap.add_argument("--resource-out", default=os.path.join(ROOT, "profiles", "dgm_gram_resource_usage.txt"))
    ap.add_argument("--only-resource-usage", action="store_true")
    ap.add_argument("--no-resource-usage", action="store_true")
    a = ap.parse_args()
    no_scratch = None
    if not a.no_resource_usage and os.path.exists(HIPCC):
        no_scratch = resource_usage(a.resource_out)
        print("# resource usage -> %s, no scratch: %s" % (a.resource_out, no_scratch), file=sys.stderr, flush=True)
    if a.only_resource_usage:
        return 0 if no_scratch else 1
    import torch
    from tlc_gnn_amd import synth
    assert torch.cuda.is_available(), "time_dgm_gram.py measures on the GPU; there is no CPU fallback"
    res = {"tool": "time_dgm_gram", "reps": a.reps, "inner": a.inner, "device": torch.cuda.get_device_name(0), "kernel": "pss", "sigma": SIGMA,
           "timer": "torch.cuda.Event around `inner` calls", "no_scratch": no_scratch}
    _, _, _, eo = synth.hiv_shaped_molecules(a.n_graphs)
    sizes = np.diff(eo).tolist()
    res["gram"] = gram_workload(torch, sizes[:a.gram_dgms], a.baseline_points, a.reps, a.inner, seed=1)
    print("# gram: %s" % res["gram"], file=sys.stderr, flush=True)
    res["paired"] = paired_workload(torch, sizes, a.reps, a.inner, seed=5)
    print("# paired: %s" % res["paired"], file=sys.stderr, flush=True)
    medium = np.random.RandomState(2).randint(350, 451, size=256).tolist()
    res["medium"] = gram_workload(torch, medium, a.baseline_points, a.reps, a.inner, seed=3)
    print("# medium: %s" % res["medium"], file=sys.stderr, flush=True)
    res["large"] = large_workload(torch, a.large, a.reps, a.inner, seed=7)
    print("# large: %s" % res["large"], file=sys.stderr, flush=True)
    ok = bool(all(res[k]["checks_pass"] for k in ("gram", "paired", "medium", "large")) and no_scratch is not False)
    res["all_checks_pass"] = ok
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    print(line)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

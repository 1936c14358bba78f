"""What the persistence landscape costs (csrc/landscape.hip), forward and VJP, next to the formulation a user would write today in torch
ops -- the padded tents [B, n_max, T], torch.topk over the points, autograd through it -- on the same GPU, in one process.  Each figure
is the median of --reps windows after a warm-up; a window is --inner calls between two device events (hipEvent through
torch.cuda.Event) with no synchronisation of the tool's inside it, and the figure is the window over --inner.  (tlc_landscape and
tlc_landscape_vjp read the offsets and the samples back themselves: that wait is part of their price and is inside their figures.)
  molecules  one diagram per HIV-shaped molecule of synth.hiv_shaped_molecules(): as many points as the molecule has edges, random
             coordinates, K = 5, T = 100.  The torch baseline materialises 8 B x B x n_max x T per tensor and keeps several for autograd:
             it runs on the first --baseline-dgms diagrams (the figure says how many) and its values are checked against the kernel's.
  medium     4 096 diagrams of about 400 points (the workgroup class); the baseline on the first --baseline-dgms / 8 of them.
  large      one 70 000-point diagram (the whole-device class: slices and a merge), with the full and with the least workspace.
Also writes profiles/landscape_resource_usage.txt (hipcc's remarks per instantiation: VGPRs, LDS, scratch; needs hipcc, no GPU:
--only-resource-usage).  Prints ONE JSON line and writes it to --out.

  python tools/time_landscape.py [--reps 5] [--inner 10] [--n-graphs 41127] [--out profiles/landscape_timing.json]
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
SRC = os.path.join("tlc-gnn_amd", "csrc", "landscape.hip")


def resource_usage(path):
    """hipcc's kernel-resource-usage remarks of csrc/landscape.hip -> path; True when no kernel uses scratch"""
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
            "(ls_wave_kernel<KT>: a wavefront per diagram; ls_lds_kernel<KT> / ls_slice_kernel<KT>: a 256-thread workgroup per (diagram or slice,\n"
            " 256 samples), LDS is dynamic: 16 B per staged point, 65 536 B at the cap and for every slice; ls_merge_kernel<KT>: a thread per\n"
            " sample; ls_vjp_*: the gradient.  KT = 1, 2, 4, 8, 16 entries of the sorted list in registers; no scratch in any instantiation)\n" % SRC)
    with open(path, "w") as fh:
        fh.write(head + "\n".join(lines) + "\n")
    return bool(scratch) and not any(scratch)


def random_points(rs, k):
    b = rs.random_sample(k)
    return np.stack([b, b + rs.random_sample(k)], 1)


class TorchLandscape:
    """the landscape and, through autograd, its gradient from torch ops; the index maps depend on the offsets alone and are built once"""

    def __init__(self, torch, offs, n_points):
        n = offs[1:] - offs[:-1]
        W = int(n.max())
        col = torch.arange(W, device=offs.device).unsqueeze(0)
        self.torch, self.valid = torch, (col < n.unsqueeze(1)).unsqueeze(2)
        self.row = (offs[:-1].unsqueeze(1) + col).clamp_(max=max(n_points - 1, 0))
        self.bytes_per_tensor = 8 * self.row.numel()

    def __call__(self, pts, ts, K):
        torch = self.torch
        b, d = pts[:, 0][self.row].unsqueeze(2), pts[:, 1][self.row].unsqueeze(2)
        v = torch.minimum(ts - b, d - ts)                                   # [B, n_max, T]
        v = torch.where(self.valid, v, torch.zeros((), dtype=v.dtype, device=v.device)).clamp_min(0.0)
        if v.shape[1] < K:
            v = torch.cat([v, v.new_zeros(v.shape[0], K - v.shape[1], v.shape[2])], 1)
        return v.topk(K, dim=1).values


def workload(torch, sizes, K, T, n_base, reps, inner, seed, least_too=False):
    from tlc_gnn_amd import engine
    rs = np.random.RandomState(seed)
    offs_h = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    offs = torch.from_numpy(offs_h).cuda()
    pts = torch.from_numpy(random_points(rs, int(offs_h[-1]))).cuda()
    ts = torch.linspace(0.0, 2.0, T, dtype=torch.float64, device="cuda")
    B = len(sizes)
    r = dict(diagrams=B, points=int(offs_h[-1]), largest=int(max(sizes)), median=float(np.median(sizes)), K=K, T=T,
             classes=dict(wave=int((np.asarray(sizes) <= 64).sum()), lds=int(((np.asarray(sizes) > 64) & (np.asarray(sizes) <= 4096)).sum()),
                          wide=int((np.asarray(sizes) > 4096).sum())))
    full, least = engine.landscape_work_bytes(B, int(max(sizes)), K, T)
    r["work_bytes"], r["work_bytes_least"] = full, least
    work = torch.empty(full, dtype=torch.uint8, device="cuda") if full else None
    out, win, st = engine.landscape(pts, offs, ts, K, work=work)
    r["status_ok"] = bool((st == 0).all())
    gout = torch.from_numpy(rs.standard_normal(tuple(out.shape))).cuda()
    grad = engine.landscape_vjp(pts, offs, ts, K, win, gout)
    r["forward"] = timed(lambda: engine.landscape(pts, offs, ts, K, work=work), reps, inner)
    r["forward_no_winners"] = timed(lambda: engine.landscape(pts, offs, ts, K, winners=False, work=work), reps, inner)
    r["vjp"] = timed(lambda: engine.landscape_vjp(pts, offs, ts, K, win, gout), reps, inner)
    if least_too and least < full:
        wl = torch.empty(least, dtype=torch.uint8, device="cuda")
        o2, w2, _ = engine.landscape(pts, offs, ts, K, work=wl)
        r["least_workspace_same_bits"] = bool(torch.equal(o2, out) and torch.equal(w2, win))
        r["forward_least_workspace"] = timed(lambda: engine.landscape(pts, offs, ts, K, work=wl), reps, inner)
    # the torch formulation on the first n_base diagrams
    nb = min(n_base, B)
    boffs, bpts = offs[:nb + 1].contiguous(), pts[:int(offs_h[nb])].clone().requires_grad_(True)
    base = TorchLandscape(torch, boffs, int(offs_h[nb]))
    r["baseline"] = dict(diagrams=nb, points=int(offs_h[nb]), padded_tensor_bytes=int(base.bytes_per_tensor * T))
    with torch.no_grad():
        bo = base(bpts, ts, K)
    r["baseline"]["values_equal"] = bool(torch.equal(bo, out[:nb]))
    (base(bpts, ts, K) * gout[:nb]).sum().backward()
    bg = bpts.grad.clone()
    # (under ties autograd's topk picks its own winner; random coordinates have none, so the gradients agree up to the order of a sum)
    r["baseline"]["grad_max_abs_diff"] = float((bg - grad[:int(offs_h[nb])]).abs().max()) if bg.numel() else 0.0

    def base_fwd():
        with torch.no_grad():
            base(bpts, ts, K)

    def base_both():
        bpts.grad = None
        (base(bpts, ts, K) * gout[:nb]).sum().backward()
    r["baseline"]["forward"] = timed(base_fwd, reps, inner)
    r["baseline"]["forward_backward"] = timed(base_both, reps, inner)
    # the kernels on the same diagrams, so that the two columns compare like with like
    r["same_diagrams"] = dict(forward=timed(lambda: engine.landscape(bpts.detach(), boffs, ts, K, work=work), reps, inner))
    wsub = win[:nb].contiguous()

    def mine_both():
        engine.landscape(bpts.detach(), boffs, ts, K, work=work)
        engine.landscape_vjp(bpts.detach(), boffs, ts, K, wsub, gout[:nb])
    r["same_diagrams"]["forward_vjp"] = timed(mine_both, reps, inner)
    r["speedup_forward"] = r["baseline"]["forward"]["median_s"] / r["same_diagrams"]["forward"]["median_s"]
    r["speedup_forward_backward"] = r["baseline"]["forward_backward"]["median_s"] / r["same_diagrams"]["forward_vjp"]["median_s"]
    r["checks_pass"] = bool(r["status_ok"] and r["baseline"]["values_equal"] and r["baseline"]["grad_max_abs_diff"] < 1e-9
                            and r.get("least_workspace_same_bits", True))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--n-graphs", type=int, default=41127)
    ap.add_argument("--baseline-dgms", type=int, default=8192)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "landscape_timing.json"))
    ap.add_argument("--resource-out", default=os.path.join(ROOT, "profiles", "landscape_resource_usage.txt"))
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
    assert torch.cuda.is_available(), "time_landscape.py measures on the GPU; there is no CPU fallback"
    res = {"tool": "time_landscape", "reps": a.reps, "inner": a.inner, "device": torch.cuda.get_device_name(0),
           "timer": "torch.cuda.Event around `inner` calls", "no_scratch": no_scratch}
    _, _, _, eo = synth.hiv_shaped_molecules(a.n_graphs)
    res["molecules"] = workload(torch, np.diff(eo).tolist(), 5, 100, a.baseline_dgms, a.reps, a.inner, seed=1)
    print("# molecules: %s" % res["molecules"], file=sys.stderr, flush=True)
    sizes = np.random.RandomState(2).randint(350, 451, size=4096).tolist()
    res["medium"] = workload(torch, sizes, 5, 100, max(a.baseline_dgms // 8, 1), a.reps, a.inner, seed=3)
    print("# medium: %s" % res["medium"], file=sys.stderr, flush=True)
    res["large"] = workload(torch, [70000], 5, 100, 1, a.reps, a.inner, seed=4, least_too=True)
    ok = bool(res["molecules"]["checks_pass"] and res["medium"]["checks_pass"] and res["large"]["checks_pass"] and no_scratch is not False)
    res["all_checks_pass"] = ok
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    print(line)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

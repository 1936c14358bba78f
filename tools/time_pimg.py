"""What the general persistence imager costs (csrc/pi_general.hip: tlc_pi_image, tlc_pi_image_vjp), next to two yardsticks timed in the
same process on the same diagrams:
  pi_raster   engine.pi_raster at the default specification (5 x 5, unit ranges, sigma = I): the kernel of that one configuration.
              The general entry is not expected to beat it; at other specifications it is only a scale (it computes another image).
  torch       the batched formulation a user would write: torch.special.erfc tables per point, the diagrams padded to the longest
              one, one batched matrix product U^T V per diagram (einsum), autograd for the gradients.  Its images are compared with the
              kernel's here.
Each figure is the median of --reps windows after a warm-up; a window is `inner` calls between two device events with no
synchronisation of the tool's inside it (engine.pi_image copies the offsets to the host once per call: that wait is part of its
price and is inside its figures).
Workloads: the 41 127 molecule-shaped diagrams (one per graph of synth.hiv_shaped_molecules(): nodes + edges points, about 50) at the
default 5 x 5, at 20 x 20 and at 50 x 50 with variance 0.01; 4 096 diagrams of about 400 points at 50 x 50; one diagram of 70 000
points at 100 x 100 (K-split); the vjp in both modes; one correlated case (r = 0.5) at 20 x 20, which has no torch yardstick.
Prints ONE JSON line and writes it to --out.

  python tools/time_pimg.py [--reps 5] [--n-graphs 41127] [--out profiles/pimg_timing.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.time_pd_grad import timed  # noqa: E402


def lines(res):
    return np.linspace(0.0, 1.0 + 1.0 / res, res + 1, endpoint=False, dtype=np.float64)


def diagrams(lens, seed):
    rs = np.random.RandomState(seed)
    k = int(lens.sum())
    b = 0.6 * rs.random_sample(k)
    pts = np.stack([b, b + 0.9 * rs.random_sample(k)], 1)
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), pts


class TorchImager:
    """images [B, Rb * Rp] of a padded batch from torch ops (separable sigma); the index maps depend on the offsets alone"""

    def __init__(self, torch, offs, spec):
        self.torch = torch
        n = offs[1:] - offs[:-1]
        B, L = n.numel(), max(int(n.max()), 1)
        col = torch.arange(L, device=offs.device).unsqueeze(0).expand(B, L)
        self.valid = col < n.unsqueeze(1)
        self.row = (offs[:-1].unsqueeze(1) + col).clamp_(max=max(int(offs[-1]) - 1, 0)) * self.valid
        self.bl, self.pl = torch.from_numpy(spec.bpnts).cuda(), torch.from_numpy(spec.ppnts).cuda()
        self.sd = (float(np.sqrt(spec.sigma[0])), float(np.sqrt(spec.sigma[1])))
        self.ramp = [float(v) for v in spec.ramp]

    def image(self, pts, detach=False):
        torch = self.torch
        b, x = pts[:, 0], pts[:, 1] - pts[:, 0]
        low, high, start, end = self.ramp
        w = torch.where(x < start, low, torch.where(x > end, high, (x - start) * (high - low) / (end - start) + low))
        bc, xc = (b.detach(), x.detach()) if detach else (b, x)
        phi = lambda z: torch.special.erfc(-z / 1.4142135623730951) / 2.0  # noqa: E731
        U = w.unsqueeze(1) * torch.diff(phi((self.bl.unsqueeze(0) - bc.unsqueeze(1)) / self.sd[0]), dim=1)
        V = torch.diff(phi((self.pl.unsqueeze(0) - xc.unsqueeze(1)) / self.sd[1]), dim=1)
        Up = U[self.row] * self.valid.unsqueeze(2)
        return torch.einsum("blr,blc->brc", Up, V[self.row]).reshape(self.valid.shape[0], -1)


def workload(torch, name, lens, spec, reps, inner, with_torch=True, with_vjp=False, seed=1):
    from tlc_gnn_amd import engine
    h_offs, h_pts = diagrams(lens, seed)
    offs, pts = torch.from_numpy(h_offs).cuda(), torch.from_numpy(h_pts).cuda()
    rb, rp = spec.resolution
    r = dict(diagrams=len(lens), points=int(h_offs[-1]), longest=int(lens.max()), median_length=float(np.median(lens)), resolution=[rb, rp],
             sigma=[float(v) for v in spec.sigma])
    img = engine.pi_image(offs, pts, spec)
    r["pi_image"] = timed(lambda: engine.pi_image(offs, pts, spec), reps, inner)
    r["pi_raster_default_5x5"] = timed(lambda: engine.pi_raster(offs, pts, 5), reps, inner)
    if with_torch:
        base = TorchImager(torch, offs, spec)
        with torch.no_grad():
            ref = base.image(pts)
            r["torch"] = timed(lambda: base.image(pts), reps, max(inner // 2, 1))
        r["max_abs_diff_torch"] = float((img - ref).abs().max())
        r["torch_over_pi_image"] = r["torch"]["median_s"] / r["pi_image"]["median_s"]
        del ref
    r["pi_image_over_pi_raster"] = r["pi_image"]["median_s"] / r["pi_raster_default_5x5"]["median_s"]
    if with_vjp:
        G = torch.from_numpy(np.random.RandomState(2).randn(len(lens), rb * rp)).cuda()
        for mode in ("weight", "full"):
            got = engine.pi_image_vjp(offs, pts, G, spec, mode)
            r["vjp_" + mode] = timed(lambda: engine.pi_image_vjp(offs, pts, G, spec, mode), reps, inner)
            if with_torch:
                x = pts.clone().requires_grad_(True)

                def fwd_bwd():
                    x.grad = None
                    (base.image(x, detach=(mode == "weight")) * G).sum().backward()
                r["torch_fwd_bwd_" + mode] = timed(fwd_bwd, reps, max(inner // 2, 1))
                r["vjp_%s_max_abs_diff_torch" % mode] = float((got - x.grad).abs().max())
        if rb == rp == 5:
            r["pi_raster_wgrad"] = timed(lambda: engine.pi_raster_wgrad(offs, pts, G, 5), reps, inner)
    torch.cuda.empty_cache()
    print("# %s: %s" % (name, r), file=sys.stderr, flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n-graphs", type=int, default=41127)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pimg_timing.json"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "time_pimg.py measures on the GPU; there is no CPU fallback"
    from tlc_gnn_amd import engine, synth
    _, _, no, eo = synth.hiv_shaped_molecules(a.n_graphs)
    mol = (np.diff(no) + np.diff(eo)).astype(np.int64)
    mid = np.random.RandomState(3).randint(300, 500, size=4096).astype(np.int64)
    small = lambda res: engine.PiSpec(lines(res), lines(res), sigma=(0.01, 0.01, 0.0))  # noqa: E731
    res = {"tool": "time_pimg", "reps": a.reps, "device": torch.cuda.get_device_name(0), "timer": "torch.cuda.Event around `inner` calls"}
    res["molecules_default_5x5"] = workload(torch, "molecules_default_5x5", mol, engine.PiSpec.default(5), a.reps, 10, with_vjp=True)
    res["molecules_20x20"] = workload(torch, "molecules_20x20", mol, small(20), a.reps, 10, with_vjp=True)
    res["molecules_50x50"] = workload(torch, "molecules_50x50", mol, small(50), a.reps, 6)
    res["mid_4096x400_50x50"] = workload(torch, "mid_4096x400_50x50", mid, small(50), a.reps, 6, with_vjp=True)
    res["one_70000_100x100"] = workload(torch, "one_70000_100x100", np.array([70000], dtype=np.int64), small(100), a.reps, 6, with_vjp=True)
    r5 = 0.5 * np.sqrt(0.01 * 0.02)
    corr = engine.PiSpec(lines(20), lines(20), sigma=(0.01, 0.02, r5))
    res["correlated_4096_molecules_20x20"] = workload(torch, "correlated_4096_molecules_20x20", mol[:4096], corr, a.reps, 3, with_torch=False,
                                                      with_vjp=False)
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())

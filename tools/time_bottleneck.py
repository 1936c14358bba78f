"""What the bottleneck distance costs (csrc/bottleneck.hip) -> profiles/bottleneck_timing.json.

One MI355X, device events around one call, the median of five windows (three where a call takes more than 2 s, one above 20 s).
Parts, the JSON rewritten after each:
  hiv      one (predicted, target) diagram pair per HIV-shaped molecule of synth.hiv_shaped_molecules(): as many points on each side
           as the molecule has edges, random coordinates (the pairs of tools/time_sliced_w.py): tlc_bottleneck_matching with both
           gradients; tlc_w2_inference_matching (order 1, with its gradient) on the same pairs in the same run; the host route -- the
           threshold search with scipy's bipartite matcher of tests/bottleneck_cases.py -- on the first --host-pairs pairs, whose
           values are compared with the device's (==);
  n1024, n2048, n4096   one random pair of that many rows (n = m = N / 2, the `pair` of tests/bottleneck_cases.py): the same three; at
           4 096 rows without the host route (scipy's matcher needs minutes there): the device's matching is checked to attain the value.

    python tools/time_bottleneck.py [--parts hiv,n1024,n2048,n4096] [--n-graphs 41127] [--host-pairs 1000] [--out profiles/bottleneck_timing.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bottleneck_cases as cases  # noqa: E402


def windows(torch, call):
    """-> (median ms, all ms, the last result): one call per window between two device events"""
    def once():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = call()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), r
    first, r = once()                                                # (warm-up: the first launch of a kernel loads its code object)
    reps = 5 if first < 2e3 else (3 if first < 2e4 else 1)
    ms = [once()[0] for _ in range(reps)] if first < 2e4 else [first]
    return float(np.median(ms)), [float(v) for v in ms], r


def note(msg):
    print("# " + msg, file=sys.stderr, flush=True)


def measure(torch, xoff, X, yoff, Y, host_problems):
    from tlc_gnn_amd import ops
    out = {}
    out["bottleneck_ms"], out["bottleneck_ms_all"], r = windows(torch, lambda: ops.bottleneck_matching(xoff, X, yoff, Y, want_grad=True, grad_target=True,
                                                                                                         check=False))
    out["status_ok"] = bool((r["status"] == 0).all())
    note("tlc_bottleneck_matching: %.3f ms" % out["bottleneck_ms"])
    out["w2_inference_ms"], out["w2_inference_ms_all"], w = windows(torch, lambda: ops.w2_inference_matching(xoff, X, yoff, Y, order=1, want_grad=True))
    out["w2_status_ok"] = bool((w["status"] == 0).all())
    note("tlc_w2_inference_matching: %.3f ms" % out["w2_inference_ms"])
    dist, w1 = r["dist"].cpu().numpy(), w["loss"].cpu().numpy()
    counts = (xoff[1:] - xoff[:-1] + yoff[1:] - yoff[:-1]).cpu().numpy()
    # d_B <= W_1 <= N d_B (to rounding of the sum)
    out["between_w1_bounds"] = bool((dist <= w1 * (1 + 1e-12)).all() and (w1 <= dist * counts * (1 + 1e-12) + 1e-300).all())
    if not host_problems:
        # (scipy's matcher takes 20 s and more for ONE threshold close to d_B of a 4 096-row pair, and the search visits twenty)
        out["host_pairs"], out["host_ms"], out["host_equal"] = 0, None, True
        # the witness stands in for the host's value: a perfect matching whose largest cost is the distance
        n, m = int(xoff[1] - xoff[0]), int(yoff[1] - yoff[0])
        worst = cases.check_matching(X[:n].cpu().numpy(), Y[:m].cpu().numpy(), r["assign_x"][:n].cpu().numpy(), r["assign_y"][:m].cpu().numpy())
        out["witness_attains_distance"] = bool(worst == dist[0])
        return out
    t = time.time()
    host = [cases.bottleneck(x, y) for x, y in host_problems]
    out["host_pairs"], out["host_ms"] = len(host), (time.time() - t) * 1e3
    out["host_ms_per_pair"] = out["host_ms"] / max(len(host), 1)
    out["host_equal"] = bool(np.array_equal(np.asarray(host, dtype=np.float64), dist[:len(host)]))
    note("host route: %.1f ms for %d pairs" % (out["host_ms"], len(host)))
    return out


def hiv(torch, n_graphs, host_pairs):
    from tlc_gnn_amd import synth
    _, _, _, eo = synth.hiv_shaped_molecules(n_graphs)
    rs = np.random.RandomState(1)

    def dgm(k):
        b = rs.random_sample(k)
        return np.stack([b, b + rs.random_sample(k)], 1)
    eo = np.ascontiguousarray(eo, dtype=np.int64)
    Xh, Yh = dgm(int(eo[-1])), dgm(int(eo[-1]))
    offs = torch.from_numpy(eo).cuda()
    sizes = 2 * np.diff(eo)
    out = dict(pairs=len(eo) - 1, points_per_side=int(eo[-1]), largest_pair=int(sizes.max()), median_pair=float(np.median(sizes)))
    k = min(host_pairs, len(eo) - 1)
    out.update(measure(torch, offs, torch.from_numpy(Xh).cuda(), offs, torch.from_numpy(Yh).cuda(),
                       [(Xh[eo[b]:eo[b + 1]], Yh[eo[b]:eo[b + 1]]) for b in range(k)]))
    out["host_ms_all_pairs_extrapolated"] = out["host_ms_per_pair"] * out["pairs"]
    return out


HOST_MAX_ROWS = 2048          # the host route is timed up to here


def one_pair(torch, N):
    rs = np.random.RandomState(N)
    Xh, Yh = cases.pair(rs, N // 2, N - N // 2)
    Xh[:, 1] = Xh[:, 0] + np.abs(Xh[:, 1] - Xh[:, 0])                # (no point below the diagonal: the order-1 loss keeps that sign)
    o = lambda k: torch.tensor([0, k], dtype=torch.int64).cuda()
    out = dict(rows=N, n=len(Xh), m=len(Yh))
    out.update(measure(torch, o(len(Xh)), torch.from_numpy(Xh).cuda(), o(len(Yh)), torch.from_numpy(Yh).cuda(), [(Xh, Yh)] if N <= HOST_MAX_ROWS else []))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="hiv,n1024,n2048,n4096")
    ap.add_argument("--n-graphs", type=int, default=41127)
    ap.add_argument("--host-pairs", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bottleneck_timing.json"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "time_bottleneck.py measures on the GPU; there is no CPU fallback"
    res = {"tool": "time_bottleneck", "device": torch.cuda.get_device_name(0), "timer": "torch.cuda.Event around one call, median of the windows"}
    for part in a.parts.split(","):
        res[part] = hiv(torch, a.n_graphs, a.host_pairs) if part == "hiv" else one_pair(torch, int(part[1:]))
        print("# %s: %s" % (part, res[part]), file=sys.stderr, flush=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    ok = all(v["status_ok"] and v["host_equal"] and v["between_w1_bounds"] and v.get("witness_attains_distance", True)
             for k, v in res.items() if isinstance(v, dict))
    res["all_checks_pass"] = bool(ok)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

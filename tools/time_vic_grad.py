"""What learning the curvature costs (csrc/vic_grad.hip, topo.VicinityImages, pipelines.train_curvature) on the PubMed-shaped graph
with its 37 676 training positives at hop 2, on one MI355X:
  structure      the one-off build of topo.VicinityStructure (two extractions, the lookup, the segment index), wall clock;
  segments       the histogram of segment lengths (copies of a graph edge among the packed vicinity edges): min, median, p99, max and
                 the share of segments and of entries per class -- what the cuts TLC_SEG_LANE_MAX / TLC_SEG_WAVE_MAX are judged by;
  segment_sum    tlc_segment_sum_f64 alone against torch's index_add_ (floating-point atomics) on the same data;
  decoder        tlc_lp_decode_bwd_pi_f32 alone against the existing tlc_lp_decode_bwd_f32;
  images         a whole VicinityImages forward + backward (--image-pairs of the positives: the diagrams of the largest vicinities
                 go through the host under pd_large='host');
  step           a whole train_curvature step against pipelines.train on a stored table (same pairs).
Device events around each window of --calls calls, the median of --reps windows after a warm-up window, per call.  A step that fails
is recorded as its error text and ends the run.  Prints ONE JSON line and writes it to --out.

  python tools/time_vic_grad.py [--reps 5] [--calls 3] [--image-pairs 4096] [--out profiles/vic_grad_timing.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def windows_median_ms(fn, reps, calls):
    """median over `reps` windows of (device time of `calls` calls) / calls, after one warm-up window"""
    import torch
    ms = []
    for w in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        if w:
            ms.append(e0.elapsed_time(e1) / calls)
    return float(np.median(ms)), [round(x, 4) for x in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--image-pairs", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vic_grad_timing.json"))
    a = ap.parse_args()
    import torch
    import bench
    from tlc_gnn_amd import _lib, engine, ops, pipelines, topo
    from tlc_gnn_amd.baselines import TLCGNN
    from tlc_gnn_amd.data import Data
    res = dict(tool="time_vic_grad", reps=a.reps, calls_per_window=a.calls, device=torch.cuda.get_device_name(0))
    wl = bench.build_workload(0)
    n, ge, pos = wl["n"], wl["train_edges"].astype(np.int32), wl["pi_pairs"]
    step = "structure"
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        S = topo.VicinityStructure(n, ge, pos, wl["hop"], flags=0)
        torch.cuda.synchronize()
        res["structure"] = dict(pairs=len(pos), graph_edges=len(ge), rows=int(S.rows.numel()), packed_nodes=int(S.ids.numel()),
                                packed_edges=int(S.eid.numel()), build_wall_ms=1e3 * (time.perf_counter() - t0))
        step = "segments"
        L = np.diff(S.seg_ptr.cpu().numpy())
        lane, wave = L <= _lib.SEG_LANE_MAX, (L > _lib.SEG_LANE_MAX) & (L <= _lib.SEG_WAVE_MAX)
        res["segments"] = dict(min=int(L.min()), median=float(np.median(L)), p99=float(np.percentile(L, 99)), max=int(L.max()), empty=int((L == 0).sum()),
                               share_of_segments=dict(lane=float(lane.mean()), wavefront=float(wave.mean()), workgroup=float((~lane & ~wave).mean())),
                               share_of_entries=dict(lane=float(L[lane].sum() / L.sum()), wavefront=float(L[wave].sum() / L.sum()),
                                                     workgroup=float(L[~lane & ~wave].sum() / L.sum())))
        step = "segment_sum"
        g = torch.from_numpy(np.random.default_rng(1).normal(size=S.eid.numel())).cuda()
        work = torch.empty(engine.segment_sum_work_bytes(len(ge)) + 255, dtype=torch.uint8, device="cuda")
        out = torch.empty(len(ge), dtype=torch.float64, device="cuda")
        eid64 = S.eid.long()
        r = dict(entries=int(S.eid.numel()), segments=len(ge))
        r["segment_sum_ms"], r["segment_sum_ms_all"] = windows_median_ms(lambda: engine.segment_sum(g, S.seg_ptr, S.seg_pos, work=work, out=out), a.reps, a.calls)
        r["index_add_ms"], r["index_add_ms_all"] = windows_median_ms(lambda: torch.zeros(len(ge), dtype=torch.float64, device="cuda").index_add_(0, eid64, g),
                                                                     a.reps, a.calls)
        r["ratio_to_index_add"] = r["segment_sum_ms"] / r["index_add_ms"]
        ref = torch.zeros(len(ge), dtype=torch.float64, device="cuda").index_add_(0, eid64, g)
        r["worst_abs_diff_to_index_add"] = float((engine.segment_sum(g, S.seg_ptr, S.seg_pos) - ref).abs().max())
        res["segment_sum"] = r
        step = "decoder"
        rs = np.random.RandomState(7)
        E = 2 * len(pos)
        pairs = torch.from_numpy(np.concatenate([pos, wl["neg"]]).astype(np.int32)).cuda()
        emb = torch.from_numpy(rs.normal(0, 0.6, size=(n, 16)).astype(np.float32)).cuda()
        post = ops.renorm_rows_(emb.clone())
        pi = torch.from_numpy(rs.uniform(0, 0.3, size=(E, 25)).astype(np.float32)).cuda()
        w1, b1 = torch.from_numpy(rs.normal(0, 0.3, size=(25, 41)).astype(np.float32)).cuda(), torch.zeros(25, device="cuda")
        w2, b2 = torch.from_numpy(rs.normal(0, 0.3, size=(1, 25)).astype(np.float32)).cuda(), torch.zeros(1, device="cuda")
        gp = torch.from_numpy(rs.normal(size=E).astype(np.float32)).cuda()
        groups = ops.endpoint_groups(pairs, n)
        r = dict(pairs=E)
        r["bwd_pi_ms"], r["bwd_pi_ms_all"] = windows_median_ms(lambda: engine.lp_decode_bwd_pi(pairs, emb, post, pi, w1, b1, w2, b2, gp), a.reps, a.calls)
        r["existing_bwd_ms"], r["existing_bwd_ms_all"] = windows_median_ms(
            lambda: ops.lp_decode_bwd(pairs, emb, post, pi, w1, b1, w2, b2, gp, groups=groups), a.reps, a.calls)
        res["decoder"] = r
        step = "images"
        k = min(a.image_pairs, len(pos))
        mod = topo.VicinityImages(n, ge, pos[:k], wl["hop"], flags=0)
        with torch.no_grad():
            mod.kappa.copy_(torch.from_numpy(np.random.default_rng(3).uniform(-0.4, 0.6, len(ge))))
        G = torch.from_numpy(np.random.default_rng(4).normal(size=(k, 25))).cuda()

        def fwd_bwd():
            mod.kappa.grad = None
            (mod()[0] * G).sum().backward()
        r = dict(pairs=k, packed_edges=int(mod.structure.eid.numel()))
        r["forward_backward_ms"], r["forward_backward_ms_all"] = windows_median_ms(fwd_bwd, a.reps, 1)
        with torch.no_grad():
            r["forward_ms"], r["forward_ms_all"] = windows_median_ms(lambda: mod(), a.reps, 1)
        res["images"] = r
        step = "step"
        tp = k // 2
        prs = np.concatenate([pos[:tp], wl["neg"][:tp]]).astype(np.int64)
        y = torch.cat((torch.ones(tp), torch.zeros(tp))).long()
        te = wl["train_edges"]
        data = Data(x=torch.from_numpy(wl["x"]), edge_index=torch.from_numpy(np.concatenate([te, te[:, ::-1]]).T.copy()).long(), y=torch.zeros(n),
                    total_edges=prs, total_edges_y=y, train_pos=tp, train_neg=tp, val_pos=0, val_neg=0, test_pos=0, test_neg=0)
        images = topo.VicinityImages(n, ge, prs, wl["hop"], flags=0)
        with torch.no_grad():
            table = images()[0]
        pipelines.setup_seed(3)
        model = TLCGNN.Net(data, wl["n_feat"], 2, PI=table)
        model.apply(pipelines.weights_init)
        model, data = model.cuda(), data.to("cuda")
        opt_a = torch.optim.Adam(model.parameters(), lr=0.01)
        opt_b = torch.optim.Adam([{"params": model.parameters()}, {"params": [images.kappa], "lr": 1e-3}], lr=0.01)
        r = dict(pairs=2 * tp)
        r["train_stored_table_ms"], r["train_stored_table_ms_all"] = windows_median_ms(lambda: pipelines.train(model, data, opt_a), a.reps, 1)
        r["train_curvature_ms"], r["train_curvature_ms_all"] = windows_median_ms(lambda: pipelines.train_curvature(model, data, opt_b, images), a.reps, 1)
        res["step"] = r
    except Exception as exc:                                                   # noqa: BLE001 (the figures so far are still worth keeping)
        res["failed_step"] = step
        res["error"] = "%s: %s" % (type(exc).__name__, exc)
    line = json.dumps(res)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    print(line)
    return 1 if "error" in res else 0


if __name__ == "__main__":
    sys.exit(main())

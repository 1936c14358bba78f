"""What the teacher's message-passing baselines cost (csrc/gnn_layers.hip) -> profiles/gnn_baselines_timing.json.

One MI355X, device events around one call, the median of five windows, every route in the same run.  Parts, the JSON rewritten after each:
  hiv      the 41 127 HIV-shaped molecule graphs of synth.hiv_shaped_molecules() as one block-diagonal batch (both orientations, the
           self loops last): the eval forward of Teacher_Model (compute_loss=False, grad_PI=False, the batch's structure held by the
           caller) for 'GIN', 'GCN', 'SAGE' and 'GAT' (tlc_pdgnn_forward); the four layers alone, as the one-launch stack
           (tlc_gnn_stack_fwd) and layer by layer (4 x tlc_gnn_layer_fwd); and the same three models written in torch ops (index_add_ +
           F.linear, the structure and gcn_norm precomputed once per batch, the same edge head and imager), whose points are compared;
  amazon   the 4 096 hop-1 vicinities of the Photo-shaped graph, stacked (data_utils_LP.stacked): the same routes;
  train    one training step (forward, kernel='wasserstein' p = 2, backward) on the first 4 096 HIV-shaped graphs, dropout 0: the HIP
           layers (autograd.GnnLayer) against the torch formulation under torch's autograd, both with the device matching loss.

    python tools/time_gnn_baselines.py [--parts hiv,amazon,train] [--n-graphs 41127] [--out profiles/gnn_baselines_timing.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KINDS = ("GIN", "GCN", "SAGE")


def windows(torch, call, reps=5):
    def once():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = call()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), r
    _, r = once()                                                    # (warm-up: the first launch of a kernel loads its code object)
    ms = [once()[0] for _ in range(reps)]
    return float(np.median(ms)), [float(v) for v in ms], r


def note(msg):
    print("# " + msg, file=sys.stderr, flush=True)


class TorchBaseline:
    """The same model in torch ops on the device: index_add_ on the edge list + F.linear, sharing the HIP model's parameters."""

    def __init__(self, torch, model, kind, ei, n):
        import torch.nn.functional as F
        self.t, self.F, self.m, self.kind, self.n = torch, F, model, kind, n
        self.src, self.dst = ei[0], ei[1]
        if kind == "GCN":                                           # gcn_norm (PD_conv.py:35-70), once per batch
            keep = ei[0] != ei[1]
            loop = torch.arange(n, device=ei.device)
            self.src, self.dst = torch.cat([ei[0][keep], loop]), torch.cat([ei[1][keep], loop])
            deg = torch.zeros(n, device=ei.device).index_add_(0, self.dst, torch.ones(self.dst.numel(), device=ei.device))
            dis = deg.pow(-0.5)
            dis[dis == float("inf")] = 0
            self.norm = (dis[self.src] * dis[self.dst])[:, None]
        if kind == "SAGE":
            deg = torch.zeros(n, device=ei.device).index_add_(0, self.dst, torch.ones(self.dst.numel(), device=ei.device))
            self.inv = (1.0 / deg.clamp(min=1))[:, None]

    def layer(self, conv, x):
        t, F = self.t, self.F
        if self.kind == "GIN":
            agg = x + t.zeros_like(x).index_add_(0, self.dst, x[self.src])
            h = F.linear(agg, conv.nn[0].weight, conv.nn[0].bias)
            return F.relu(h) if conv.relu else h
        if self.kind == "GCN":
            xw = x @ conv.weight
            return t.zeros_like(xw).index_add_(0, self.dst, self.norm * xw[self.src]) + conv.bias
        mean = t.zeros_like(x).index_add_(0, self.dst, x[self.src]) * self.inv
        return F.linear(mean, conv.lin_l.weight, conv.lin_l.bias) + F.linear(x, conv.lin_r.weight)

    def stack(self, x):
        d, F = self.m.DIM0_Model, self.F
        slope = self.t.tensor(0.1, device=x.device)
        for k, conv in enumerate((d.conv1, d.conv2, d.conv4, d.conv3)):
            x = self.layer(conv, x)
            if self.kind != "GIN" and k < 3:
                x = F.prelu(x, slope)
        return x

    def forward(self, x, ei, m):
        F = self.F
        h = self.stack(x)
        cat = self.t.cat((h[ei[0, :m]], h[ei[1, :m]]), dim=1)
        hid = F.prelu(F.linear(cat, self.m.lin5.weight, self.m.lin5.bias), self.t.tensor(0.1, device=x.device))
        return F.linear(hid, self.m.lin6.weight, self.m.lin6.bias)


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / max(1e-12, float(b.double().abs().max())))


def measure_forward(torch, x, ei, gptr, eptr):
    """Every route's eval forward on one batch: x f32 [n, 1], ei int64 [2, m + n] (loops last), node / edge offsets."""
    from tlc_gnn_amd import engine, ops
    from tlc_gnn_amd.Knowledge_Distillation.Teacher_model import Teacher_Model
    from tlc_gnn_amd.Knowledge_Distillation.gat_conv import GraphBatch
    from tlc_gnn_amd.Knowledge_Distillation.gnn_layers import GnnBatch
    n, m = x.shape[0], ei.shape[1] - x.shape[0]
    out = dict(nodes=n, edges=m, graphs=int(gptr.numel()) - 1)
    call = lambda model, csr: model(x, ei, None, compute_loss=False, grad_PI=False, graph_ptr=gptr, edge_ptr=eptr, csr=csr)
    with torch.no_grad():
        torch.manual_seed(1234)
        gat = Teacher_Model(type='GAT').eval().cuda()
        held = GraphBatch(ei, n)
        out["GAT_ms"], out["GAT_ms_all"], _ = windows(torch, lambda: call(gat, held))
        note("GAT (tlc_pdgnn_forward): %.3f ms" % out["GAT_ms"])
        for kind in KINDS:
            torch.manual_seed(1234)
            model = Teacher_Model(type=kind).eval().cuda()
            r = {}
            r["batch_build_ms"], _, b = windows(torch, lambda: GnnBatch(ei, n, kind), reps=3)
            r["tiles"] = None if b.tiles is None else int(b.tiles.numel()) - 1
            r["forward_ms"], r["forward_ms_all"], res = windows(torch, lambda: call(model, b))
            d = model.DIM0_Model
            layers = [c.layer(s) for c, s in zip((d.conv1, d.conv2, d.conv4, d.conv3), ((-1.0 if kind == "GIN" else 0.1),) * 3 + (-1.0,))]

            def by_layer():
                h = x
                for wa, ws, bias, act, slope in layers:
                    h = ops.gnn_layer(b.rowptr, b.src, b.coef, b.self_scale, h, wa, ws, bias, act, slope)
                return h
            r["layers_ms"], r["layers_ms_all"], hl = windows(torch, by_layer)
            if b.tiles is not None:
                r["stack_ms"], r["stack_ms_all"], hs = windows(torch, lambda: ops.gnn_stack(b.rowptr, b.src, b.coef, b.self_scale, b.tiles, x, layers))
                r["stack_equals_layers"] = bool(torch.equal(hs, hl))
            tb = TorchBaseline(torch, model, kind, ei, n)
            r["torch_layers_ms"], r["torch_layers_ms_all"], ht = windows(torch, lambda: tb.stack(x))

            def torch_forward():
                pts = tb.forward(x, ei, m)
                return pts, engine.pi_raster(eptr, pts.to(torch.float64), 5)
            r["torch_forward_ms"], r["torch_forward_ms_all"], (pts, _) = windows(torch, torch_forward)
            r["layers_rel_diff_vs_torch"], r["points_rel_diff_vs_torch"] = rel(hl, ht), rel(res[0], pts)
            note("%s: forward %.3f ms (stack %s ms, layer by layer %.3f ms); torch ops: forward %.3f ms, layers %.3f ms; GnnBatch %.3f ms"
                 % (kind, r["forward_ms"], r.get("stack_ms"), r["layers_ms"], r["torch_forward_ms"], r["torch_layers_ms"], r["batch_build_ms"]))
            out[kind] = r
    return out


def hiv_batch(torch, n_graphs):
    from tlc_gnn_amd import synth
    e_all, f, node_offs, edge_offs = synth.hiv_shaped_molecules(n_graphs, 1234)
    glob = e_all.astype(np.int64) + np.repeat(node_offs[:-1], np.diff(edge_offs))[:, None]
    both = np.concatenate([glob, glob[:, ::-1]])
    both = both[np.argsort(np.searchsorted(node_offs[1:], both[:, 0], side="right"), kind="stable")]
    eptr = np.concatenate([[0], np.cumsum(2 * np.diff(edge_offs))]).astype(np.int64)
    loops = np.arange(int(node_offs[-1]))
    ei = torch.from_numpy(np.concatenate([both, np.stack([loops, loops], 1)]).T.copy()).cuda()
    x = torch.from_numpy(f.astype(np.float32)).view(-1, 1).cuda()
    return x, ei, torch.from_numpy(node_offs.astype(np.int64)).cuda(), torch.from_numpy(eptr).cuda()


def amazon_batch(torch, n_pairs=4096, seed=1234):
    from tlc_gnn_amd import synth
    from tlc_gnn_amd.Knowledge_Distillation.data_utils_LP import Vicinities, stacked
    n, edges, kappa, hop, _ = synth.shaped_graph("Photo")
    ricci = np.concatenate([np.concatenate([edges, kappa[:, None]], 1), np.concatenate([edges[:, ::-1], kappa[:, None]], 1)]).tolist()
    vic = Vicinities(edges, ricci)
    pairs = edges[np.random.RandomState(seed).permutation(len(edges))[:n_pairs]]
    b = vic.batch(pairs, hop, node_cap=512, edge_cap=8192)
    x, ei = stacked(b)
    return x, ei, b["node_ptr"], b["edge_ptr"]


def measure_train(torch, x, ei, gptr, eptr):
    """One training step per type: the HIP layers against the torch formulation, the same device loss."""
    from tlc_gnn_amd import autograd
    from tlc_gnn_amd.Knowledge_Distillation.Teacher_model import Teacher_Model
    n, m = x.shape[0], ei.shape[1] - x.shape[0]
    rs = np.random.RandomState(7)
    bb = rs.rand(m)
    PD = torch.tensor(np.stack([bb, bb + rs.uniform(0, 0.6, size=m)], 1), dtype=torch.float32).cuda()
    out = dict(nodes=n, edges=m, graphs=int(gptr.numel()) - 1)
    for kind in KINDS:
        torch.manual_seed(1234)
        model = Teacher_Model(type=kind, dropout=0.0).cuda().train()
        tb = TorchBaseline(torch, model, kind, ei, n)

        def hip_step():
            model.zero_grad(set_to_none=True)
            loss = model(x, ei, PD, kernel='wasserstein', p=2, grad_PI=False, graph_ptr=gptr, edge_ptr=eptr)[2]
            loss.backward()
            return loss.detach()

        def torch_step():
            model.zero_grad(set_to_none=True)
            pts = tb.forward(x, ei, m)
            loss = autograd.diagram_loss(pts, PD.to(torch.float64), order=2, xoff=eptr, yoff=eptr)[0].sum()
            loss.backward()
            return loss.detach()
        r = {}
        r["hip_step_ms"], r["hip_step_ms_all"], lh = windows(torch, hip_step)
        r["torch_step_ms"], r["torch_step_ms_all"], lt = windows(torch, torch_step)
        r["loss_rel_diff"] = rel(lh.reshape(-1), lt.reshape(-1))
        note("%s training step: HIP layers %.3f ms, torch ops %.3f ms" % (kind, r["hip_step_ms"], r["torch_step_ms"]))
        out[kind] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="hiv,amazon,train")
    ap.add_argument("--n-graphs", type=int, default=41127)
    ap.add_argument("--train-graphs", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gnn_baselines_timing.json"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "time_gnn_baselines.py measures on the GPU; there is no CPU fallback"
    res = {"tool": "time_gnn_baselines", "device": torch.cuda.get_device_name(0), "timer": "torch.cuda.Event around one call, median of five windows"}
    for part in a.parts.split(","):
        if part == "hiv":
            res[part] = measure_forward(torch, *hiv_batch(torch, a.n_graphs))
        elif part == "amazon":
            res[part] = measure_forward(torch, *amazon_batch(torch))
        else:
            res[part] = measure_train(torch, *hiv_batch(torch, a.train_graphs))
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())

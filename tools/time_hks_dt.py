"""What the derivative in the diffusion time costs: tlc_hks_batch_dt and tlc_hks_large_batch_dt against their parents in the same
run, one learned-time step end to end, and the baseline a user would write without this library.  Each step runs in a child process
of its own under its own time limit (a step that fails or runs out of time ends the run; nothing is started after it):
  jacobi    the 41 127 HIV-shaped molecule graphs of tools/time_hks.py, times 0.1 and 10 in one call: engine.hks_batch against
            engine.hks_batch(dt=True);
  large     the PubMed-shaped hop-2 vicinities above TLC_HKS_NMAX nodes of tools/time_hks_large.py, per time 0.1 and 10:
            engine.hks_large_batch against engine.hks_large_batch(dout=True);
  step      one topo.images(topo.hks_filtration(t, ...)) forward + backward on the HIV-shaped graphs, t = 1, and its parts
            (autograd.hks_signature alone, forward + backward);
  baseline  the normalised signature and its gradient in t by a padded batched torch.linalg.eigh with autograd on the same GPU, on the
            first --baseline-graphs of the HIV-shaped graphs, against autograd.hks_signature on the same graphs.
Device events around each window of --calls calls, the median of --reps windows after a warm-up window, per call.
Prints ONE JSON line and writes it to --out.

  python tools/time_hks_dt.py [--reps 5] [--calls 3] [--limit 300] [--out profiles/hks_dt_timing.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TIMES = (0.1, 10.0)


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


def hiv_packed(n_graphs):
    import torch
    from tlc_gnn_amd import synth
    edges, _, node_offs, edge_offs = synth.hiv_shaped_molecules(41127)
    node_offs, edge_offs = node_offs[:n_graphs + 1], edge_offs[:n_graphs + 1]
    edges = edges[:edge_offs[-1]]
    return torch.from_numpy(node_offs).cuda(), torch.from_numpy(edge_offs).cuda(), torch.from_numpy(edges).cuda(), node_offs, edge_offs, edges


def step_jacobi(a):
    from tlc_gnn_amd import engine
    no, eo, E, nptr, _, _ = hiv_packed(41127)
    tot = int(nptr[-1])
    r = dict(graphs=len(nptr) - 1, nodes=tot, times=list(TIMES))
    r["hks_batch_ms"], r["hks_batch_ms_all"] = windows_median_ms(lambda: engine.hks_batch(no, eo, E, list(TIMES), total_nodes=tot), a.reps, a.calls)
    r["hks_batch_dt_ms"], r["hks_batch_dt_ms_all"] = windows_median_ms(lambda: engine.hks_batch(no, eo, E, list(TIMES), total_nodes=tot, dt=True),
                                                                     a.reps, a.calls)
    r["dt_over_parent"] = r["hks_batch_dt_ms"] / r["hks_batch_ms"]
    return r


def step_large(a):
    from tlc_gnn_amd import engine, synth, _lib
    from tlc_gnn_amd.Knowledge_Distillation import data_utils_NC as kd_nc
    _, edges, _, _, _ = synth.shaped_graph("PubMed")
    vic = kd_nc.NodeVicinities(edges, None)
    b = vic.batch(np.random.RandomState(0).permutation(np.unique(edges))[:a.n_queries], 2, filt='degree')
    no, eo, E = b["node_ptr"], b["edge_ptr"], b["edges"].contiguous()
    sizes = np.diff(no.cpu().numpy())
    m_of = np.diff(eo.cpu().numpy())
    sel = np.nonzero((sizes > _lib.HKS_NMAX) & (sizes <= _lib.HKS_LARGE_NMAX))[0]
    tot = int(sizes.sum())
    r = dict(graphs=int(len(sel)), n_max=int(sizes[sel].max()), n_median=float(np.median(sizes[sel])), edges=int(m_of[sel].sum()))
    for t in TIMES:
        run = lambda dout: engine.hks_large_batch(no, eo, E, sel.tolist(), sizes[sel].tolist(), [t], total_nodes=tot, dout=dout)
        p, p_all = windows_median_ms(lambda: run(None), a.reps, a.calls)
        d, d_all = windows_median_ms(lambda: run(True), a.reps, a.calls)
        r["t=%g" % t] = dict(hks_large_batch_ms=p, hks_large_batch_ms_all=p_all, hks_large_batch_dt_ms=d, hks_large_batch_dt_ms_all=d_all,
                             dt_over_parent=d / p)
    return r


def step_step(a):
    import torch
    from tlc_gnn_amd import autograd, topo
    no, eo, E, nptr, _, _ = hiv_packed(41127)
    t = torch.tensor(1.0, dtype=torch.float64, device="cuda", requires_grad=True)

    def full():
        t.grad = None
        topo.images(topo.hks_filtration(t, no, eo, E), no, eo, E).sum().backward()

    def signature():
        t.grad = None
        autograd.hks_signature(t.reshape(1), no, eo, E).sum().backward()

    r = dict(graphs=len(nptr) - 1, time=1.0)
    r["images_of_hks_filtration_fwd_bwd_ms"], r["images_of_hks_filtration_fwd_bwd_ms_all"] = windows_median_ms(full, a.reps, 1)
    r["hks_signature_fwd_bwd_ms"], r["hks_signature_fwd_bwd_ms_all"] = windows_median_ms(signature, a.reps, a.calls)
    return r


def step_baseline(a):
    import torch
    from tlc_gnn_amd import autograd
    B = a.baseline_graphs
    no, eo, E, nptr, eptr, e = hiv_packed(B)
    n_of = np.diff(nptr)
    nmax = int(n_of.max())
    owner = np.repeat(np.arange(B), np.diff(eptr))
    A = torch.zeros(B, nmax, nmax, dtype=torch.float64, device="cuda")
    ow, ea, eb = (torch.from_numpy(x.astype(np.int64)).cuda() for x in (owner, e[:, 0], e[:, 1]))
    A[ow, ea, eb] = 1.0
    A[ow, eb, ea] = 1.0
    deg = A.sum(2)
    s = torch.where(deg > 0, deg.clamp(min=1.0).rsqrt(), torch.zeros_like(deg))
    # padding rows get a diagonal of 3 (outside the spectrum's [0, 2]) and are masked out of the signature
    real = torch.arange(nmax, device="cuda")[None, :] < torch.from_numpy(n_of).cuda()[:, None]
    L = torch.diag_embed(torch.where(real, (deg > 0).to(torch.float64), torch.full_like(deg, 3.0))) - s[:, :, None] * A * s[:, None, :]
    t = torch.tensor(1.0, dtype=torch.float64, device="cuda", requires_grad=True)

    def eigh_route():
        t.grad = None
        lam, phi = torch.linalg.eigh(L)
        hks = ((phi * phi) * torch.exp(-t * lam)[:, None, :]).sum(2)
        hks = torch.where(real, hks, torch.zeros_like(hks))
        f = hks / (hks.max(1, keepdim=True).values + 1e-10)
        f[real].sum().backward()
        return f

    def ours():
        t.grad = None
        f = autograd.hks_signature(t.reshape(1), no, eo, E)
        f.sum().backward()
        return f

    fa = eigh_route()
    ga = float(t.grad)
    fb = ours()
    gb = float(t.grad)
    r = dict(graphs=B, n_max=nmax, time=1.0, worst_abs_diff=float((fa[real] - fb[0]).detach().abs().max()), grad_eigh=ga, grad_hks_signature=gb)
    r["eigh_autograd_fwd_bwd_ms"], r["eigh_autograd_fwd_bwd_ms_all"] = windows_median_ms(eigh_route, a.reps, 1)
    r["hks_signature_fwd_bwd_ms"], r["hks_signature_fwd_bwd_ms_all"] = windows_median_ms(ours, a.reps, a.calls)
    r["eigh_over_hks_signature"] = r["eigh_autograd_fwd_bwd_ms"] / r["hks_signature_fwd_bwd_ms"]
    return r


STEPS = {"jacobi": step_jacobi, "large": step_large, "step": step_step, "baseline": step_baseline}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="windows per figure")
    ap.add_argument("--calls", type=int, default=3, help="calls per window")
    ap.add_argument("--n-queries", type=int, default=4096)
    ap.add_argument("--baseline-graphs", type=int, default=4096)
    ap.add_argument("--limit", type=float, default=300.0, help="seconds each step may take")
    ap.add_argument("--steps", default="jacobi,large,step,baseline")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hks_dt_timing.json"))
    ap.add_argument("--step", default=None, help="(internal) run one step in this process and print its JSON")
    a = ap.parse_args()
    if a.step:
        import torch
        assert torch.cuda.is_available(), "time_hks_dt.py measures on the GPU; there is no CPU fallback"
        r = STEPS[a.step](a)
        r["device"] = torch.cuda.get_device_name(0)
        print("RESULT " + json.dumps(r), flush=True)
        return 0
    res = {"tool": "time_hks_dt", "reps": a.reps, "calls_per_window": a.calls}
    for step in a.steps.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(a.reps), "--calls", str(a.calls),
               "--n-queries", str(a.n_queries), "--baseline-graphs", str(a.baseline_graphs)]
        t0 = time.perf_counter()
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print("# step %s ran out of its %g s: stopping" % (step, a.limit), file=sys.stderr)
            return 124
        if p.returncode != 0:
            print("# step %s ended with status %d: stopping" % (step, p.returncode), file=sys.stderr)
            return p.returncode if p.returncode > 0 else 1
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
        r = json.loads(line[len("RESULT "):])
        res["device"] = r.pop("device")
        res[step] = r
        print("# %s (%.1f s): %s" % (step, time.perf_counter() - t0, r), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

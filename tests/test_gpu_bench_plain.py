"""GPU: a plain `bench.py --gpus 1 --steps K --warmup W` prints the headline line and nothing that takes runs of its own (those sit
behind --full), starts no other program, and --dump-outputs writes what the timed region's last step computed."""
import gc
import json
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# what a --full run adds to the line: every one of these takes runs, child processes or host work beside the K timed steps
FULL_ONLY = ("timed_outputs_equal", "timed_outputs_checked", "config", "roofline", "roofline_issue", "roofline_chain", "roofline_lp",
             "rotated_batches", "same_batch_every_step", "strong_scaling", "kernel_ms", "sweep", "full_sweep", "ricci", "other_shapes",
             "pdgnn", "pdgnn_amazon", "cpu_baseline")


def test_plain_run_is_the_headline_alone(tmp_path, capsys, monkeypatch):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import bench
    from tlc_gnn_amd import engine

    def no_children(*a, **k):
        raise AssertionError("a plain run started another program: %r" % (a,))
    monkeypatch.setattr(subprocess, "Popen", no_children)
    monkeypatch.setattr(subprocess, "call", no_children)
    K, W = 4, 1                                        # (K - 1) % 3 == 0: the last step's buffer is the first of the three again
    dump = tmp_path / "dump"
    monkeypatch.setattr("sys.argv", ["bench.py", "--gpus", "1", "--steps", str(K), "--warmup", str(W), "--dump-outputs", str(dump)])
    bench.main()
    torch.cuda.synchronize()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 1                             # ONE line, and it is the JSON result
    out = json.loads(lines[0])
    assert out["metric"].startswith("persistence-images/sec") and out["unit"] == "persistence-images/sec"
    assert out["higher_is_better"] is True and out["dtype"] == "f64"
    assert out["n_gpus"] == 1 and out["steps"] == K and out["warmup"] == W and out["full"] is False
    assert out["value"] > 0 and out["ms_per_step"] > 0 and out["pi_ms_per_step"] > 0 and out["lp_ms_per_step"] > 0
    assert out["ms_per_step"] >= out["pi_ms_per_step"]                    # host wall clock of the region holds the image leg's device time
    assert np.isclose(out["value"], 37676 / (out["pi_ms_per_step"] * 1e-3), rtol=1e-9)
    assert not [k for k in FULL_ONLY if k in out]
    # the dump: the rows the region's last step wrote -- bit for bit those of a stream-ordered call on the same pairs (the check a
    # --full run makes itself), status bytes too; the last forward's probabilities
    wl = bench.build_workload(0)
    E = len(wl["pi_pairs"])
    pi, st, prob = (np.load(dump / (nm + ".npy")) for nm in ("pi_images", "pi_status", "lp_prob"))
    assert sorted(p.name for p in dump.iterdir()) == ["lp_prob.npy", "pi_images.npy", "pi_status.npy"]
    assert pi.shape == (E, 25) and pi.dtype == np.float64 and st.shape == (E,) and st.dtype == np.float32
    assert prob.shape == (2 * E,) and prob.dtype == np.float32
    g = engine.DeviceGraph(wl["rowptr"], wl["col"], wl["w"])
    ref_o, ref_s = g.pd_pi_batch(torch.from_numpy(wl["pi_pairs"]).cuda(), wl["hop"])
    assert np.array_equal(pi, ref_o.cpu().numpy())
    assert np.array_equal(st, ref_s.cpu().numpy().astype(np.float32))
    assert np.isfinite(prob).all() and prob.std() > 0
    g.close()
    gc.collect()                                        # (main()'s own handle goes with its closures)

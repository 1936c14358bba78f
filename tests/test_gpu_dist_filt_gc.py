"""GPU: filt='ricci' of the graph-classification drop-ins (data_utils_GC: compute_persistence_image, compute_persistence_image_batch, the
packed route) on molecule-sized graphs -- equal to each other and to the batch call fed the numpy restatement's values -- and the packed
curvature helper against per-graph curvature calls."""
import numpy as np
import pytest

import dist_filt_cases as dc

pytestmark = pytest.mark.gpu


def _molecules(n_graphs):
    """(n, edges[m, 2] each edge once lo < hi, kappa[m]) per graph, and each graph's curvature in the reference's list form"""
    from tlc_gnn_amd import synth
    edges, _, no, eo = synth.hiv_shaped_molecules(n_graphs, seed=7)
    rs = np.random.RandomState(3)
    graphs, curvs = [], []
    for g in range(n_graphs):
        e = edges[eo[g]:eo[g + 1]].astype(np.int64)
        k = rs.uniform(-0.5, 0.9, len(e))
        graphs.append((int(no[g + 1] - no[g]), e, k))
        curvs.append(sorted([[int(a), int(b), float(x)] for (a, b), x in zip(e.tolist(), k.tolist())] +
                            [[int(b), int(a), float(x)] for (a, b), x in zip(e.tolist(), k.tolist())]))
    return graphs, curvs


def _same(a, b, what):
    assert len(a) == len(b) == 9, what
    for j in (0, 1, 2, 5, 6):                                                 # d0, d1, the three images
        assert np.array_equal(np.asarray(a[j]), np.asarray(b[j])), (what, j)
    assert a[3] == b[3] and np.array_equal(a[4].numpy(), b[4].numpy()) and a[7:] == b[7:], what


def test_ricci_through_the_three_routes():
    import torch
    from tlc_gnn_amd.Knowledge_Distillation import data_utils_GC as kd
    graphs, curvs = _molecules(50)
    plain = [(n, e) for n, e, _ in graphs]
    want_f = [dc.forward(n, e, k + 1.0, 0, -1, dc.NORM_EPS | dc.UNREACHABLE_100)[0] for n, e, k in graphs]
    ref = kd.compute_persistence_image_batch(plain, filtrations=want_f)
    batch = kd.compute_persistence_image_batch(plain, filt='ricci', ricci_curv=curvs)
    packed = kd.pack_dataset(plain)
    kappa = torch.from_numpy(np.concatenate([k for _, _, k in graphs])).cuda()
    gt = kd.ground_truth_packed(*packed, filt='ricci', component='whole', kappa=kappa).tuples()
    assert all(len(r) == 9 for r in ref)
    for i, (n, e, k) in enumerate(graphs):
        _same(batch[i], ref[i], ("batch", i))
        _same(gt[i], ref[i], ("packed", i))
        as_dict = {(a, b): x for a, b, x in curvs[i]}
        _same(kd.compute_persistence_image((n, e), filt='ricci', ricci_curv=curvs[i] if i % 2 else as_dict), ref[i], ("single", i))
        f, ei = kd.compute_persistence_image((n, e), filt='ricci', ricci_curv=curvs[i], mode='filtration')
        assert f == want_f[i].tolist() and np.array_equal(ei.numpy(), e.T), i
    # the packed route reads RAW edges: both orientations, each carrying the pair's value
    both = [(n, np.concatenate([e, e[:, ::-1]])) for n, e, _ in graphs]
    kappa2 = torch.from_numpy(np.concatenate([np.concatenate([k, k]) for _, _, k in graphs])).cuda()
    gt2 = kd.ground_truth_packed(*kd.pack_dataset(both), filt='ricci', component='largest', kappa=kappa2).tuples()
    for i in range(50):
        _same(gt2[i], ref[i], ("packed raw", i))
    # the curvature stays an input: without it the call says so; unknown names are refused as before
    for call in (lambda: kd.compute_persistence_image(plain[0], filt='ricci'), lambda: kd.compute_persistence_image_batch(plain, filt='ricci'),
                 lambda: kd.ground_truth_packed(*packed, filt='ricci'), lambda: kd.compute_persistence_image(plain[0], filt='nope'),
                 lambda: kd.ground_truth_packed(*packed, filt='nope')):
        with pytest.raises(NotImplementedError):
            call()


def test_packed_curvature_equals_per_graph_calls():
    from tlc_gnn_amd import engine, synth
    from tlc_gnn_amd.Knowledge_Distillation import data_utils_GC as kd
    graphs, _ = _molecules(20)
    packed = kd.pack_dataset([(n, e) for n, e, _ in graphs])
    for method in ("OTD", "Sinkhorn"):
        got = kd.packed_curvature(*packed, method=method)
        at = 0
        for n, e, _ in graphs:
            rowptr, col, _ = synth.edges_to_csr(n, e)
            alone = engine.ollivier_ricci_otd(rowptr, col, e) if method == "OTD" else engine.ollivier_ricci_sinkhorn(rowptr, col, e)
            assert np.array_equal(got[at:at + len(e)], alone), method
            at += len(e)
        assert at == len(got)

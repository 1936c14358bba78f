"""CPU: the host rules of the node-classification drop-ins (pipelines_GIN.py, Knowledge_Distillation/ConvCurv_GIN.py) against the
reference's: masks per loader (:101-116), the name rules for hidden size, dropout, hop and epochs, and create_wmlp's structure; and
the two work-size functions of nc_curv.hip, which are host code."""
import itertools
import random

import numpy as np
import torch


def _data(n, k, **kw):
    from tlc_gnn_amd.data import Data
    y = torch.arange(n) % k
    return Data(y=y, **kw)


def test_split_masks_amazon_coauthor():
    from tlc_gnn_amd import pipelines_GIN as p
    for loader in ("Amazon", "Coauthor"):
        d = _data(7650, 8)
        tr, va, te = p.split_masks(d, loader)
        idx = np.arange(7650)
        assert tr.dtype == torch.bool
        assert np.array_equal(tr.numpy(), idx < 160)                                   # 20 * classes
        assert np.array_equal(va.numpy(), (idx >= 160) & (idx < 660))
        assert np.array_equal(te.numpy(), idx >= 7650 - 1000)


def test_split_masks_planetoid_and_synthesis():
    from tlc_gnn_amd import pipelines_GIN as p
    n = 1500
    m = torch.zeros(n, dtype=torch.uint8)
    m[:30] = 1
    d = _data(n, 3, train_mask=m, val_mask=1 - m, test_mask=m)
    tr, va, te = p.split_masks(d, "Planetoid")
    assert tr.dtype == torch.bool and int(tr.sum()) == 30 and int(va.sum()) == n - 30 and torch.equal(te, tr)
    # the reference's shuffled split: random.shuffle(index), then i < 400 / 400 <= i < 800 / i >= n - 200 on the shuffled values
    tr, va, te = p.split_masks(_data(n, 3), "Synthesis", rng=random.Random(7))
    index = list(range(n))
    random.Random(7).shuffle(index)
    assert tr.tolist() == [i < 400 for i in index]
    assert va.tolist() == [400 <= i < 800 for i in index]
    assert te.tolist() == [i >= n - 200 for i in index]


def test_name_rules():
    from tlc_gnn_amd import pipelines_GIN as p
    from tlc_gnn_amd.Knowledge_Distillation import ConvCurv_GIN as m
    assert [m.hidden_dim_of(s) for s in ("Physics", "computers", "Computers", "photo", "Cora", "PubMed", "CS")] == [64, 64, 256, 256, 256, 256, 256]
    assert [m.dropout_of(s) for s in ("Cora", "Physics", "CS", "PubMed", "photo")] == [0.6, 0.8, 0.2, 0.4, 0.4]
    assert [m.hop_of(s) for s in ("Cora", "Citeseer", "PubMed", "photo", "CS")] == [2, 2, 2, 1, 1]
    assert [p.settings(s) for s in ("Photo", "Computers", "PubMed", "Cora", "CS")] == [(500, 200), (500, 200), (200, 100), (200, 100), (200, 100)]
    assert [p.loader_of(s) for s in ("Cora", "Photo", "Physics", "X")] == ["Planetoid", "Amazon", "Coauthor", "Synthesis"]
    assert m.num("3") == 3 and m.num("0.5") == 0.5


def test_create_wmlp_structure():
    from tlc_gnn_amd.Knowledge_Distillation import ConvCurv_GIN as m
    mlp = m.create_wmlp([50, 256], 256, 1)
    assert len(mlp) == 3
    assert isinstance(mlp[0], torch.nn.Linear) and mlp[0].bias is None and tuple(mlp[0].weight.shape) == (256, 50)
    assert isinstance(mlp[1], torch.nn.PReLU) and tuple(mlp[1].weight.shape) == (256,) and bool((mlp[1].weight == 0.2).all())
    assert isinstance(mlp[2], torch.nn.Linear) and mlp[2].bias is not None and tuple(mlp[2].weight.shape) == (256, 256)
    conv = m.curvGN(500, 3, skip_sum=True)
    assert sorted(k for k, _ in conv.named_parameters()) == ["lin.bias", "lin.weight", "lin1.bias", "lin1.weight", "w_mlp_out.0.weight",
                                                             "w_mlp_out.1.weight", "w_mlp_out.2.bias", "w_mlp_out.2.weight"]


def test_nc_work_size_functions():
    """include/tlcgnn.h: tlc_nc_group_work_ints = 2 n + 4 E; tlc_nc_curv_work_bytes = 4 (3 E C + ceil(E / 64) C + 32 C max(C, D)) for C in
    1..256 and D in 1..64; -1 outside the range."""
    from tlc_gnn_amd import _lib
    L = _lib.lib()
    for n, E in ((1, 0), (1, 1), (10, 63), (19717, 108365), (5, 2 ** 31 - 1), (2 ** 31 - 1, 0), (2 ** 31 - 1, 2 ** 31 - 1)):
        assert L.tlc_nc_group_work_ints(n, E) == 2 * n + 4 * E, (n, E)
    for n, E in ((0, 0), (0, 5), (-1, 5), (3, -1), (-2 ** 31, 0)):
        assert L.tlc_nc_group_work_ints(n, E) == -1, (n, E)
    for n, E, Cc, D in itertools.product((1, 19717), (0, 1, 63, 64, 65, 108365, 2 ** 31 - 1), (1, 3, 64, 255, 256), (1, 17, 50, 64)):
        want = 4 * (3 * E * Cc + -(-E // 64) * Cc + 32 * Cc * max(Cc, D))
        assert L.tlc_nc_curv_work_bytes(n, E, Cc, D) == want, (n, E, Cc, D)
    assert L.tlc_nc_curv_work_bytes(1, 0, 1, 1) == 128                           # the split-K scratch alone
    assert L.tlc_nc_curv_work_bytes(7, 100, 3, 50) == 4 * (900 + 2 * 3 + 32 * 150)
    for n, E, Cc, D in ((0, 5, 8, 5), (-1, 5, 8, 5), (4, -1, 8, 5), (4, 5, 0, 5), (4, 5, -1, 5), (4, 5, 257, 5), (4, 5, 8, 0), (4, 5, 8, -3),
                        (4, 5, 8, 65), (4, 5, 257, 65)):
        assert L.tlc_nc_curv_work_bytes(n, E, Cc, D) == -1, (n, E, Cc, D)

"""No GPU: the host side of the teacher's GIN / GCN / SAGE baselines.  The new symbols are exported and bound, the backward's scratch size
is pinned, the torch restatement (tests/gnn_baseline_cases.py) agrees with dense-matrix forms on small graphs, and Teacher_Model
constructs with the reference's defaults with exactly the parameter names the module documents."""
import ctypes as C

import numpy as np
import pytest
import torch

import gnn_baseline_cases as gb

NEW = ("tlc_gnn_layer_fwd", "tlc_gnn_layer_bwd_work_bytes", "tlc_gnn_layer_bwd", "tlc_gnn_stack_fwd")


def test_symbols_are_exported_and_bound_with_argtypes():
    from tlc_gnn_amd import _lib
    L = _lib.lib()
    for name in NEW:
        assert name in _lib.SYMBOLS and hasattr(L, name), name
        assert getattr(L, name).argtypes, name
    assert len(L.tlc_gnn_layer_fwd.argtypes) == 16 and len(L.tlc_gnn_layer_bwd.argtypes) == 22 and len(L.tlc_gnn_stack_fwd.argtypes) == 14
    assert L.tlc_gnn_layer_bwd_work_bytes.restype is C.c_int64


@pytest.mark.parametrize("n,c_in,c_out", [(0, 1, 32), (1, 1, 32), (135, 5, 16), (200000, 32, 32), (123457, 64, 8)])
def test_backward_scratch_size_is_the_layout(n, c_in, c_out):
    """dZ [n][c_out] | G [n][c_in] | H [n][c_in], each on a multiple of four floats, | 32 split-K partials of the larger weight gradient."""
    from tlc_gnn_amd import _lib
    up4 = lambda v: (v + 3) // 4 * 4
    want = 4 * (up4(n * c_out) + 2 * up4(n * c_in) + 32 * max(c_out * c_in, c_out))
    assert _lib.lib().tlc_gnn_layer_bwd_work_bytes(n, c_in, c_out) == want
    for bad in ((-1, 1, 32), (1, -1, 32), (1, 1, -32)):
        assert _lib.lib().tlc_gnn_layer_bwd_work_bytes(*bad) == -1


def _dense(ei, n):
    A = torch.zeros(n, n, dtype=torch.float64)           # A[i, j] = number of edges j -> i (repeats and loops counted)
    A.index_put_((ei[1], ei[0]), torch.ones(ei.shape[1], dtype=torch.float64), accumulate=True)
    return A


def test_gin_restatement_is_the_dense_form():
    rs = np.random.RandomState(0)
    gen = torch.Generator().manual_seed(0)
    n = 9
    ei = gb.random_edges(rs, n, 30, loops="double")
    ei = torch.cat([ei, ei[:, :3]], dim=1)                # repeated edges
    x = torch.randn(n, 5, generator=gen, dtype=torch.float64)
    p = gb.random_layer_params("GIN", 5, 8, gen)
    want = (_dense(ei, n) + torch.eye(n, dtype=torch.float64)) @ x @ p["w"].t() + p["b"]
    assert _dense(ei, n)[0, 0] == 2 and _dense(ei, n).max() >= 2
    assert torch.allclose(gb.gin_layer(x, ei, p["w"], p["b"]), want, rtol=0, atol=1e-12)
    assert torch.allclose(gb.gin_layer(x, ei, p["w"], p["b"], "relu"), want.clamp(min=0), rtol=0, atol=1e-12)


def test_gcn_restatement_is_the_oracle_gcn_layer_on_a_symmetric_graph():
    from oracle import lp_forward_ref as ref
    rs = np.random.RandomState(1)
    gen = torch.Generator().manual_seed(1)
    n = 12
    e = gb.random_edges(rs, n, 25, loops="none", repeats=False)
    ei = torch.cat([e, e.flip(0)], dim=1)
    x = torch.randn(n, 4, generator=gen, dtype=torch.float64)
    p = gb.random_layer_params("GCN", 4, 8, gen)
    got = gb.gcn_layer(x, ei, p["weight"], p["bias"])
    want = ref.gcn_conv(x.float(), ei, p["weight"].float(), p["bias"].float())
    assert gb.rel(got, want) <= 1e-6                      # (the oracle's layer is float32)
    # and the dense form D^-1/2 (A + I) D^-1/2 with the loops of the list replaced by one per node
    ei_l = torch.cat([ei, torch.tensor([[3, 3, 5], [3, 3, 5]])], dim=1)        # repeated and single loops: dropped, one per node added
    A = _dense(ei, n) + torch.eye(n, dtype=torch.float64)
    dis = A.sum(1).pow(-0.5)
    dense = (dis[:, None] * A * dis[None, :]) @ (x @ p["weight"]) + p["bias"]
    assert torch.allclose(gb.gcn_layer(x, ei_l, p["weight"], p["bias"]), dense, rtol=0, atol=1e-12)


def test_sage_restatement_is_the_dense_form_with_an_empty_row():
    rs = np.random.RandomState(2)
    gen = torch.Generator().manual_seed(2)
    n = 10
    ei = gb.random_edges(rs, n, 28, loops="some")
    ei = ei[:, ei[1] != 4]                                # node 4 has no in-edge
    x = torch.randn(n, 3, generator=gen, dtype=torch.float64)
    p = gb.random_layer_params("SAGE", 3, 8, gen)
    A = _dense(ei, n)
    assert A[4].sum() == 0
    mean = (A / A.sum(1).clamp(min=1)[:, None]) @ x
    want = mean @ p["wl"].t() + p["bl"] + x @ p["wr"].t()
    got = gb.sage_layer(x, ei, p["wl"], p["bl"], p["wr"])
    assert torch.allclose(got, want, rtol=0, atol=1e-12)
    assert torch.allclose(got[4], p["bl"] + p["wr"] @ x[4], rtol=0, atol=1e-12)


def _expected_state(kind, hidden=32, out_dim=25):
    want = {}
    for conv, (i, o) in (("conv1", (1, hidden)), ("conv2", (hidden, hidden)), ("conv3", (hidden, hidden)), ("conv4", (hidden, hidden)),
                         ("conv5", (hidden, hidden))):
        for k, shape in gb.STATE_KEYS[kind](i, o).items():
            want["DIM0_Model.%s.%s" % (conv, k)] = shape
    if kind == "SAGE":
        want.update({"DIM0_Model.BN.weight": (hidden,), "DIM0_Model.BN.bias": (hidden,), "DIM0_Model.BN.running_mean": (hidden,),
                     "DIM0_Model.BN.running_var": (hidden,), "DIM0_Model.BN.num_batches_tracked": ()})
    for name, shape in (("lin5", (hidden, 2 * hidden)), ("lin6", (2, hidden)), ("lin1", (hidden, 2)), ("lin2", (out_dim, hidden)),
                        ("lin3", (hidden, hidden)), ("lin4", (hidden, hidden))):
        want[name + ".weight"], want[name + ".bias"] = shape, shape[:1]
    return want


@pytest.mark.parametrize("kwargs,kind", [({}, "GIN"), ({"type": "GCN"}, "GCN"), ({"type": "SAGE"}, "SAGE")])
def test_teacher_constructs_with_the_reference_defaults_and_names(kwargs, kind):
    """Teacher_Model() is the reference's default, type='GIN' (Teacher_model.py:21)."""
    from tlc_gnn_amd.Knowledge_Distillation.Teacher_model import Teacher_Model
    torch.manual_seed(0)
    model = Teacher_Model(**kwargs)
    assert model.DIM0_Model.type == kind
    got = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    assert got == _expected_state(kind)
    if kind == "GIN":
        assert float(model.DIM0_Model.conv1.eps) == 0.0 and "DIM0_Model.conv1.eps" not in dict(model.named_parameters())
    if kind == "GCN":
        w = model.DIM0_Model.conv2.weight
        assert float(model.DIM0_Model.conv2.bias.detach().abs().max()) == 0.0 and float(w.detach().abs().max()) <= np.sqrt(6.0 / 64) + 1e-7     # glorot / zeros


def test_base_model_default_is_gcn_and_unimplemented_types_raise():
    from tlc_gnn_amd.Knowledge_Distillation.Teacher_model import Base_Model, Teacher_Model
    assert Base_Model().type == "GCN"                     # :146
    for t in ("PDGNN", "GAT_original"):
        with pytest.raises(NotImplementedError, match="GIN"):
            Teacher_Model(type=t)
    out = Base_Model(type="SAGE")(torch.zeros(0, 1), torch.zeros(2, 0, dtype=torch.int64))
    assert out.shape == (0, 2)

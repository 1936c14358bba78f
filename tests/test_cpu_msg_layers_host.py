"""CPU: the PDGNN layer family's host side -- the restatement of tests/msg_layer_cases.py against dense-matrix forms, the modules'
parameters against the reference's names and shapes (Knowledge_Distillation/gat_conv.py:78-100, PD_conv.py:129-142), PDConv's refusals and
ops.csr_transpose_pos's contract.  No GPU: nothing here runs a layer."""
import numpy as np
import pytest
import torch

import msg_layer_cases as mc


def _small(seed, n=5, m=9, c_in=3, C=4):
    rs = np.random.RandomState(seed)
    gen = torch.Generator().manual_seed(seed)
    ei = mc.random_edges(rs, n, m, loops="some", repeats=True)
    x = torch.randn(n, c_in, generator=gen, dtype=torch.float64)
    return ei, x, mc.random_layer_params(c_in, C, gen)


@pytest.mark.parametrize("agg", mc.AGGS)
@pytest.mark.parametrize("node_feat,edge_attn", mc.MODES)
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_restatement_equals_the_dense_form_on_5_node_graphs(seed, node_feat, edge_attn, agg):
    ei, x, p = _small(seed)
    got = mc.layer(x, ei, p, node_feat, edge_attn, agg)
    ref = mc.dense_layer(x, ei, p, node_feat, edge_attn, agg)
    assert got.shape == (5, 8) and mc.rel(got, ref) <= 1e-13


def test_restatement_of_an_empty_row_is_the_bias_and_prelu_takes_the_slope_below_zero():
    ei, x, p = _small(3)
    e = mc.looped(ei, 5)
    e = e[:, e[1] != 2]                                                    # node 2 without any entry (through the C ABI only)
    out = mc.layer(x, e, p, True, True, "sum_minmax", edges_as_given=True)
    assert torch.equal(out[2], p["bias"])
    act = mc.layer(x, e, p, True, True, "sum_minmax", prelu_slope=0.1, edges_as_given=True)
    assert torch.allclose(act, torch.where(out > 0, out, 0.1 * out), rtol=0, atol=1e-15)


@pytest.mark.parametrize("node_feat,edge_attn", mc.MODES)
@pytest.mark.parametrize("double_input", [False, True])
def test_gatconv_builds_the_references_parameters_for_every_flag_combination(node_feat, edge_attn, double_input):
    from tlc_gnn_amd.Knowledge_Distillation.gat_conv import GATConv
    conv = GATConv(6, 16, double_input=double_input, concat=False, new_node_feat=node_feat, use_edge_attn=edge_attn)
    want = mc.gat_state_keys(12 if double_input else 6, 16, node_feat)
    assert {k: tuple(v.shape) for k, v in conv.state_dict().items()} == want
    assert conv.lin_r is conv.lin_l and hasattr(conv, "lin_ij") == node_feat
    assert bool((conv.bias == 0).all()) and conv.new_node_feat == node_feat and conv.use_edge_attn == edge_attn


def test_gatconv_with_both_flags_still_builds_todays_parameters_and_keeps_its_refusals():
    from tlc_gnn_amd.Knowledge_Distillation.gat_conv import GATConv
    torch.manual_seed(0)
    a = GATConv(1, 32, concat=False)
    torch.manual_seed(0)
    b = GATConv(1, 32, concat=False, new_node_feat=True, use_edge_attn=True)
    assert {k: tuple(v.shape) for k, v in a.state_dict().items()} == mc.gat_state_keys(1, 32, True)
    for (ka, va), (kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert ka == kb and torch.equal(va, vb)
    for kwargs in ({"heads": 2}, {"concat": True}, {"add_self_loops": False}, {"bias": False}, {"negative_slope": 0.1}):
        with pytest.raises(NotImplementedError):
            GATConv(1, 32, **{"concat": False, "new_node_feat": False, **kwargs})
    conv = GATConv(1, 32, concat=False, new_node_feat=False, dropout=0.5).train()
    ei = torch.tensor([[0, 1], [1, 0]])
    with pytest.raises(NotImplementedError):
        conv(torch.zeros(2, 1), ei)                                        # attention dropout in train mode
    with pytest.raises(NotImplementedError):
        conv.eval()((torch.zeros(2, 1), torch.zeros(2, 1)), ei)            # tuple input


@pytest.mark.parametrize("node_feat", [True, False])
@pytest.mark.parametrize("double_input", [False, True])
def test_pdconv_builds_the_references_parameters(node_feat, double_input):
    from tlc_gnn_amd.Knowledge_Distillation.PD_conv import PDConv
    torch.manual_seed(1)
    conv = PDConv(32, 16, double_input=double_input, new_node_feat=node_feat)
    c_in = 64 if double_input else 32
    assert {k: tuple(v.shape) for k, v in conv.state_dict().items()} == mc.pd_state_keys(c_in, 16, node_feat)
    bound = float(np.sqrt(6.0 / (c_in + 16)))                             # glorot
    wmax = float(conv.weight.detach().abs().max())
    assert 0.5 * bound < wmax <= bound
    assert bool((conv.bias == 0).all())


@pytest.mark.parametrize("kwargs", [{"improved": True}, {"cached": True}, {"normalize": False}, {"add_self_loops": False}, {"bias": False}])
def test_pdconv_refuses_what_it_does_not_implement(kwargs):
    from tlc_gnn_amd.Knowledge_Distillation.PD_conv import PDConv
    with pytest.raises(NotImplementedError):
        PDConv(1, 32, **kwargs)


def test_pdconv_refuses_a_sparse_adjacency():
    from tlc_gnn_amd.Knowledge_Distillation.PD_conv import PDConv
    conv = PDConv(1, 8)
    with pytest.raises(NotImplementedError):
        conv(torch.zeros(3, 1), object())


def test_gcn_norm_is_the_references_for_a_dense_edge_index():
    from gnn_baseline_cases import gcn_norm as ref_norm
    from tlc_gnn_amd.Knowledge_Distillation.PD_conv import gcn_norm
    rs = np.random.RandomState(4)
    ei = mc.random_edges(rs, 7, 20, loops="some", repeats=True)
    e1, w1 = gcn_norm(ei, None, 7, dtype=torch.float64)
    e2, w2 = ref_norm(ei, 7, torch.float64)
    assert torch.equal(e1, e2) and torch.allclose(w1, w2, rtol=0, atol=1e-15)
    w = torch.rand(ei.shape[1], dtype=torch.float64) + 0.5
    e3, w3 = gcn_norm(ei, w, 7)                                            # weighted: the degree is the weighted in-degree
    deg = torch.zeros(7, dtype=torch.float64).index_add_(0, e3[1], _raw_weights(ei, w, 7))
    assert torch.allclose(w3, _raw_weights(ei, w, 7) / (deg[e3[0]] * deg[e3[1]]).sqrt(), rtol=1e-13, atol=0)


def _raw_weights(ei, w, n):
    """add_remaining_self_loops' weights: the kept edges', then per node an existing loop's weight or 1."""
    keep = ei[0] != ei[1]
    loop_w = torch.ones(n, dtype=w.dtype)
    loop_w[ei[0][~keep]] = w[~keep]
    return torch.cat([w[keep], loop_w])


@pytest.mark.parametrize("node_feat,edge_attn", [(False, False), (True, False), (False, True)])
def test_teacher_model_constructs_with_the_ablation_flags(node_feat, edge_attn):
    """Teacher_Model(type='GAT', new_node_feat=False, use_edge_attn=False) -- what train_Teacher_Model.py:169-170 can ask for."""
    from tlc_gnn_amd.Knowledge_Distillation.Teacher_model import Teacher_Model
    model = Teacher_Model(type='GAT', dropout=0.0, new_node_feat=node_feat, use_edge_attn=edge_attn)
    names = {k: tuple(v.shape) for k, v in model.DIM0_Model.state_dict().items()}
    want = {}
    for conv, (ci, co) in (("conv1", (1, 32)), ("conv2", (64, 32)), ("conv3", (64, 16)), ("conv4", (64, 32)), ("conv5", (64, 32))):
        want.update({"%s.%s" % (conv, k): v for k, v in mc.gat_state_keys(ci, co, node_feat).items()})
    assert names == want
    assert model._one_call_ok(torch.zeros(3, 1), None) is False
    _, leaves = mc.teacher_params(model, node_feat, edge_attn)
    assert len(leaves) == 4 + 4 * (2 + int(node_feat) + int(edge_attn))


def test_the_type_strings_pdgnn_and_gat_original_keep_raising():
    from tlc_gnn_amd.Knowledge_Distillation.Teacher_model import Base_Model
    for t in ("PDGNN", "GAT_original"):
        with pytest.raises(NotImplementedError):
            Base_Model(type=t)


@pytest.mark.parametrize("seed", [0, 1])
def test_csr_transpose_pos_contract_on_cpu_tensors(seed):
    """Row j of the transpose lists exactly the entries whose source is j, positions ascending; col_t is the entry's target row."""
    from tlc_gnn_amd import ops
    rs = np.random.RandomState(seed)
    n = 9
    e = mc.looped(mc.random_edges(rs, n, 25, loops="some", repeats=True), n)
    order = torch.sort(e[1], stable=True).indices
    col = torch.cat([e[0][order].to(torch.int32), torch.full((4,), -7, dtype=torch.int32)])     # (room behind rowptr[n], as csr_by_target leaves)
    rowptr = torch.zeros(n + 1, dtype=torch.int32)
    rowptr[1:] = torch.cumsum(torch.bincount(e[1], minlength=n), 0)
    rowptr_t, col_t, pos_t = ops.csr_transpose_pos(rowptr, col, n)
    nnz = int(rowptr[n])
    assert rowptr_t.dtype == col_t.dtype == pos_t.dtype == torch.int32 and col_t.numel() == pos_t.numel() == nnz
    assert int(rowptr_t[0]) == 0 and int(rowptr_t[n]) == nnz
    assert sorted(pos_t.tolist()) == list(range(nnz))
    tgt_of = torch.repeat_interleave(torch.arange(n), (rowptr[1:] - rowptr[:-1]).long())
    for j in range(n):
        seg = pos_t[int(rowptr_t[j]):int(rowptr_t[j + 1])].long()
        assert bool((col[seg] == j).all()) and seg.tolist() == sorted(seg.tolist())
        assert torch.equal(col_t[int(rowptr_t[j]):int(rowptr_t[j + 1])].long(), tgt_of[seg])
    empty = ops.csr_transpose_pos(torch.zeros(1, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), 0)
    assert empty[0].tolist() == [0] and empty[1].numel() == 0 and empty[2].numel() == 0

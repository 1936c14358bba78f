"""Drop-in for the reference's Knowledge_Distillation/PD_conv.py: `gcn_norm` (:35-70) and `PDConv` (:73-225), the layer behind the
reference's model_type 'PDGNN' (Teacher_model.py:177-181).

PDConv is the PDGNN layer without attention, aggregated as sum || min (:219):

    x' = x @ weight      m_e = leaky_relu(lin_ij([x'_i || x'_j]), 0.2) with new_node_feat, else x'_j      out_i = [sum_e m_e || min_e m_e] + bias

over the edges after add_remaining_self_loops.  It runs on the layer family of csrc/msg_layers.hip (`tlc_msg_layer_fwd` with
TLC_MSG_AGG_SUM_MIN and no TLC_MSG_EDGE_ATTN; with gradients `autograd.MsgLayer`, whose backward `tlc_msg_layer_bwd` has no floating-point
atomics).  The normalised edge weights are NOT computed in forward: `message` ignores them (:190-196, the weighted return is commented
out), so only gcn_norm's structure -- self loops removed, one loop per node added -- reaches the output, and that is `ops.csr_by_target`.
A self loop's own weight in edge_weight therefore has no effect either.  improved, cached, normalize=False, add_self_loops=False,
bias=False and SparseTensor input raise NotImplementedError.
"""
import torch
from torch.nn import Linear, Parameter

from .. import ops, autograd
from .gat_conv import glorot, GraphBatch


def gcn_norm(edge_index, edge_weight=None, num_nodes=None, improved=False, add_self_loops=True, dtype=None):
    """:35-70 for a dense edge_index [2, E]: add_remaining_self_loops, then deg^-1/2[row] * w * deg^-1/2[col] with the in-degree by
    weight -> (edge_index [2, E'], weight [E']) with the kept edges first, then one loop per node (an existing loop's weight is kept, as
    add_remaining_self_loops does; else fill_value 1, or 2 with improved).  On a CUDA edge_index without weights, improved=False and
    add_self_loops=True the values are those of `ops.gcn_norm_csr` (the CSR the GCN baseline reads); this function returns the edge-list
    form the reference's callers expect, by torch ops."""
    if not isinstance(edge_index, torch.Tensor):
        raise NotImplementedError("gcn_norm (HIP): dense edge_index only (no SparseTensor)")
    if num_nodes is None:
        num_nodes = int(edge_index.max()) + 1 if edge_index.numel() else 0
    fill_value = 2. if improved else 1.
    if edge_weight is None:
        edge_weight = torch.ones((edge_index.size(1),), dtype=dtype, device=edge_index.device)
    if add_self_loops:
        row, col = edge_index[0], edge_index[1]
        keep = row != col
        loop_w = torch.full((num_nodes,), fill_value, dtype=edge_weight.dtype, device=edge_index.device)
        loop_w[row[~keep]] = edge_weight[~keep]
        loops = torch.arange(num_nodes, dtype=edge_index.dtype, device=edge_index.device)
        edge_index = torch.cat([edge_index[:, keep], loops.unsqueeze(0).repeat(2, 1)], dim=1)
        edge_weight = torch.cat([edge_weight[keep], loop_w])
    row, col = edge_index[0], edge_index[1]
    deg = torch.zeros(num_nodes, dtype=edge_weight.dtype, device=edge_index.device).scatter_add_(0, col, edge_weight)
    deg_inv_sqrt = deg.pow(-0.5)
    deg_inv_sqrt.masked_fill_(deg_inv_sqrt == float('inf'), 0)
    return edge_index, deg_inv_sqrt[row] * edge_weight * deg_inv_sqrt[col]


class PDConv(torch.nn.Module):
    def __init__(self, in_channels, out_channels, double_input=False, new_node_feat=True, improved=False, cached=False,
                 add_self_loops=True, normalize=True, bias=True, **kwargs):
        super(PDConv, self).__init__()
        if improved or cached or not normalize or not add_self_loops or not bias:
            raise NotImplementedError("PDConv (HIP): improved=False, cached=False, normalize=True, add_self_loops=True, bias=True only "
                                      "(what Teacher_model.py:177-181 builds)")
        self.in_channels, self.out_channels = in_channels, out_channels
        self.improved, self.cached, self.normalize, self.add_self_loops = improved, cached, normalize, add_self_loops
        self.new_node_feat = bool(new_node_feat)
        if new_node_feat:
            self.lin_ij = Linear(2 * out_channels, out_channels, bias=False)                    # :129-130
        self.weight = Parameter(torch.Tensor((2 if double_input else 1) * in_channels, out_channels))   # :131-134
        self.bias = Parameter(torch.Tensor(2 * out_channels))                                   # :140
        self.reset_parameters()

    def reset_parameters(self):
        glorot(self.weight)
        self.bias.data.zero_()

    def forward(self, x, edge_index, edge_weight=None, prelu_slope=-1.0, csr=None):
        """prelu_slope >= 0: the F.prelu that follows the layer in Base_Model.forward (Teacher_model.py:218-227), fused.
        csr: a `GraphBatch` of this edge_index held by the caller, or a (rowptr, col) pair as GATConv takes (anything else raises);
        default: built here.  edge_weight is accepted and ignored, as the reference's message does."""
        if not isinstance(x, torch.Tensor) or not isinstance(edge_index, torch.Tensor):
            raise NotImplementedError("PDConv (HIP): tensor x and dense edge_index only (no SparseTensor)")
        assert x.dim() == 2
        if isinstance(csr, GraphBatch):
            csr.check(edge_index, x.shape[0])
        elif csr is not None and not (isinstance(csr, (tuple, list)) and len(csr) == 2):
            raise TypeError("PDConv (HIP): csr is a GraphBatch(edge_index, n) or a (rowptr, col) pair of GATConv.csr_by_target")
        mode = ops.msg_mode(self.new_node_feat, False)
        wl = self.weight.t()                                                                     # x @ weight = x Wl^T
        wij = self.lin_ij.weight if self.new_node_feat else None
        params = [p for p in (self.weight, wij, self.bias) if p is not None]
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params)):
            # (the backward gathers over the transpose, which a GraphBatch holds: a bare pair is not enough, so the structure is built here)
            batch = csr if isinstance(csr, GraphBatch) else GraphBatch(edge_index, x.shape[0], tiled=False)
            return autograd.msg_layer(x, wl, None, wij, self.bias, batch, mode, "sum_min", prelu_slope)
        rowptr, col = (csr.rowptr, csr.col) if isinstance(csr, GraphBatch) else (csr if csr is not None else ops.csr_by_target(edge_index, x.shape[0]))
        return ops.msg_layer(rowptr, col, x, wl.detach(), None, None if wij is None else wij.detach(), self.bias.detach(), mode, "sum_min", prelu_slope)

    def __repr__(self):
        return '{}({}, {})'.format(self.__class__.__name__, self.in_channels, self.out_channels)

"""The sum-aggregating baselines of the PDGNN teacher: GINConv, GCNConv and SAGEConv as Teacher_model.py:148-175,202-208 builds them
(torch_geometric 1.6.1's), on one fused HIP layer (`tlc_gnn_layer_fwd` / `tlc_gnn_layer_bwd`, csrc/gnn_layers.hip):

    agg_i = self_scale * x_i + sum over the in-edges e of i of coef[e] * x_src[e]        y_i = act(Wa agg_i + Ws x_i + b)

  type  structure                                   coef                           self_scale  Wa, Ws, b
  GIN   edge_index as given (loops, repeats kept)   --                             1 + eps = 1 nn.0.weight, --, nn.0.bias
  GCN   gcn_norm's operator (PD_conv.py:35-70)      its values                     0           weight^T, --, bias
  SAGE  edge_index as given                         1 / max(in-degree of i, 1)     0           lin_l.weight, lin_r.weight, lin_l.bias

GCN: the reference computes x @ weight first, then propagates, then adds the bias; the operator is linear, so aggregate-then-project is the
same function up to fp32 rounding.  SAGE is the PyG 1.6.1 form lin_l(mean_j x_j) + lin_r(x_i); self loops are not touched, an empty row
gives 0.

PARITY UNPINNED at this boundary: torch_geometric is not installed where this was written and the reference ships no checkpoint, so the
parameter names (`convK.nn.0.weight`, `convK.eps`, `convK.weight`, `convK.lin_l.weight`, ...) and initialisations are PyG 1.6.1's as far
as SURVEY.md 8(c) records them, not compared against a loaded state dict.
"""
import torch
from torch.nn import Linear, Parameter

from .. import ops, autograd
from .gat_conv import glorot

KINDS = ("GIN", "GCN", "SAGE")


class GnnBatch:
    """The structure of one (block-diagonal) batch for one baseline type, built ONCE per batch and reused by the four layers and by the
    backward: the CSR by target with its coefficients, its transpose as a CSR by source (built on first use by a backward) and the tile cut
    for the one-launch stack (cut on first use by a forward without gradients).  GIN and SAGE: the raw edge list grouped by a stable sort
    (torch ops on the device; entries of a row in edge_index order); GCN: ops.gcn_norm_csr / gcn_norm_csr_t.
    Reuse rule as GraphBatch's: it holds the edge_index it was built from and `check()` raises on another or edited tensor."""

    def __init__(self, edge_index, n, kind, tiled=True):
        if kind not in KINDS:
            raise ValueError("GnnBatch: kind %r; one of %s" % (kind, KINDS))
        assert edge_index.is_cuda and edge_index.dtype == torch.int64 and edge_index.dim() == 2 and edge_index.shape[0] == 2
        self.edge_index, self.n, self.kind, self.version = edge_index, int(n), kind, edge_index._version
        self.self_scale = 1.0 if kind == "GIN" else 0.0                 # GINConv(eps=0): (1 + eps) x_i
        self._t, self._tiled, self._tiles, self._cut, self._ends = None, bool(tiled), None, False, None
        if kind == "GCN":
            self.rowptr, self.src, self.coef = ops.gcn_norm_csr(edge_index, self.n)
            self._inv = None
        else:
            self.rowptr, self.src, deg = self._group(edge_index[1], edge_index[0])
            self._inv = (1.0 / deg.clamp(min=1).to(torch.float32)) if kind == "SAGE" else None
            self.coef = None if self._inv is None else torch.repeat_interleave(self._inv, deg)

    def _group(self, key, other):
        """CSR of the edges grouped by `key` (stable: a row's entries in edge_index order): (rowptr int32 [n + 1], other int32, counts)."""
        order = torch.sort(key, stable=True).indices
        cnt = torch.bincount(key, minlength=self.n)
        rowptr = torch.zeros(self.n + 1, dtype=torch.int32, device=key.device)
        rowptr[1:] = torch.cumsum(cnt, 0)
        return rowptr, other[order].to(torch.int32).contiguous(), cnt

    def transpose(self):
        """(rowptr_t, col_t, coef_t): the same operator as a CSR by source, each entry with the forward's coefficient of its edge."""
        if self._t is None:
            ei = self.edge_index
            if self.kind == "GCN":
                self._t = ops.gcn_norm_csr_t(ei, self.n, self.rowptr)
            else:
                order = torch.sort(ei[0], stable=True).indices
                tgt = ei[1][order]
                rowptr_t = torch.zeros(self.n + 1, dtype=torch.int32, device=ei.device)
                rowptr_t[1:] = torch.cumsum(torch.bincount(ei[0], minlength=self.n), 0)
                self._t = (rowptr_t, tgt.to(torch.int32).contiguous(), None if self._inv is None else self._inv[tgt].contiguous())
        return self._t

    @property
    def tiles(self):
        """ops.gat_tiles of this CSR (any CSR has such a cut or none; an edge crosses a position in both directions or in neither, so the
        cut of the CSR by target is the transpose's too); None for a batch without close enough cuts."""
        if self._tiled and not self._cut:
            self._tiles, self._cut = ops.gat_tiles(self.rowptr, self.src, self.n), True
        return self._tiles

    def edge_ends(self, m):
        """int32 (src, dst) of the first m edges (the batch without the self loops appended last): the edge head's operands."""
        if self._ends is None or self._ends[0] != m:
            ei = self.edge_index
            self._ends = (m, ei[0, :m].to(torch.int32).contiguous(), ei[1, :m].to(torch.int32).contiguous())
        return self._ends[1], self._ends[2]

    def check(self, edge_index, n, kind=None):
        if edge_index is not self.edge_index or edge_index._version != self.version or int(n) != self.n or (kind is not None and kind != self.kind):
            raise ValueError("GnnBatch: built for another (or since edited) edge_index / node count / layer type; build a new one")
        return self


class _GnnConv(torch.nn.Module):
    kind = None

    def _operands(self):
        raise NotImplementedError

    def _act(self, prelu_slope):
        return ("prelu", float(prelu_slope)) if prelu_slope is not None and prelu_slope >= 0 else (None, 0.0)

    def layer(self, prelu_slope=-1.0):
        """(wa, ws, bias, act, slope) of this layer, detached: one entry of ops.gnn_stack's `layers`."""
        wa, ws, b = self._operands()
        act, slope = self._act(prelu_slope)
        return (wa.detach(), None if ws is None else ws.detach(), None if b is None else b.detach(), act, slope)

    def forward(self, x, edge_index, prelu_slope=-1.0, csr=None):
        """prelu_slope >= 0: the F.prelu that follows the layer in Base_Model.forward (Teacher_model.py:221-227), fused.
        csr: a GnnBatch of this edge_index held by the caller; default: built here."""
        assert isinstance(x, torch.Tensor) and x.dim() == 2
        batch = csr.check(edge_index, x.shape[0], self.kind) if isinstance(csr, GnnBatch) else GnnBatch(edge_index, x.shape[0], self.kind)
        wa, ws, b = self._operands()
        act, slope = self._act(prelu_slope)
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            return autograd.gnn_layer(x, wa, ws, b, batch, act, slope)
        return ops.gnn_layer(batch.rowptr, batch.src, batch.coef, batch.self_scale, x, wa.detach(), None if ws is None else ws.detach(),
                             None if b is None else b.detach(), act, slope)


class GINConv(_GnnConv):
    """torch_geometric.nn.GINConv(nn, eps=0, train_eps=False) with nn = Sequential(Linear[, ReLU]) (Teacher_model.py:166-175):
    nn((1 + eps) x_i + sum_j x_j).  Parameters `nn.0.weight [out, in]`, `nn.0.bias`, buffer `eps = [0.]`."""
    kind = "GIN"

    def __init__(self, nn, eps=0., train_eps=False):
        super(GINConv, self).__init__()
        mods = list(nn)
        if train_eps or float(eps) != 0.0 or not mods or not isinstance(mods[0], Linear) or mods[0].bias is None or len(mods) > 2 \
                or (len(mods) == 2 and not isinstance(mods[1], torch.nn.ReLU)):
            raise NotImplementedError("GINConv (HIP): nn = Sequential(Linear) or Sequential(Linear, ReLU), eps = 0, train_eps=False")
        self.nn = nn
        self.register_buffer('eps', torch.Tensor([0.]))
        self.relu = len(mods) == 2

    def _operands(self):
        return self.nn[0].weight, None, self.nn[0].bias

    def _act(self, prelu_slope):
        if prelu_slope is not None and prelu_slope >= 0:
            raise NotImplementedError("GINConv (HIP): the GIN branch of Base_Model.forward has no PReLU between its layers")
        return ("relu", 0.0) if self.relu else (None, 0.0)


class GCNConv(_GnnConv):
    """The reference's GCNConv (PD_conv.py, a copy of PyG 1.6.1's): `weight [in, out]` (glorot), `bias [out]` (zeros)."""
    kind = "GCN"

    def __init__(self, in_channels, out_channels):
        super(GCNConv, self).__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.weight = Parameter(torch.Tensor(in_channels, out_channels))
        self.bias = Parameter(torch.Tensor(out_channels))
        glorot(self.weight)
        self.bias.data.zero_()

    def _operands(self):
        return self.weight.t(), None, self.bias


class SAGEConv(_GnnConv):
    """torch_geometric 1.6.1's SAGEConv: lin_l(mean_j x_j) + lin_r(x_i); `lin_l.weight`, `lin_l.bias`, `lin_r.weight`."""
    kind = "SAGE"

    def __init__(self, in_channels, out_channels):
        super(SAGEConv, self).__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.lin_l = Linear(in_channels, out_channels, bias=True)
        self.lin_r = Linear(in_channels, out_channels, bias=False)

    def _operands(self):
        return self.lin_l.weight, self.lin_r.weight, self.lin_l.bias

"""Drop-in for the reference's Knowledge_Distillation/ConvCurv_GIN.py: the curvature-graph node classifier whose per-edge inputs
w_mul are the images of a frozen PDGNN (Teacher_Model) of each endpoint's Ricci ball.

  Net :18-146 (compute_NodeFeat :78-97, compute_PI :100-129, forward :131-146), curvGN :149-176, create_wmlp :178-185, num :187-191,
  call :193-208.

curvGN runs on the HIP kernels of csrc/nc_curv.hip through autograd.CurvConv (forward and backward are library calls); dropout, ELU
and log_softmax stay torch ops.  Module and parameter names are the reference's, so a reference state_dict loads.  Differences:
the teacher (a module or a state dict) and the curvature are arguments instead of hard-coded paths, there is no file cache of w_mul
(it stays the attribute `w_mul`), and compute_PI is batched: NodeVicinities.batch over a chunk of nodes and ONE block-diagonal teacher
forward per chunk.  Teacher edge convention: the vicinity's edges followed by one self loop per node, as in gcn_LP_GIN.Net; the
reference's call omits the self loops and thereby drops the last n real edges inside Teacher_Model -- that latent
bug is not reproduced.
"""
import numpy as np
import torch
import torch.nn.functional as F
from torch.nn import Linear, PReLU, Sequential as seq

from .. import autograd, ops


def hidden_dim_of(name):
    """:22-25 (PyG's Amazon lower-cases its names: Computers -> 64, Photo -> 256)."""
    return 64 if name in ['Physics', 'computers'] else 256


def dropout_of(name):
    """:132-139"""
    if name in ['Cora']:
        return 0.6
    if name in ['Physics']:
        return 0.8
    if name in ['CS']:
        return 0.2
    return 0.4


def hop_of(name):
    """:80, :194"""
    return 2 if name in ["Cora", "Citeseer", "PubMed"] else 1


def _remove_self_loops(edge_index):
    return edge_index[:, edge_index[0] != edge_index[1]]


def _add_self_loops(edge_index, num_nodes):
    loops = torch.arange(num_nodes, dtype=edge_index.dtype, device=edge_index.device)
    return torch.cat([edge_index, torch.stack([loops, loops])], dim=1)


def _undirected_edges(edge_index):
    """nx.Graph(remove_self_loops(edge_index)) as an edge array [m,2] (lower label first, each edge once), what Vicinities takes."""
    e = _remove_self_loops(edge_index.detach().cpu()).numpy().T
    if len(e) == 0:
        return np.zeros((0, 2), dtype=np.int64)
    e = np.sort(e, axis=1)
    return np.unique(e, axis=0).astype(np.int64)


class Net(torch.nn.Module):
    def __init__(self, data, name, num_features, num_classes, hop=None, g=None, dimension=5, skip_cat=False, skip_sum=False,
                 teacher=None, ricci_curv=None, w_mul=None, chunk=4096, ricci_method="Sinkhorn"):
        """teacher: the trained Teacher_Model (frozen here) or its state dict -- required to compute w_mul (the reference loads it from
        a hard-coded path, :43-44; a random teacher would give meaningless images, so there is no default); ricci_curv: the
        reference's [[u, v, kappa], ...] list of g's edges (None: loaddatas.compute_ricci_curvature on the GPU); g: the graph as an
        edge array or networkx graph (None: the edges of data.edge_index).  w_mul: precomputed edge inputs [E, 2 dimension^2]
        (skips compute_NodeFeat / compute_PI; the teacher may then be left out: an untrained one only fills the state dict's
        modelGIN entries).  ricci_method: how that curvature is computed when ricci_curv is None -- "Sinkhorn" (the default) or
        "OTD", the exact transport distance the reference's node-classification pipeline builds its curvature files with
        (pipelines_GIN.py:79: `OllivierRicci(Gd, alpha=0.5, method="OTD")`); not reproduced: the library's nbr_topk cut of
        neighbourhoods above 3 000, weighted graphs, directed graphs."""
        super(Net, self).__init__()
        from ..loaddatas import RICCI_METHODS
        if ricci_method not in RICCI_METHODS:
            raise ValueError("ConvCurv_GIN.Net: ricci_method must be 'Sinkhorn' or 'OTD', got %r" % (ricci_method,))
        self.ricci_method = ricci_method
        from .Teacher_model import Teacher_Model
        self.dimension = dimension
        hidden_dim = hidden_dim_of(name)
        self.conv1 = curvGN(num_features, hidden_dim, dimension=dimension, skip_cat=skip_cat, skip_sum=skip_sum)
        if skip_cat:
            self.conv2 = curvGN(hidden_dim * 2, num_classes, dimension=dimension, skip_cat=False, skip_sum=skip_sum)
        else:
            self.conv2 = curvGN(hidden_dim, num_classes, dimension=dimension, skip_cat=False, skip_sum=skip_sum)
        self.skip_cat = skip_cat
        self.skip_sum = skip_sum
        self.leakyrelu = torch.nn.LeakyReLU(0.2, True)
        self.linear = torch.nn.Linear(dimension * dimension, 1, bias=True)
        self.linear_1 = torch.nn.Linear(dimension * dimension + 16, dimension * dimension, bias=True)
        self.hop = hop_of(name) if hop is None else hop
        self.g = g
        self.name = name
        if teacher is None and w_mul is None:
            raise ValueError("ConvCurv_GIN.Net: pass the trained teacher (a Teacher_Model or its state dict) to compute w_mul, "
                             "or pass w_mul itself")
        if teacher is None or isinstance(teacher, dict):
            model = Teacher_Model(hidden_dim=32, type='GAT', num_models=1, dropout=0, new_node_feat=True, use_edge_attn=True)
            if teacher is not None:
                model.load_state_dict(teacher)
            teacher = model
        self.modelGIN = teacher.to(data.edge_index.device) if torch.cuda.is_available() else teacher
        for param in self.modelGIN.parameters():
            param.requires_grad = False
        if w_mul is not None:
            self.w_mul = w_mul
        else:
            self.compute_NodeFeat(data, name, ricci_curv)
            self.compute_PI(data, name, chunk=chunk)

    def compute_NodeFeat(self, data, name, ricci_curv=None):
        """:78-97: the device graph the balls are cut from (NodeVicinities), built once; the per-node filtrations themselves are
        extracted in compute_PI's batches."""
        from .data_utils_NC import NodeVicinities
        g = self.g if self.g is not None else _undirected_edges(data.edge_index)
        if ricci_curv is None:
            from ..data import Data
            from ..loaddatas import compute_ricci_curvature
            if self.g is None:                                   # the data's own edges, in their order (it orients each edge)
                e = _remove_self_loops(data.edge_index.detach().cpu())
            else:
                e = torch.from_numpy(np.asarray(g if not hasattr(g, "edges") else list(g.edges()), dtype=np.int64).reshape(-1, 2).T.copy())
            # (compute_ricci_curvature takes the node count from len(data.y))
            ricci_curv = compute_ricci_curvature(Data(edge_index=e, y=torch.zeros(data.num_nodes, dtype=torch.long)), method=self.ricci_method)
        self._vic = NodeVicinities(g, ricci_curv)

    @torch.no_grad()
    def compute_PI(self, data, name, chunk=4096):
        """:100-129, batched.  PI[u] = the teacher's image of u's Ricci ball (hop 2 for Cora / Citeseer / PubMed, else 1), zero for a
        ball without an edge; F.normalize per row for 'photo'.  w_mul[e] = [PI[u] || PI[v]] for e = (u, v), zero on self loops.
        Sets self.PI (float32 [n, 25]) and self.w_mul (float32 [E, 50]) on the device."""
        self.modelGIN.eval()
        hop = hop_of(name)
        n = data.num_nodes
        dev = data.edge_index.device if data.edge_index.is_cuda else torch.device("cuda")
        PI = torch.zeros(n, 25, device=dev)
        nodes = np.arange(n, dtype=np.int64)
        for lo in range(0, n, chunk):
            b = self._vic.batch(nodes[lo:lo + chunk], hop)
            node_ptr, edge_ptr = b["node_ptr"], b["edge_ptr"]
            n_tot = int(node_ptr[-1])
            if n_tot == 0 or int(edge_ptr[-1]) == 0:
                continue
            e = b["edges"].long() + node_ptr[b["pair_of_edge"]].view(-1, 1)           # block-diagonal node ids
            loops = torch.arange(n_tot, device=e.device)
            edge_index = torch.cat([e.t(), torch.stack([loops, loops])], dim=1)
            x = b["f"].to(torch.float32).view(-1, 1)
            _, img, *_ = self.modelGIN(x, edge_index, None, compute_loss=False, grad_PI=False, graph_ptr=node_ptr, edge_ptr=edge_ptr)
            img = img.to(torch.float32)
            if name in ['photo']:
                img = F.normalize(img, dim=1)
            ok = (edge_ptr[1:] - edge_ptr[:-1]) > 0                                    # (None, None) balls stay zero (:107-108)
            PI[lo:lo + len(ok)][ok] = img[ok]
        self.PI = PI
        ei = data.edge_index.to(dev)
        w_mul = torch.cat([PI[ei[0]], PI[ei[1]]], dim=1)
        w_mul[ei[0] == ei[1]] = 0.0
        self.w_mul = w_mul.contiguous()
        return self.w_mul

    def forward(self, data):
        """:131-146"""
        dropout = dropout_of(self.name)
        x, edge_index = data.x, data.edge_index
        x = F.dropout(x, p=dropout, training=self.training)
        x = self.conv1(x, edge_index, self.w_mul)
        x = F.elu(x)
        x = F.dropout(x, p=dropout, training=self.training)
        x = self.conv2(x, edge_index, self.w_mul)
        return F.log_softmax(x, dim=1)


class curvGN(torch.nn.Module):
    """:149-176 -- propagate with aggr='add' (flow source_to_target): out[t] = sum over edges (s, t) of softmax_s(w_mlp_out(w_mul))
    * lin(x)[s]; the softmax normalises over a node's OUT-edges, the sum runs over its IN-edges.  One HIP call forward
    (autograd.CurvConv); the edge grouping is built once per edge_index and kept."""

    def __init__(self, in_channels, out_channels, dimension=5, skip_cat=False, skip_sum=False):
        super(curvGN, self).__init__()
        self.lin = Linear(in_channels, out_channels)
        self.skip_cat = skip_cat
        self.skip_sum = skip_sum
        if skip_cat or skip_sum:
            self.lin1 = Linear(in_channels, out_channels)
        widths = [dimension * dimension * 2, out_channels]
        self.w_mlp_out = create_wmlp(widths, out_channels, 1)
        self._groups = None

    def groups(self, edge_index, num_nodes):
        """ops.nc_group of edge_index, cached for the same tensor (same storage, shape and version)."""
        key = (edge_index.data_ptr(), tuple(edge_index.shape), edge_index._version, int(num_nodes), edge_index.device)
        if self._groups is None or self._groups[0] != key or self._groups[1] is not edge_index:
            self._groups = (key, edge_index, ops.nc_group(edge_index, num_nodes))
        return self._groups[2]

    def forward(self, x, edge_index, w_mul):
        if len(self.w_mlp_out) != 3:
            raise NotImplementedError("curvGN (HIP): the edge MLP of create_wmlp([2 d^2, C], C, 1) only")
        x = x.contiguous()
        grp = self.groups(edge_index, x.shape[0])
        m = self.w_mlp_out
        out = autograd.curv_conv(x, self.lin.weight, self.lin.bias, m[0].weight, m[1].weight, m[2].weight, m[2].bias,
                                 w_mul.detach().to(torch.float32).contiguous(), grp)
        if self.skip_cat:
            return torch.cat((out, autograd.nc_linear(x, self.lin1.weight, self.lin1.bias)), dim=-1)
        if self.skip_sum:
            return out + autograd.nc_linear(x, self.lin1.weight, self.lin1.bias)
        return out


def create_wmlp(widths, nfeato, lbias):
    """:178-185"""
    mlp_modules = []
    for k in range(len(widths) - 1):
        mlp_modules.append(Linear(widths[k], widths[k + 1], bias=False))
        mlp_modules.append(PReLU(widths[k + 1], 0.2))
    mlp_modules.append(Linear(widths[len(widths) - 1], nfeato, bias=lbias))
    return seq(*mlp_modules)


def num(strings):
    """:187-191"""
    try:
        return int(strings)
    except ValueError:
        return float(strings)


def call(data, name, num_features, num_classes, teacher=None, ricci_curv=None, g=None, w_mul=None, ricci_method="Sinkhorn"):
    """:193-208: remove_self_loops, then one self loop per node appended (add_self_loops); the model and the data on the device.
    teacher (or w_mul) is required, and ricci_method ("Sinkhorn" or "OTD") is handed on: see Net."""
    hop = hop_of(name)
    data.edge_index = _add_self_loops(_remove_self_loops(data.edge_index), data.x.size(0))
    device = torch.device('cuda' if torch.cuda.is_available() else 'cpu')
    data = data.to(device)
    model = Net(data, name, num_features, num_classes, hop, g, teacher=teacher, ricci_curv=ricci_curv, w_mul=w_mul, ricci_method=ricci_method).to(device)
    return model, data

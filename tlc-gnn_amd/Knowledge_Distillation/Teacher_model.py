"""Drop-in for the reference's Knowledge_Distillation/Teacher_model.py (PDGNN): type='GAT' (the PDGNN layer) and the message-passing
baselines it is compared against, type='GIN' (the reference's default for Teacher_Model), 'GCN' (its default for Base_Model) and 'SAGE'.

  Teacher_Model.__init__ :21-44, forward :46-104 (grad_PI=False: :53-59, :83-84), compute_PD_loss :106-137 (kernel='wasserstein'),
  Base_Model.__init__ :146-211 (GAT branch :182-189), Base_Model.forward :213-229.

The whole forward stays on the GPU: four fused GAT layers, the edge head and the persistence image raster
(`tlc_gat_layer_fwd`, `tlc_edge_head_fwd`, `tlc_pi_raster`); the reference copies the predicted diagram to the host and
rasterises it with the Cython CPU code (:84).

Training: with `compute_loss=True, kernel='wasserstein'` the diagram loss is the device matching
(`tlc_w2_partial_matching`; the reference calls POT's ot.emd on the host, wasserstein.py:303) and `loss.backward()` runs
`tlc_edge_head_bwd` and `tlc_gat_layer_bwd` (autograd.py).  Train mode with dropout > 0 (the shipped script trains with dropout = 0,
train_Teacher_Model.py:163): torch's F.dropout at the reference's five points (:58, :218-227), on tensors of the same shapes, so a seed
draws the reference's masks; the edge head then runs unfused (the mask sits between its two GEMMs).  kernel='sliced_wasserstein' is the
reference's 'sliced' branch as a device loss (`tlc_sliced_wasserstein`, any diagram size).  What is NOT here: kernel='sliced' under
that name (the reference's own branch cannot run: it ends in `return loss, ind_tmp_test, loss_xy, ...` with those names never bound,
:110-123,139, and hands lists of CUDA tensors to scipy's cityblock) and draw_fig.  grad_PI=True (the signature's default; the
training script passes False, train_Teacher_Model.py:51): the image of the differentiable imager (pimg.py:354-400) with its gradient
-- through the points' weights only, because the reference detaches the coordinates inside the normal-CDF factors (:392,395);
`tlc_pi_raster_wgrad` (autograd.DiagramImage).

Evaluation (train_Teacher_Model.py:85-113: `model(filt, edge_index, PD, p=p, kernel=kernel, pair_diagonal=True, grad_PI=False)`):
pair_diagonal=True -> compute_PD_loss(type='inference') :66,134-136 -> `wasserstein_distance_inference` (wasserstein.py:93-195)
-> `tlc_w2_inference_matching`; loss_yd0 is then the targets left to the diagonal.

The baselines (Base_Model.__init__ :148-175,202-208, forward :213-241; gnn_layers.py): one fused HIP layer for the three types
(`tlc_gnn_layer_fwd`, backward `tlc_gnn_layer_bwd` without atomics); without gradients and dropout the four layers of a batch of small
graphs run as ONE launch (`tlc_gnn_stack_fwd`), then the edge head and the imager as for 'GAT'.  The GIN branch has no PReLU between its
layers (:233-241); the other types have F.prelu(0.1) behind conv1, conv2 and conv4.  conv5 (and SAGE's BN) are constructed and unused, as
in the reference.  Parameter names and initialisations are PyG 1.6.1's as far as SURVEY.md 8(c) records them: torch_geometric is not
installed where this was written and the reference ships no checkpoint, so this boundary is UNPINNED (gnn_layers.py).

The ablations of the training scripts (train_Teacher_Model.py:169-170: new_node_feat, use_edge_attn) go through type='GAT': every layer
is built with the two flags (:185-189), and the three configurations with a flag off run on the layer family of csrc/msg_layers.hip
(`tlc_msg_layer_fwd`, and `tlc_msg_layer_bwd` without floating-point atomics; gat_conv.py).  The one-call inference forward
(`tlc_pdgnn_forward`) serves the full configuration only -- it reads every layer's lin_ij -- so an ablated model runs layer by layer.
PD_conv.py's PDConv, the layer behind the reference's type='PDGNN' (:177-181), exists as a layer module (Knowledge_Distillation/PD_conv.py,
the same family with sum || min).  The `type` strings 'PDGNN' and 'GAT_original' themselves keep raising: the baselines' tests pin that
refusal, so a PDGNN stack is built from PDConv layers by hand until a change lifts it.
"""
import time

import torch
import torch.nn.functional as F
from torch.nn import Linear

from .. import ops, engine, autograd
from torch.nn import BatchNorm1d, ReLU, Sequential

from .gat_conv import GATConv, GraphBatch
from .gnn_layers import GCNConv, GINConv, SAGEConv, GnnBatch

BASELINES = ('GIN', 'GCN', 'SAGE')


class Base_Model(torch.nn.Module):
    def __init__(self, in_dim=1, hidden_dim=32, dropout=0.2, type='GCN', out_dim=2, new_node_feat=True, use_edge_attn=True):
        super(Base_Model, self).__init__()
        if type != 'GAT' and type not in BASELINES:
            raise NotImplementedError("Base_Model (HIP): type %r is not implemented; implemented are 'GAT' (the PDGNN layer) and the "
                                      "baselines 'GIN', 'GCN', 'SAGE'" % (type,))
        if type == 'GCN':                                                                          # :148-153
            self.conv1 = GCNConv(in_dim, hidden_dim)
            self.conv2 = GCNConv(hidden_dim, hidden_dim)
            self.conv3 = GCNConv(hidden_dim, out_dim)
            self.conv4 = GCNConv(hidden_dim, hidden_dim)
            self.conv5 = GCNConv(hidden_dim, hidden_dim)
        elif type == 'GIN':                                                                        # :162-175
            self.conv1 = GINConv(Sequential(Linear(in_dim, hidden_dim), ReLU()))
            self.conv2 = GINConv(Sequential(Linear(hidden_dim, hidden_dim), ReLU()))
            self.conv3 = GINConv(Sequential(Linear(hidden_dim, out_dim)))
            self.conv4 = GINConv(Sequential(Linear(hidden_dim, hidden_dim), ReLU()))
            self.conv5 = GINConv(Sequential(Linear(hidden_dim, hidden_dim), ReLU()))
        elif type == 'SAGE':                                                                       # :202-208
            self.conv1 = SAGEConv(in_dim, hidden_dim)
            self.conv2 = SAGEConv(hidden_dim, hidden_dim)
            self.conv3 = SAGEConv(hidden_dim, out_dim)
            self.conv4 = SAGEConv(hidden_dim, hidden_dim)
            self.conv5 = SAGEConv(hidden_dim, hidden_dim)
            self.BN = BatchNorm1d(hidden_dim)
        else:
            self.conv1 = GATConv(in_dim, hidden_dim, concat=False, new_node_feat=new_node_feat, use_edge_attn=use_edge_attn)
            self.conv2 = GATConv(hidden_dim, hidden_dim, double_input=True, concat=False, new_node_feat=new_node_feat, use_edge_attn=use_edge_attn)
            self.conv3 = GATConv(hidden_dim, int(out_dim / 2), double_input=True, concat=False, new_node_feat=new_node_feat, use_edge_attn=use_edge_attn)
            self.conv4 = GATConv(hidden_dim, hidden_dim, double_input=True, concat=False, new_node_feat=new_node_feat, use_edge_attn=use_edge_attn)
            self.conv5 = GATConv(hidden_dim, hidden_dim, double_input=True, concat=False, new_node_feat=new_node_feat, use_edge_attn=use_edge_attn)
        self.hidden_dim = hidden_dim
        self.dropout = dropout
        self.type = type
        self.out_dim = out_dim

    def forward(self, x, edge_index, csr=None):
        """csr: a `GraphBatch` of this edge_index held by the caller (a loop that runs the model on the same batch again, e.g.
        evaluate_time of train_Teacher_Model.py:124-151, builds it once); default: built here, once for the four layers."""
        if x.size()[0] == 0:
            return torch.zeros([0, 2], device=x.device)
        # F.dropout of :218-227 (train mode only): on the input and behind the prelu of conv1 / conv2 / conv4.  torch's own op, at the
        # same points and on tensors of the same shapes as the reference, so the same seed draws the same masks
        drop = (lambda t: F.dropout(t, p=self.dropout, training=True)) if (self.training and self.dropout > 0) else (lambda t: t)
        if self.type in BASELINES:
            return self._forward_baseline(x, edge_index, csr, drop)
        if csr is None:
            csr = GraphBatch(edge_index, x.shape[0])                   # one CSR (and tile cut) for the four layers of THIS call
        elif isinstance(csr, GraphBatch):
            csr.check(edge_index, x.shape[0])                          # (handed down whole: the layers take its tiles)
        x = self.conv1(drop(x), edge_index, prelu_slope=0.1, csr=csr)  # conv -> F.prelu(0.1) fused (:218-219)
        x = self.conv2(drop(x), edge_index, prelu_slope=0.1, csr=csr)
        x = self.conv4(drop(x), edge_index, prelu_slope=0.1, csr=csr)
        x = self.conv3(drop(x), edge_index, csr=csr)
        return x


    def _forward_baseline(self, x, edge_index, csr, drop):
        """:213-241 for 'GIN' / 'GCN' / 'SAGE': F.dropout in front of every layer (train mode only), F.prelu(0.1) behind conv1 / conv2 /
        conv4 except in the GIN branch.  csr: a `GnnBatch` of this edge_index and type held by the caller; default: built here."""
        if csr is None:
            csr = GnnBatch(edge_index, x.shape[0], self.type)
        elif isinstance(csr, GnnBatch):
            csr.check(edge_index, x.shape[0], self.type)
        else:
            raise TypeError("Base_Model (HIP): type %r takes csr=GnnBatch(edge_index, n, %r)" % (self.type, self.type))
        slope = -1.0 if self.type == 'GIN' else 0.1
        convs = (self.conv1, self.conv2, self.conv4, self.conv3)
        wants_grad = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for c in convs for p in c.parameters()))
        if not wants_grad and not (self.training and self.dropout > 0) and x.is_cuda and x.dtype == torch.float32 \
                and self.out_dim == self.hidden_dim and ops.gnn_stack_ok(x.shape[1], self.hidden_dim, csr.tiles):
            layers = [c.layer(s) for c, s in zip(convs, (slope, slope, slope, -1.0))]
            return ops.gnn_stack(csr.rowptr, csr.src, csr.coef, csr.self_scale, csr.tiles, x, layers)   # the four layers, one launch
        x = self.conv1(drop(x), edge_index, prelu_slope=slope, csr=csr)
        x = self.conv2(drop(x), edge_index, prelu_slope=slope, csr=csr)
        x = self.conv4(drop(x), edge_index, prelu_slope=slope, csr=csr)
        x = self.conv3(drop(x), edge_index, csr=csr)
        return x


class Teacher_Model(torch.nn.Module):
    def __init__(self, hidden_dim=32, out_dim=25, num_models=3, dropout=0.2, type='GIN', max_loop_len=10, new_node_feat=True,
                 use_edge_attn=True):
        super(Teacher_Model, self).__init__()
        self.DIM0_Model = Base_Model(1, hidden_dim, dropout, type, out_dim=hidden_dim, new_node_feat=new_node_feat,
                                     use_edge_attn=use_edge_attn)
        self.lin5 = Linear(2 * hidden_dim, hidden_dim)
        self.lin6 = Linear(hidden_dim, 2)
        self.num_models = num_models
        self.lin1 = Linear(2, hidden_dim)
        self.lin2 = Linear(hidden_dim, out_dim)
        self.lin3 = Linear(hidden_dim, hidden_dim)
        self.lin4 = Linear(hidden_dim, hidden_dim)
        self.dropout = dropout

    def _one_call_params(self):
        d = self.DIM0_Model
        ps = []
        for conv in (d.conv1, d.conv2, d.conv4, d.conv3):
            ps += [conv.lin_l.weight, conv.att_l, conv.lin_ij.weight, conv.bias]
        return [p.detach() for p in ps + [self.lin5.weight, self.lin5.bias, self.lin6.weight, self.lin6.bias]]

    def _one_call_ok(self, x0, csr):
        """tlc_pdgnn_forward serves the reference's configuration (in_dim 1, hidden 32, float32) when no gradient is wanted and no
        dropout is drawn; everything else takes the layer-by-layer path below."""
        c1 = getattr(self.DIM0_Model, 'conv1', None)
        if self.DIM0_Model.type == 'GAT' and not (c1.new_node_feat and c1.use_edge_attn):
            return False                                              # (_one_call_params reads lin_ij and att_l of every layer)
        if self.DIM0_Model.type != 'GAT' or not x0.is_cuda or x0.dim() != 2 or x0.shape[1] != 1 or x0.shape[0] == 0 or self.lin5.out_features != 32 \
                or self.DIM0_Model.conv1.out_channels != 32 or self.DIM0_Model.conv3.out_channels != 16 or self.lin5.weight.dtype != torch.float32 \
                or (self.training and self.dropout > 0) or not (csr is None or isinstance(csr, GraphBatch)):
            return False
        return not (torch.is_grad_enabled() and (x0.requires_grad or any(p.requires_grad for p in self.parameters())))

    def forward(self, x0, edge_index0, PD, kernel='sliced', M=50, p=1, pair_diagonal=False, draw_fig=False, fig_name='',
                compute_loss=True, grad_PI=True, graph_ptr=None, edge_ptr=None, pd_ptr=None, csr=None, w2_large='refuse', sigma=1.0):
        """Reference signature.  compute_loss=True needs kernel='wasserstein' (p = 1 or 2) and returns
        loss0 (differentiable), loss_xy0, loss_xd0, loss_yd0 like :63-66.  pair_diagonal=False (training, :64): every target
        point is matched, loss_yd0 is 0 (wasserstein.py:330-372, num_models=1); pair_diagonal=True (evaluation, :66): the
        distance in which both diagrams may use the diagonal, loss_yd0 = the targets left to it.
        kernel='sliced_wasserstein': the reference's 'sliced' branch (:110-124, the sliced Wasserstein distance over M directions,
        `tlc_sliced_wasserstein`) with the return repaired: loss0 differentiable, loss_xy0 / loss_xd0 / loss_yd0 zeros (the branch
        computes no parts); p and pair_diagonal have no effect there.  kernel='sliced' itself (the signature's default) keeps raising.
        kernel='pss' (not in the reference): loss0 = the sum over the graphs of the squared persistence scale-space kernel distance with
        bandwidth `sigma` between the predicted and the target diagram (`autograd.diagram_kernel_distance`, tlc_dgm_gram); the three
        parts are zeros as for 'sliced_wasserstein'.  Smooth, no assignment, no cap on the points.

        x0 [n,1] filtration, edge_index0 [2, m+n] with the n self loops LAST (train_Teacher_Model.py:43-44).
        Block-diagonal batches: pass graph_ptr (int64 [B+1] node offsets) and edge_ptr (int64 [B+1] offsets into the
        non-self-loop edges) to get one image per graph [B,25]; otherwise one image [25] for the whole input.  With a loss,
        pd_ptr (int64 [B+1]) gives the rows of PD that belong to each graph; without it every graph must have exactly as
        many target points as edges (PD = Ord0 + Ext1 of the same graph: n - 1 + m - n + 1 = m points, data_utils_GC.py:166).
        csr: a `GraphBatch(edge_index0, n)` -- for the baselines a `GnnBatch(edge_index0, n, type)` -- the caller built once for this
        batch (else the CSR by target is built per call).
        w2_large (kernel='wasserstein'): 'refuse' raises for a graph whose matching has more than 4 096 rows, 'device' matches up to
        65 536 in the workspace tier (`ops.w2_large_matching`), the range in which the reference still trains with this loss.
        """
        if draw_fig:
            raise NotImplementedError("Teacher_Model (HIP): draw_fig=False only")
        if compute_loss and kernel not in ('wasserstein', 'sliced_wasserstein', 'pss'):
            raise NotImplementedError("Teacher_Model (HIP): compute_loss needs kernel='wasserstein', 'sliced_wasserstein' or 'pss' (the "
                                      "reference's 'sliced' branch cannot run: Teacher_model.py:110-123 ends in names that were never "
                                      "bound, :139; kernel='sliced_wasserstein' is that branch with the return repaired)")
        t1 = time.time()
        if not compute_loss and self._one_call_ok(x0, csr):
            # inference: the whole forward is one library call (tlc_pdgnn_forward: the same kernels, submitted natively)
            n = x0.shape[0]
            m = edge_index0.shape[1] - n
            offs = torch.tensor([0, m], dtype=torch.int64, device=x0.device) if edge_ptr is None else edge_ptr.to(torch.int64)
            held = csr if isinstance(csr, GraphBatch) else None
            if held is not None:
                held.check(edge_index0, n)
            x, img = ops.pdgnn_forward(x0, edge_index0, self._one_call_params(), offs, res=5, hidden=self.lin5.out_features,
                                       rowptr=None if held is None else held.rowptr, col=None if held is None else held.col,
                                       tiles=None if held is None else held.tiles)
            if grad_PI:
                img = img.to(x.dtype)
            if edge_ptr is None:
                img = img[0]
            t2 = time.time()
            return x, img, None, None, None, None, t2 - t1, 0.0
        x = self.DIM0_Model(x0, edge_index0, csr=csr)
        n = x0.shape[0]
        m = edge_index0.shape[1] - n
        if isinstance(csr, (GraphBatch, GnnBatch)):
            src, dst = csr.edge_ends(m)                               # (int32 copies made once per batch, like its CSR)
        else:
            src = edge_index0[0, :m].to(torch.int32).contiguous()     # strips the appended self loops (:54-55)
            dst = edge_index0[1, :m].to(torch.int32).contiguous()
        if self.training and self.dropout > 0:
            # :56-59 with the dropout mask between the head's two GEMMs: the fused kernel (tlc_edge_head) has no place for it, so this
            # one case runs lin5 -> prelu -> F.dropout -> lin6 as separate device ops (torch's linear = rocBLAS; its autograd)
            h = F.linear(torch.cat((x[src.long()], x[dst.long()]), dim=-1), self.lin5.weight, self.lin5.bias)
            h = F.dropout(F.prelu(h, torch.tensor(0.1, device=h.device, dtype=h.dtype)), p=self.dropout, training=True)
            x = F.linear(h, self.lin6.weight, self.lin6.bias)
        elif torch.is_grad_enabled() and (x.requires_grad or self.lin5.weight.requires_grad or self.lin6.weight.requires_grad):
            x = autograd.edge_head(x, self.lin5.weight, self.lin5.bias, self.lin6.weight, self.lin6.bias, src, dst, 0.1)
        else:
            x = ops.edge_head(src, dst, x, self.lin5.weight.detach(), self.lin5.bias.detach(), 0.1,
                              self.lin6.weight.detach(), self.lin6.bias.detach())                  # :56-59 (no dropout)
        t2 = time.time()
        loss0 = loss_xy0 = loss_xd0 = loss_yd0 = None
        if compute_loss:                                                                           # :61-66, compute_PD_loss :124-136
            xoff = None if edge_ptr is None else edge_ptr.to(torch.int64)
            yoff = xoff if pd_ptr is None else pd_ptr.to(torch.int64)
            if pd_ptr is None and edge_ptr is not None and int(PD.shape[0]) != m:
                # (one target point per edge is what makes edge_ptr double as the target offsets)
                raise ValueError("Teacher_Model: PD has %d points for %d edges; pass pd_ptr (target offsets per graph)" % (int(PD.shape[0]), m))
            if pd_ptr is not None and (edge_ptr is None or pd_ptr.numel() != edge_ptr.numel()):
                raise ValueError("Teacher_Model: pd_ptr needs edge_ptr with the same number of graphs")
            if kernel == 'sliced_wasserstein':                                                     # :110-124
                loss0 = autograd.sliced_diagram_loss(x, PD.to(torch.float64), M=M, xoff=xoff, yoff=yoff).sum().reshape(1)
                loss_xy0, loss_xd0, loss_yd0 = (torch.zeros(1, dtype=loss0.dtype, device=loss0.device) for _ in range(3))
            elif kernel == 'pss':
                one = torch.tensor([0, int(PD.shape[0])], dtype=torch.int64, device=x.device)
                loss0 = autograd.diagram_kernel_distance(x, torch.tensor([0, m], dtype=torch.int64, device=x.device) if xoff is None else xoff,
                                                         PD.to(torch.float64), one if yoff is None else yoff, kernel='pss', sigma=sigma).sum().reshape(1)
                loss_xy0, loss_xd0, loss_yd0 = (torch.zeros(1, dtype=loss0.dtype, device=loss0.device) for _ in range(3))
            else:
                parts = autograd.diagram_loss(x, PD.to(torch.float64), order=p, xoff=xoff, yoff=yoff, infer=bool(pair_diagonal), large=w2_large)
                loss0, loss_xy0, loss_xd0 = parts[0].sum().reshape(1), parts[1].sum().reshape(1), parts[2].sum().reshape(1)
                loss_yd0 = parts[3].sum().reshape(1) if pair_diagonal else torch.zeros(1, dtype=loss0.dtype, device=loss0.device)
        x0_out = x
        offs = torch.tensor([0, m], dtype=torch.int64, device=x.device) if edge_ptr is None else edge_ptr.to(torch.int64)
        if grad_PI:
            # :80-81, the differentiable imager (pimg.py:354-400): the same image, float32 like the reference's, with the gradient the
            # reference's graph carries -- through the points' weights only (it detaches the CDF factors)
            img = autograd.diagram_image(x, offs, 5) if (torch.is_grad_enabled() and x.requires_grad) else \
                engine.pi_raster(offs, x.detach().to(torch.float64), 5).to(x.dtype)
        else:
            img = engine.pi_raster(offs, x.detach().to(torch.float64), 5)                          # :84, on the device
        if edge_ptr is None:
            img = img[0]
        t3 = time.time()
        return x0_out, img, loss0, loss_xy0, loss_xd0, loss_yd0, t2 - t1, t3 - t2

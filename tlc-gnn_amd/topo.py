"""Topological layers on a LEARNED filtration: the exact extended persistence of a packed batch of graphs as a differentiable
function of the node values f, composed with the imager and the Wasserstein loss of `autograd`.

    f (an MLP on node features, an HKS time, ...)  ->  diagrams(f, ...)  ->  images(...) / landscapes(...) / wasserstein_to(...) /
                                                       sliced_wasserstein_to(...) / bottleneck_to(...) / kernel_distance_to(...) /
                                                       gram(...)  ->  loss.backward()

`hks_filtration(time, ...)` is the second of these filtrations: the normalised heat-kernel signature as a differentiable function of its
diffusion time (`autograd.hks_signature`: values and d / d t from tlc_hks_batch_dt and tlc_hks_large_batch_dt), so a time can be learned
through everything below.

`VicinityImages` / `vicinity_images(kappa, structure)` put the chain behind the product's own inputs: the image table of a fixed pair
list in a fixed graph as a differentiable function of the graph's curvature (gather of kappa + 1 onto the packed vicinity edges,
`distance_filtration`, `images`).

The diagrams are `engine.pd_from_filtration`'s with TLC_KEEP_ZERO_PERS (what `data_utils_GC.compute_persistence_image` computes),
bit for bit; their gradient is the selection of `autograd.ExtendedPersistence`: each coordinate is a copy of one
f[v].  All arguments are CUDA tensors in the packed layout of `engine.pd_from_filtration`: node_offs / edge_offs int64[B + 1], edges
int32[sum m, 2] local ids, f float32 or float64 [sum n]."""
import torch

from . import _lib, autograd, engine

WHICH = ("ord0+ext1", "ord0", "ext1", "ord0+ext0+ext1")


def check_which(which):
    if which not in WHICH:
        raise ValueError("which should be one of %s, not %r" % (WHICH, which))
    return which


def hks_filtration(time, node_offs, edge_offs, edges, normalise=True, hks_sparse='host'):
    """-> float64[sum n]: the heat-kernel-signature filtration of every graph at the diffusion time `time` (a scalar or one-element float
    tensor, which may require grad), the values of `data_utils_LP.hks_filtration_device(..., hks_large='device')` bit for bit.  It goes
    straight into `diagrams` / `images` / `wasserstein_to` / `sliced_wasserstein_to` as f, and their gradient reaches `time`.  The time is
    read to the host once per call; a graph the device tiers do not take raises RuntimeError (`autograd.hks_signature`).
    hks_sparse='device': what the Jacobi and large tiers leave as too large (any node count, a time inside [0, HKS_SPARSE_TIME_MAX])
    takes the sparse tier, value and derivative from tlc_hks_sparse_batch_dt, instead of raising; 'host', the default, raises."""
    if not torch.is_tensor(time) or time.numel() != 1:
        raise ValueError("hks_filtration: time should be a scalar or one-element tensor")
    return autograd.hks_signature(time.reshape(1), node_offs, edge_offs, edges, normalise=normalise, hks_sparse=hks_sparse)[0]


def distance_filtration(w, node_offs, edge_offs, edges, roots=None, descriptor="sum", norm="max", include_roots=False, unreachable_100=False):
    """-> [sum n]: the distance filtration of every graph -- per node the weighted shortest-path distance to the root(s) of its graph,
    the filtration of `filtration.build_fv` / `ricci_filtration.build_fv` bit for bit -- as a differentiable function of the edge
    weights w [sum m] (kappa + 1 of every packed edge, > 0; `autograd.distance_filtration`, tlc_dist_filtration and its VJP).  roots:
    int32[B, 2] local ids (column 1 == -1: one root), None: node 0 of every graph.  descriptor 'sum' / 'min' / 'max' over two roots; norm
    'max', 'max_eps' or 'none'.  It goes straight into `diagrams` / `images` / `wasserstein_to` / `sliced_wasserstein_to` as f, and their
    gradient reaches w along the shortest-path trees.  Under ties among path lengths the tree is a fixed convention (include/tlcgnn.h)."""
    if roots is None:
        B = node_offs.numel() - 1
        roots = torch.stack([torch.zeros(B, dtype=torch.int32, device=node_offs.device),
                             torch.full((B,), -1, dtype=torch.int32, device=node_offs.device)], 1).contiguous()
    return autograd.distance_filtration(w, node_offs, edge_offs, edges, roots, descriptor=descriptor, norm=norm,
                                        include_roots=include_roots, unreachable_100=unreachable_100)


def diagrams(f, node_offs, edge_offs, edges, pd_large="host"):
    """-> dict(ord0, ord0_offs, rel1, rel1_offs, ext1, ext1_offs, ext0, counts): the three diagrams of every graph packed
    ([K, 2] points with int64[B + 1] offsets: the input `autograd.diagram_image` and `autograd.diagram_loss` take) and ext0 [B, 2]
    = [min f, max f], all differentiable in f; counts int32[B, 4] is not."""
    up, down, one, ext0, counts = autograd.extended_persistence(f, node_offs, edge_offs, edges, _lib.KEEP_ZERO_PERS, pd_large)
    ord0, o0 = autograd.packed_points(up, node_offs, counts[:, 0])
    rel1, o1 = autograd.packed_points(down, node_offs, counts[:, 1])
    ext1, o2 = autograd.packed_points(one, edge_offs, counts[:, 2])
    return dict(ord0=ord0, ord0_offs=o0, rel1=rel1, rel1_offs=o1, ext1=ext1, ext1_offs=o2, ext0=ext0, counts=counts)


def _select(f, node_offs, edge_offs, edges, which, pd_large):
    """(points, offs) of the diagram `which` of every graph; 'ord0+ext1': a graph's Ord0 points, then its Ext1 points;
    'ord0+ext0+ext1': with the point (min f, max f) between them -- what the TLC-GNN pipeline images (tlc_pd_pi_batch without
    TLC_PI_ORD0_EXT1: the diagram's other points have negative persistence and weigh nothing)."""
    up, _, one, ext0, counts = autograd.extended_persistence(f, node_offs, edge_offs, edges, _lib.KEEP_ZERO_PERS, pd_large)
    if which == "ord0+ext0+ext1":
        # PD_zero + PD_one of sg2dgm/riccidist2dgm.py:327 without its points of negative persistence: three slots per graph in the
        # concatenation of the three arrays -- the Ord0 points, the one point (min f, max f), the Ext1 points
        B = node_offs.numel() - 1
        starts = torch.stack([node_offs[:-1], torch.arange(B, device=f.device) + up.shape[0], edge_offs[:-1] + up.shape[0] + B], 1).flatten()
        cnt = torch.stack([counts[:, 0], torch.ones_like(counts[:, 0]), counts[:, 2]], 1).flatten()
        pts, offs = autograd.pack_rows(torch.cat([up, ext0, one]), starts, cnt)
        return pts, offs[::3].contiguous()
    if which == "ord0":
        return autograd.packed_points(up, node_offs, counts[:, 0])
    if which == "ext1":
        return autograd.packed_points(one, edge_offs, counts[:, 2])
    # two slots per graph in the concatenation of the two slot arrays
    starts = torch.stack([node_offs[:-1], edge_offs[:-1] + up.shape[0]], 1).flatten()
    pts, offs = autograd.pack_rows(torch.cat([up, one]), starts, counts[:, [0, 2]].flatten())
    return pts, offs[::2].contiguous()


def images(f, node_offs, edge_offs, edges, which="ord0+ext1", res=5, pd_large="host", imager=None, grad="weight"):
    """[B, res * res] persistence images of every graph's diagram `which` -- the three images of
    `data_utils_GC.compute_persistence_image` (Ord0 ++ Ext1, Ord0, Ext1) -- as a differentiable function of f, through
    `autograd.diagram_image`.  The imager's gradient is the reference's (pimg.py:354-400): a point's two normal-CDF factors are
    computed from detached coordinates, so the gradient flows through the point's weight only.
    imager: a `Knowledge_Distillation.pimg.PersistenceImager` (any grid, sigma and ramp; [B, Rb * Rp], `res` is then unused);
    grad='full': the true derivative, which also follows a point's position -- what matters most under a small sigma."""
    check_which(which)
    pts, offs = _select(f, node_offs, edge_offs, edges, which, pd_large)
    return autograd.diagram_image(pts, offs, res, imager=imager, grad=grad)


def landscapes(f, node_offs, edge_offs, edges, ts, K=5, which="ord0+ext1", pd_large="host"):
    """[B, K, T] persistence landscapes of every graph's diagram `which` at the sample values ts [T] (a 1-D tensor without grad) -- the
    K largest tent values min(t - birth, death - t) > 0 at every sample, `autograd.diagram_landscape` -- as a differentiable function
    of f.  The sibling of `images` without a sigma or a ramp: the gradient of a cell reaches the one node value behind the birth or
    the death of the point that attains it.  Points of zero persistence are never present."""
    check_which(which)
    if not torch.is_tensor(ts) or ts.dim() != 1:
        raise ValueError("landscapes: ts should be a 1-D tensor of sample values")
    if ts.requires_grad:
        raise ValueError("landscapes: ts requires grad, but the samples get no gradient (detach them)")
    if not 1 <= int(K) <= _lib.LS_KMAX or not 1 <= ts.numel() <= _lib.LS_TMAX:
        raise ValueError("landscapes: K = %d outside 1 .. %d or %d samples outside 1 .. %d" % (int(K), _lib.LS_KMAX, ts.numel(), _lib.LS_TMAX))
    pts, offs = _select(f, node_offs, edge_offs, edges, which, pd_large)
    return autograd.diagram_landscape(pts, offs, ts, K=K)


def wasserstein_to(f, node_offs, edge_offs, edges, target_pts, target_offs, which="ord0+ext1", order=2, pd_large="host", w2_large="refuse"):
    """[B] Wasserstein distances (order `order`, both diagrams may use the diagonal: `autograd.diagram_loss(..., infer=True)`) between
    every graph's diagram `which` and the fixed target diagrams target_pts [sum k, 2] / target_offs int64[B + 1]; differentiable in f.
    w2_large: 'refuse' raises for a pair of more than 4 096 points in all, 'device' matches pairs of up to 65 536 (the workspace tier,
    `ops.w2_large_matching`: exact, but a million and more serial steps per problem)."""
    check_which(which)
    pts, offs = _select(f, node_offs, edge_offs, edges, which, pd_large)
    return autograd.diagram_loss(pts, target_pts.to(pts.dtype), order=order, xoff=offs, yoff=target_offs, infer=True, large=w2_large)[0]


def sliced_wasserstein_to(f, node_offs, edge_offs, edges, target_pts, target_offs, which="ord0+ext1", M=50, pd_large="host"):
    """[B] sliced Wasserstein distances (`autograd.sliced_diagram_loss` over the reference's M directions) between every graph's
    diagram `which` and the target diagrams target_pts [sum k, 2] / target_offs int64[B + 1]; differentiable in f (and in target_pts
    when it requires grad).  The sibling of `wasserstein_to` without a cap on the points and at a fraction of its cost: sorts instead of an assignment."""
    check_which(which)
    pts, offs = _select(f, node_offs, edge_offs, edges, which, pd_large)
    return autograd.sliced_diagram_loss(pts, target_pts.to(pts.dtype), M=M, xoff=offs, yoff=target_offs)


def kernel_distance_to(f, node_offs, edge_offs, edges, target_pts, target_offs, which="ord0+ext1", sigma=1.0, kernel="pss", pd_large="host"):
    """[B] SQUARED kernel distances k(F, F) + k(G, G) - 2 k(F, G) (`autograd.diagram_kernel_distance`; 'pss': the persistence
    scale-space kernel with bandwidth sigma, 'gauss': the plain Gaussian) between every graph's diagram `which` and the target diagrams
    target_pts [sum k, 2] / target_offs int64[B + 1]; differentiable in f (and in target_pts when it requires grad).  The smooth sibling
    of `sliced_wasserstein_to`: a double sum of Gaussians, no assignment, no sort, no cap on the points."""
    check_which(which)
    pts, offs = _select(f, node_offs, edge_offs, edges, which, pd_large)
    return autograd.diagram_kernel_distance(pts, offs, target_pts.to(pts.dtype), target_offs, kernel=kernel, sigma=sigma)


def gram(f, node_offs, edge_offs, edges, which="ord0+ext1", sigma=1.0, kernel="pss", pd_large="host"):
    """[B, B] Gram matrix of the kernel between every two graphs' diagrams `which` (`autograd.diagram_gram`, the symmetric call) as a
    differentiable function of f: what a kernel SVM on the exact diagrams takes, and the only B x B operation of this module."""
    check_which(which)
    pts, offs = _select(f, node_offs, edge_offs, edges, which, pd_large)
    return autograd.diagram_gram(pts, offs, kernel=kernel, sigma=sigma)


def bottleneck_to(f, node_offs, edge_offs, edges, target_pts, target_offs, which="ord0+ext1", pd_large="host"):
    """[B] bottleneck distances (`autograd.bottleneck_loss`: both diagrams may use the diagonal) between every graph's diagram `which` and
    the target diagrams target_pts [sum k, 2] / target_offs int64[B + 1]; differentiable in f (and in target_pts when it requires grad).
    The worst-point sibling of `wasserstein_to`: the gradient reaches the one or two node values behind the pair that attains the
    distance.  A pair of more than 4 096 points in all raises RuntimeError."""
    check_which(which)
    pts, offs = _select(f, node_offs, edge_offs, edges, which, pd_large)
    return autograd.bottleneck_loss(pts, target_pts.to(pts.dtype), xoff=offs, yoff=target_offs)


# ---- the product's own images as a function of the GRAPH's curvature ------------------------------------------------
_VI_FLAGS = (_lib.KEEP_ZERO_PERS | _lib.INCLUDE_ROOTS | _lib.NORM_EPS | _lib.PI_ORD0_EXT1 | _lib.UNREACHABLE_100 | _lib.DESC_ROOT1
             | _lib.NO_NORM)


def dist_options(flags):
    """The TLC flag word of the vicinity pipeline -> (`distance_filtration`'s keyword arguments, one_root)."""
    desc = flags & _lib.DESC_ROOT1
    one_root = desc == _lib.DESC_ROOT1
    descriptor = "sum" if one_root or desc == 0 else ("min" if desc == _lib.DESC_MIN else "max")
    norm = "none" if flags & _lib.NO_NORM else ("max_eps" if flags & _lib.NORM_EPS else "max")
    return dict(descriptor=descriptor, norm=norm, include_roots=bool(flags & _lib.INCLUDE_ROOTS),
                unreachable_100=bool(flags & _lib.UNREACHABLE_100)), one_root


class VicinityStructure:
    """What does not change while the curvature is learned: the packed vicinities of a fixed pair list in a fixed graph, the graph edge
    behind every packed edge, the pairs' local root ids, the segment index of the gather's adjoint and the per-pair status."""

    def __init__(self, n_nodes, graph_edges, pairs, hop, flags=0, res=5, imager=None, grad="full", pd_large="host", device=None):
        import numpy as np
        from . import synth
        if flags & ~_VI_FLAGS:
            raise ValueError("VicinityImages: flags %#x: TLC_NO_EXT1 and unknown bits are not taken (the images are Ord0 ++ Ext1)" % flags)
        if grad not in ("weight", "full"):
            raise ValueError("VicinityImages: grad is %r, not 'weight' or 'full'" % (grad,))
        engine.check_pd_large(pd_large)
        ge = np.ascontiguousarray(graph_edges.cpu().numpy() if torch.is_tensor(graph_edges) else graph_edges, dtype=np.int64).reshape(-1, 2)
        key = ge[:, 0] * int(n_nodes) + ge[:, 1]
        if len(ge) and not ((ge[:, 0] < ge[:, 1]).all() and (ge >= 0).all() and (ge < n_nodes).all() and (key[1:] > key[:-1]).all()):
            raise ValueError("VicinityImages: graph_edges should list every undirected edge once, lo < hi, ascending by (lo, hi) "
                             "(np.unique(np.sort(edges, 1), axis=0)): kappa[k] is the curvature of graph_edges[k]")
        dev = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
        pairs_h = np.ascontiguousarray(pairs.cpu().numpy() if torch.is_tensor(pairs) else pairs, dtype=np.int32).reshape(-1, 2)
        self.n_nodes, self.n_edges, self.n_pairs, self.hop, self.flags = int(n_nodes), len(ge), len(pairs_h), int(hop), int(flags)
        self.res, self.imager, self.grad, self.pd_large = int(res), imager, grad, pd_large
        self.opts, self.one_root = dist_options(flags)
        # the diagram behind the image, as tlc_pd_pi_batch has it: Ord0 ++ Ext1 under TLC_PI_ORD0_EXT1, else with the point (min f, max f)
        self.which = "ord0+ext1" if flags & _lib.PI_ORD0_EXT1 else "ord0+ext0+ext1"
        self.graph_edges = torch.from_numpy(ge.astype(np.int32)).to(dev)
        self.pairs = torch.from_numpy(pairs_h).to(dev)
        rowptr, col, w = synth.edges_to_csr(n_nodes, ge, None)            # unit weights: only the structure is read
        graph = engine.DeviceGraph(rowptr, col, w, device=dev.index)
        try:
            with torch.cuda.device(dev):
                # every pair once for its status; then the pairs that get a row, packed without the others
                first = self._extract(graph, self.pairs)
                # (a vicinity without an edge -- one node, or the two ends of a far pair under TLC_INCLUDE_ROOTS -- has no tree edge: the
                # persistence stage's IndexError, TLC_ST_NO_TREE_EDGE in tlc_pd_pi_batch)
                lone = (first["status"] == _lib.ST_OK) & (first["n"] > 0) & (first["m0"] == 0)
                self.status = torch.where(lone, torch.full_like(first["status"], _lib.ST_NO_TREE_EDGE), first["status"])
                keep = (first["status"] == _lib.ST_OK) & (first["m"] > 0) & (first["lookup"] == _lib.ST_OK)
                self.rows = keep.nonzero().flatten()
                b = first if bool(keep.all()) else self._extract(graph, self.pairs[self.rows].contiguous())
        finally:
            graph.close()
        if self.rows.numel() and bool(((b["status"] != _lib.ST_OK) | (b["lookup"] != _lib.ST_OK)).any()):
            raise RuntimeError("VicinityImages: a vicinity changed between two extractions of the same pair")
        self.node_ptr, self.edge_ptr, self.ids, self.edges = b["node_ptr"], b["edge_ptr"], b["ids"], b["edges"]
        self.eid, self.roots = b["eid"], b["roots"]
        self.seg_ptr, self.seg_pos = engine.segment_index(self.eid, self.n_edges)
        self.columns = self.res * self.res
        if imager is not None:
            rb, rp = (imager if isinstance(imager, engine.PiSpec) else imager.spec(skew=True)).resolution
            self.columns = rb * rp

    def _extract(self, graph, pairs):
        n0, m0 = graph.vicinity_sizes(pairs, self.hop, flags=self.flags)
        node_ptr, edge_ptr, totals = engine.pack_offsets(n0, m0)
        lo_n, _, tot_n, tot_m = totals.tolist() if len(n0) else (0, 0, 0, 0)
        if lo_n < 0:
            raise RuntimeError("VicinityImages: a vicinity has more nodes than the packed local ids hold (status TLC_ST_TOO_LARGE)")
        _, ids, _, _, st, _, edges, m = graph.vicinity_filtration(pairs, self.hop, flags=self.flags, zero=False,
                                                                  offsets=(node_ptr, edge_ptr, tot_n, tot_m))
        ids, edges = ids[:int(tot_n)], edges[:int(tot_m)]
        m = edge_ptr[1:] - edge_ptr[:-1]
        eid, roots, lst = engine.packed_edge_lookup(self.graph_edges, node_ptr, edge_ptr, ids, edges, pairs=pairs, one_root=self.one_root)
        return dict(node_ptr=node_ptr, edge_ptr=edge_ptr, ids=ids, edges=edges, status=st, n=n0, m0=m0, m=m, eid=eid, roots=roots, lookup=lst)


def vicinity_filtration_of(kappa, structure):
    """-> float64[sum n]: the distance filtration of the structure's packed vicinities under the curvature kappa float64[M] (weights
    kappa + 1 > 0), differentiable in kappa: steps 1 and 2 of `vicinity_images`."""
    S = structure
    if kappa.dim() != 1 or kappa.numel() != S.n_edges:
        raise ValueError("vicinity_images: kappa should have one entry per graph edge (%d), not shape %s" % (S.n_edges, tuple(kappa.shape)))
    w = autograd.gather_edge_values(kappa.to(torch.float64) + 1.0, S.eid, S.seg_ptr, S.seg_pos)
    return distance_filtration(w, S.node_ptr, S.edge_ptr, S.edges, roots=S.roots, **S.opts)


def vicinity_images(kappa, structure):
    """-> (images float64[n_pairs, res * res], status uint8[n_pairs]): `graph2pi.get_pimg_for_all_edges` of the structure's pairs as a
    differentiable function of the graph's curvature kappa float64[M] (one entry per row of the structure's graph_edges):
    w = kappa + 1 gathered onto the packed vicinity edges (`autograd.gather_edge_values`), `distance_filtration`, `images` (which=
    'ord0+ext1' under TLC_PI_ORD0_EXT1, else 'ord0+ext0+ext1': the diagram tlc_pd_pi_batch images), and the rows scattered to their pairs.  The row of a pair whose status is not ST_OK -- no edge, a missing node, not
    connected without TLC_UNREACHABLE_100, a single node -- or whose vicinity holds no edge or not both of its ends (d(u, v) > hop) is zeros and
    carries no gradient, as in `DeviceGraph.pd_pi_batch`.  Under ties among path lengths or filtration values -- real Ollivier-Ricci
    curvatures tie often -- the gradient is a convention, not a derivative: the trees of tlc_dist_filtration's d_parent and the
    vertex rule of `autograd.ExtendedPersistence`."""
    S = structure
    out = torch.zeros((S.n_pairs, S.columns), dtype=torch.float64, device=S.pairs.device)
    if S.rows.numel() == 0:
        return out, S.status
    f = vicinity_filtration_of(kappa, S)
    img = images(f, S.node_ptr, S.edge_ptr, S.edges, which=S.which, res=S.res, pd_large=S.pd_large, imager=S.imager, grad=S.grad)
    return out.index_copy(0, S.rows, img.to(torch.float64)), S.status       # (rows are distinct: the backward is a plain gather)


class VicinityImages(torch.nn.Module):
    """The image table of the link predictor as a layer: `forward()` -> (images [n_pairs, res * res], status) of a fixed pair list at
    the module's learned curvature `kappa` (a float64 Parameter, one entry per row of graph_edges, zeros at the start: unit
    weights), or at the kappa handed in.  graph_edges int[M, 2]: every undirected edge once, lo < hi, ascending; pairs int[n_pairs, 2];
    flags: the TLC flag word of `DeviceGraph.pd_pi_batch` (descriptor, norm, TLC_INCLUDE_ROOTS, TLC_UNREACHABLE_100); imager / grad:
    as in `images` (grad='full' by default: a learned curvature moves points, not only their weights).  The structure
    (`VicinityStructure`) is built once, here.  Weights must stay positive: kappa > -1."""

    def __init__(self, n_nodes, graph_edges, pairs, hop, flags=0, res=5, imager=None, grad="full", pd_large="host"):
        super().__init__()
        self.structure = VicinityStructure(n_nodes, graph_edges, pairs, hop, flags=flags, res=res, imager=imager, grad=grad, pd_large=pd_large)
        self.kappa = torch.nn.Parameter(torch.zeros(self.structure.n_edges, dtype=torch.float64, device=self.structure.pairs.device))

    def forward(self, kappa=None):
        return vicinity_images(self.kappa if kappa is None else kappa, self.structure)

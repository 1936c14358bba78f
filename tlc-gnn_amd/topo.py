"""Topological layers on a LEARNED filtration: the exact extended persistence of a packed batch of graphs as a differentiable
function of the node values f, composed with the imager and the Wasserstein loss of `autograd`.

    f (an MLP on node features, an HKS time, ...)  ->  diagrams(f, ...)  ->  images(...) / wasserstein_to(...) /
                                                       sliced_wasserstein_to(...)  ->  loss.backward()

`hks_filtration(time, ...)` is the second of these filtrations: the normalised heat-kernel signature as a differentiable function of its
diffusion time (`autograd.hks_signature`: values and d / d t from tlc_hks_batch_dt and tlc_hks_large_batch_dt), so a time can be learned
through everything below.

The diagrams are `engine.pd_from_filtration`'s with TLC_KEEP_ZERO_PERS (what `data_utils_GC.compute_persistence_image` computes),
bit for bit; their gradient is the selection of `autograd.ExtendedPersistence`: each coordinate is a copy of one
f[v].  All arguments are CUDA tensors in the packed layout of `engine.pd_from_filtration`: node_offs / edge_offs int64[B + 1], edges
int32[sum m, 2] local ids, f float32 or float64 [sum n]."""
import torch

from . import _lib, autograd, engine

WHICH = ("ord0+ext1", "ord0", "ext1")


def check_which(which):
    if which not in WHICH:
        raise ValueError("which should be one of %s, not %r" % (WHICH, which))
    return which


def hks_filtration(time, node_offs, edge_offs, edges, normalise=True):
    """-> float64[sum n]: the heat-kernel-signature filtration of every graph at the diffusion time `time` (a scalar or one-element float
    tensor, which may require grad), the values of `data_utils_LP.hks_filtration_device(..., hks_large='device')` bit for bit.  It goes
    straight into `diagrams` / `images` / `wasserstein_to` / `sliced_wasserstein_to` as f, and their gradient reaches `time`.  The time is
    read to the host once per call; a graph the device tiers do not take raises RuntimeError (`autograd.hks_signature`)."""
    if not torch.is_tensor(time) or time.numel() != 1:
        raise ValueError("hks_filtration: time should be a scalar or one-element tensor")
    return autograd.hks_signature(time.reshape(1), node_offs, edge_offs, edges, normalise=normalise)[0]


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
    """(points, offs) of the diagram `which` of every graph; 'ord0+ext1': a graph's Ord0 points, then its Ext1 points."""
    up, _, one, _, counts = autograd.extended_persistence(f, node_offs, edge_offs, edges, _lib.KEEP_ZERO_PERS, pd_large)
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


def wasserstein_to(f, node_offs, edge_offs, edges, target_pts, target_offs, which="ord0+ext1", order=2, pd_large="host"):
    """[B] Wasserstein distances (order `order`, both diagrams may use the diagonal: `autograd.diagram_loss(..., infer=True)`) between
    every graph's diagram `which` and the fixed target diagrams target_pts [sum k, 2] / target_offs int64[B + 1]; differentiable in f."""
    check_which(which)
    pts, offs = _select(f, node_offs, edge_offs, edges, which, pd_large)
    return autograd.diagram_loss(pts, target_pts.to(pts.dtype), order=order, xoff=offs, yoff=target_offs, infer=True)[0]


def sliced_wasserstein_to(f, node_offs, edge_offs, edges, target_pts, target_offs, which="ord0+ext1", M=50, pd_large="host"):
    """[B] sliced Wasserstein distances (`autograd.sliced_diagram_loss` over the reference's M directions) between every graph's
    diagram `which` and the target diagrams target_pts [sum k, 2] / target_offs int64[B + 1]; differentiable in f (and in target_pts
    when it requires grad).  The sibling of `wasserstein_to` without its cap of 4 096 points: sorts instead of an assignment."""
    check_which(which)
    pts, offs = _select(f, node_offs, edge_offs, edges, which, pd_large)
    return autograd.sliced_diagram_loss(pts, target_pts.to(pts.dtype), M=M, xoff=offs, yoff=target_offs)

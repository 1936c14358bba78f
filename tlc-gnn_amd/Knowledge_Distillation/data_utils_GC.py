"""Drop-in for the ground-truth generation of the reference's Knowledge_Distillation/data_utils_GC.py (PDGNN, graph
classification: whole graph = one diagram) and for the forward-only loop of train_Teacher_Model_GC.evaluate_time.

  compute_persistence_image :98-170 (filt='degree' and 'hks': node functions on the host, the reference's own numpy / scipy calls; 'hks'
  on the device with hks_backend='device'; 'degree', and in the batch call 'centrality' and 'clustering', on the device with
  struct_backend='device'),
  filt='ricci' with the curvature as an input: `ricci_filtration_device` (tlc_dist_filtration; data_utils_NC's build_fv with root 0 and
  norm=True -- the reference's own branch :121-124 cannot run, see there),
  original_extended_persistence :78-82, call :228-279 (largest connected component, relabel), evaluate_time :118-143.

The extended persistence of every graph runs in `tlc_pd_from_filtration` (Knowledge_Distillation fork: zero-persistence pairs
kept), the three images (Ord0 ++ Ext1, Ord0, Ext1; :155-163) in `tlc_pi_raster`; `*_batch` processes a whole dataset in one
launch of each instead of the reference's per-graph Python loop.

The packed route at the end of the file -- `pack_dataset`, `ground_truth_packed`, `call_packed`, `evaluate_packed` -- is the same ground
truth with nothing per graph on the host: components, relabelling and deduplication in `tlc_graph_components`, everything else tensor ops.
"""
import numpy as np

from .. import engine, _lib


def _edges_nodes(g):
    if hasattr(g, "edges") and callable(getattr(g, "edges")):
        nodes = list(g.nodes())
        e = np.array([(a, b) for a, b in g.edges()], dtype=np.int64).reshape(-1, 2)
        return len(nodes), e
    n, e = g
    return int(n), np.asarray(e, dtype=np.int64).reshape(-1, 2)


def degree_filtration(n, edges):
    """:117-119  degree / (max degree + 1e-10), in fp64 like the reference's Python floats."""
    deg = np.bincount(edges.reshape(-1), minlength=n).astype(np.float64)
    return deg / (deg.max() + 1e-10)


def _connected(n, edges):
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in edges.tolist():
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[ra] = rb
    return len({find(i) for i in range(n)}) == 1


def hks_filtration(n, edges, hks_time):
    """:114-116  hks_signature / (max + 1e-10): the reference's scipy calls on the same matrix (nodes 0..n-1), host side."""
    from .data_utils_LP import hks_signature
    v = hks_signature(n, edges, hks_time)
    return v / (max(v) + 1e-10)


def edge_weights(edges, ricci_curv):
    """kappa + 1 of every row of edges [m, 2] from one graph's curvature in any of the reference's forms: the list of [u, v, kappa] rows
    that `compute_ricci_curvature` writes (either or both directions), or the dict {(u, v): kappa} that `data_utils_NC` builds of it."""
    if isinstance(ricci_curv, dict):
        table = ricci_curv
    else:
        table = {}
        for u, v, k in (ricci_curv.tolist() if hasattr(ricci_curv, "tolist") else ricci_curv):
            table[(int(u), int(v))] = float(k)
    out = np.empty(len(edges), dtype=np.float64)
    for i, (a, b) in enumerate(np.asarray(edges).tolist()):
        k = table.get((a, b), table.get((b, a)))
        if k is None:
            raise KeyError("ricci_curv has no entry for the edge (%d, %d)" % (a, b))
        out[i] = k + 1.0
    return out


def ricci_filtration_device(node_ptr, edge_ptr, edges, w, total_nodes=None):
    """filt='ricci' on a packed batch: `data_utils_NC.ricci_filtration(g, 0, hop, curv).build_fv(weight_graph=True, norm=True)` of every
    graph -- the weighted shortest-path distance to node 0 over the weights w = kappa + 1, 100 where node 0 is not reached, divided by
    (the maximum + 1e-10) -- from `engine.dist_filtration` (tlc_dist_filtration), bit for bit.
    This is NOT the reference's own graph-classification branch (data_utils_GC.py:121-124), which cannot run: it hands `build_fv` the
    curvature as a list of [u, v, kappa] rows, `build_fv` indexes that list with a tuple (:45), and its `except BaseException` turns
    every distance into 100.  The intended behaviour is the node-classification file's, which builds the dict first."""
    import torch
    B = node_ptr.numel() - 1
    roots = torch.stack([torch.zeros(B, dtype=torch.int32, device=node_ptr.device), torch.full((B,), -1, dtype=torch.int32, device=node_ptr.device)], 1)
    return engine.dist_filtration(node_ptr, edge_ptr, edges, w, roots.contiguous(), descriptor="sum", norm="max_eps", unreachable_100=True,
                                  total_nodes=total_nodes)[0]


def packed_curvature(node_ptr, edge_ptr, edges, alpha=0.5, method="OTD"):
    """Ollivier-Ricci curvature of every edge of a packed batch of simple graphs (each undirected edge once, local ids) in ONE call of the
    curvature engine on the block-diagonal union graph: the curvature of an edge depends on its endpoints' neighbourhoods only, so the
    union gives each graph's own values.  -> float64[sum m] numpy, aligned with `edges`.  method 'OTD' (`engine.ollivier_ricci_otd`) or
    'Sinkhorn' (`engine.ollivier_ricci_sinkhorn`).  The engines take host CSR arrays, so the batch is read back once."""
    from ..synth import edges_to_csr
    no, eo, e = (np.asarray(t.cpu()) if hasattr(t, "cpu") else np.asarray(t) for t in (node_ptr, edge_ptr, edges))
    e = e.reshape(-1, 2).astype(np.int64)
    g = e + np.repeat(no[:-1], np.diff(eo))[:, None]
    rowptr, col, _ = edges_to_csr(int(no[-1]), g)
    if method == "OTD":
        return engine.ollivier_ricci_otd(rowptr, col, g, alpha=alpha)
    if method == "Sinkhorn":
        return engine.ollivier_ricci_sinkhorn(rowptr, col, g, alpha=alpha)
    raise ValueError("packed_curvature: method 'OTD' or 'Sinkhorn', not %r" % (method,))


def _need_curvature(what):
    return NotImplementedError("data_utils_GC (HIP): filt='ricci' takes the curvature as an input (%s); it is not computed here -- "
                               "`packed_curvature` computes it for a packed batch" % what)


def compute_persistence_image_batch(graphs, filt='degree', filtrations=None, hks_time=0.1, hks_backend='host', struct_backend='host',
                                    hks_large='host', hks_sparse='host', pd_large='host', ricci_curv=None):
    """graphs: list of networkx-like graphs with nodes 0..n-1, or (n, edges[m,2]) tuples.
    Returns a list with the reference's 9-tuple per graph (:166), or (None, None) for graphs without an edge / not
    connected (:101-103).  filt: 'degree' or 'hks' (host side, :114-119); `filtrations` supplies f per graph for anything else.
    filt='ricci' with ricci_curv = one curvature per graph (each in a form `edge_weights` takes): `ricci_filtration_device` on the whole
    list in one launch (each undirected edge once, like the device backends) -- see there why this is not the reference's GC branch.
    hks_backend='device': filt='hks' from `tlc_hks_batch`, one launch for the whole list (`data_utils_LP.hks_filtration_device`; graphs
    it does not take are counted in `data_utils_LP.hks_host_fallback`); it has no effect on the other filtrations.
    hks_large='device': with filt='hks' and hks_backend='device', the graphs above _lib.HKS_NMAX nodes from `tlc_hks_large_batch` instead of
    the host (`data_utils_LP.hks_filtration_device`; counted in `data_utils_LP.hks_large_device`); no effect otherwise.
    hks_backend='device' wants each undirected edge ONCE per graph and raises RuntimeError otherwise (an (n, edges) tuple with both
    directions, as PyG stores edge_index, or with a repeated pair; also self loops and ids outside 0 .. n-1); hks_backend='host' keeps
    scipy's multigraph semantics: repeated entries add up to edge weights (both directions give the simple graph's values).
    struct_backend='device': filt 'degree', 'centrality' and 'clustering' from `tlc_struct_batch`, one launch for the whole list
    (`data_utils_LP.struct_filtration_device`: the values of `data_utils_LP.structural_filtration`, bit for bit; 'degree' equals the host
    backend's); the same contract on the edges as hks_backend='device'.  With the default 'host', 'centrality' and 'clustering' are not
    computed here (pass `filtrations`).  It has no effect on 'hks' or on `filtrations`.
    pd_large='device': the diagrams of graphs above _lib.PD_L_NMAX nodes or _lib.PD_L_MMAX edges from `tlc_pd_wide` (the whole device, no
    node cap) instead of one workgroup of `tlc_pd_from_filtration`, which does not compute a graph above 65 535 nodes at all
    (`engine.pd_from_filtration`); the same diagrams as multisets, images within the summation order."""
    import torch
    from .data_utils_LP import (STRUCT_DEVICE_FILTS, check_hks_backend, check_hks_large, check_hks_sparse, check_struct_backend, hks_filtration_device,
                                struct_filtration_device)
    check_hks_backend(hks_backend)
    check_struct_backend(struct_backend)
    check_hks_large(hks_large)
    check_hks_sparse(hks_sparse)
    engine.check_pd_large(pd_large)
    on_device = filtrations is None and filt in STRUCT_DEVICE_FILTS and struct_backend == 'device'
    ricci = filtrations is None and filt == 'ricci'
    if ricci and ricci_curv is None:
        raise _need_curvature("ricci_curv: a list with one curvature per graph")
    if filt not in ('degree', 'hks') and filtrations is None and not on_device and not ricci:
        raise NotImplementedError("data_utils_GC (HIP): filt='degree', 'hks' and 'ricci' are computed here; pass `filtrations` for anything else")
    parsed, keep = [], []
    for gi, g in enumerate(graphs):
        n, e = _edges_nodes(g)
        ok = len(e) > 0 and _connected(n, e)
        parsed.append((n, e))
        if ok:
            keep.append(gi)
    out = [(None, None)] * len(graphs)
    if not keep:
        return out
    node_offs = np.concatenate([[0], np.cumsum([parsed[gi][0] for gi in keep])]).astype(np.int64)
    edge_offs = np.concatenate([[0], np.cumsum([len(parsed[gi][1]) for gi in keep])]).astype(np.int64)
    edges = np.concatenate([parsed[gi][1] for gi in keep]).astype(np.int32)
    dev = "cuda"
    d_node_offs, d_edge_offs, d_edges = torch.from_numpy(node_offs).to(dev), torch.from_numpy(edge_offs).to(dev), torch.from_numpy(edges).to(dev)
    if filtrations is None and filt == 'hks' and hks_backend == 'device':
        d_f = hks_filtration_device(d_node_offs, d_edge_offs, d_edges, hks_time, int(node_offs[-1]), hks_large=hks_large, hks_sparse=hks_sparse)
        f = d_f.cpu().numpy()
        fs = [f[node_offs[k]:node_offs[k + 1]] for k in range(len(keep))]
    elif ricci:
        d_w = torch.from_numpy(np.concatenate([edge_weights(parsed[gi][1], ricci_curv[gi]) for gi in keep])).to(dev)
        d_f = ricci_filtration_device(d_node_offs, d_edge_offs, d_edges, d_w, int(node_offs[-1]))
        f = d_f.cpu().numpy()
        fs = [f[node_offs[k]:node_offs[k + 1]] for k in range(len(keep))]
    elif on_device:
        d_f = struct_filtration_device(filt, d_node_offs, d_edge_offs, d_edges, int(node_offs[-1]))
        f = d_f.cpu().numpy()
        fs = [f[node_offs[k]:node_offs[k + 1]] for k in range(len(keep))]
    else:
        fs = [np.asarray(filtrations[gi], dtype=np.float64) if filtrations is not None else
              (hks_filtration(parsed[gi][0], parsed[gi][1], hks_time) if filt == 'hks' else degree_filtration(*parsed[gi])) for gi in keep]
        d_f = torch.from_numpy(np.concatenate(fs)).to(dev)
    r = engine.pd_from_filtration(d_node_offs, d_edge_offs, d_edges, d_f, _lib.KEEP_ZERO_PERS, want_rank=False, pd_large=pd_large)
    counts = r["counts"].cpu().numpy()
    up, one = r["up"], r["one"]
    # gather the ragged diagrams: Ord0 of graph k = up[node_offs[k] : +counts[k,0]], Ext1 = one[edge_offs[k] : +counts[k,2]]
    idx0 = torch.cat([torch.arange(int(node_offs[k]), int(node_offs[k]) + int(counts[k, 0]), device=dev) for k in range(len(keep))])
    idx1 = torch.cat([torch.arange(int(edge_offs[k]), int(edge_offs[k]) + int(counts[k, 2]), device=dev) for k in range(len(keep))])
    p0, p1 = up[idx0], one[idx1]
    o0 = np.concatenate([[0], np.cumsum(counts[:, 0])]).astype(np.int64)
    o1 = np.concatenate([[0], np.cumsum(counts[:, 2])]).astype(np.int64)
    # Ord0 ++ Ext1 per graph (:163)
    both_idx, ob = [], [0]
    for k in range(len(keep)):
        both_idx.append(torch.arange(o0[k], o0[k + 1], device=dev))
        both_idx.append(len(p0) + torch.arange(o1[k], o1[k + 1], device=dev))
        ob.append(ob[-1] + int(counts[k, 0] + counts[k, 2]))
    pall = torch.cat((p0, p1))[torch.cat(both_idx)]
    to = lambda a: torch.from_numpy(np.asarray(a, dtype=np.int64)).to(dev)
    img = engine.pi_raster(to(ob), pall, 5).cpu().numpy()
    img0 = engine.pi_raster(to(o0), p0, 5).cpu().numpy()
    img1 = engine.pi_raster(to(o1), p1, 5).cpu().numpy()
    p0n, p1n = p0.cpu().numpy(), p1.cpu().numpy()
    for k, gi in enumerate(keep):
        n, e = parsed[gi]
        d0, d1 = p0n[o0[k]:o0[k + 1]], p1n[o1[k]:o1[k + 1]]
        PI0 = img0[k] if len(d0) else np.zeros(25)
        PI1 = img1[k] if len(d1) else np.zeros(25)
        pers_img = PI1 if len(d0) == 0 else (PI0 if len(d1) == 0 else img[k])
        edge_index = torch.from_numpy(e.T.copy()).long()
        out[gi] = (d0, d1, pers_img, fs[k].tolist(), edge_index, PI0, PI1, 0.0, 0.0)
    return out


def compute_persistence_image(g, filt='hks', hks_time=0.1, hop=2, ricci_curv=None, mode='PI', num_models=5, max_loop_len=10,
                              cycle_the=2, hks_backend='host', struct_backend='host', hks_large='host', hks_sparse='host', pd_large='host'):
    """Reference signature (:98).  filt='hks' (the default), 'degree', or 'ricci' with ricci_curv (the graph's curvature in a form
    `edge_weights` takes; `ricci_filtration_device`: data_utils_NC's build_fv with root 0 and norm=True, not the reference's GC branch,
    which cannot run); mode 'PI' -> 9-tuple, 'filtration' -> (filtration_val, edge_index).
    hks_backend (not in the reference): 'host' or 'device', see compute_persistence_image_batch: 'device' wants each undirected edge
    once and raises RuntimeError for a tuple that repeats one; 'host' keeps scipy's multigraph semantics (repeats add up to weights).
    struct_backend (not in the reference): 'host' or 'device': filt='degree' from `tlc_struct_batch` (the same bits, the same contract).
    hks_large, pd_large (not in the reference): 'host' or 'device', see compute_persistence_image_batch."""
    import torch
    from .data_utils_LP import check_hks_backend, check_hks_large, check_hks_sparse, check_struct_backend, hks_filtration_device, struct_filtration_device
    check_hks_backend(hks_backend)
    check_struct_backend(struct_backend)
    check_hks_large(hks_large)
    check_hks_sparse(hks_sparse)
    engine.check_pd_large(pd_large)
    if filt == 'ricci' and ricci_curv is None:
        raise _need_curvature("ricci_curv")
    if filt not in ('degree', 'hks', 'ricci'):
        raise NotImplementedError("data_utils_GC (HIP): filt='hks', 'degree' and 'ricci' are implemented; pass other values as "
                                  "`filtrations` to compute_persistence_image_batch")
    n, e = _edges_nodes(g)
    if len(e) == 0 or not _connected(n, e):
        return None, None
    if mode == 'filtration':
        if filt == 'ricci':
            ptr = lambda k: torch.tensor([0, k], dtype=torch.int64, device="cuda")
            f = ricci_filtration_device(ptr(n), ptr(len(e)), torch.from_numpy(e.astype(np.int32)).cuda(),
                                        torch.from_numpy(edge_weights(e, ricci_curv)).cuda(), n).cpu().numpy()
        elif filt == 'hks' and hks_backend == 'device':
            ptr = lambda k: torch.tensor([0, k], dtype=torch.int64, device="cuda")
            f = hks_filtration_device(ptr(n), ptr(len(e)), torch.from_numpy(e.astype(np.int32)).cuda(), hks_time, n,
                                      hks_large=hks_large, hks_sparse=hks_sparse).cpu().numpy()
        elif filt == 'degree' and struct_backend == 'device':
            ptr = lambda k: torch.tensor([0, k], dtype=torch.int64, device="cuda")
            f = struct_filtration_device(filt, ptr(n), ptr(len(e)), torch.from_numpy(e.astype(np.int32)).cuda(), n).cpu().numpy()
        else:
            f = hks_filtration(n, e, hks_time) if filt == 'hks' else degree_filtration(n, e)
        return f.tolist(), torch.from_numpy(e.T.copy()).long()
    return compute_persistence_image_batch([(n, e)], filt=filt, hks_time=hks_time, hks_backend=hks_backend, struct_backend=struct_backend,
                                           hks_large=hks_large, hks_sparse=hks_sparse, pd_large=pd_large, ricci_curv=None if ricci_curv is None else [ricci_curv])[0]


def largest_component(n, edges):
    """:246-248  the largest connected component (the first one among equals), relabelled 0 .. k-1 in the order of the old ids
    (nx.convert_node_labels_to_integers of the subgraph); self loops dropped (:240), each undirected edge once (nx.Graph)."""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    e = np.unique(np.sort(e[e[:, 0] != e[:, 1]], 1), axis=0)
    a = sp.coo_matrix((np.ones(len(e), dtype=np.int8), (e[:, 0], e[:, 1])), shape=(n, n))
    _, lab = connected_components(a, directed=False)
    keep = lab == np.bincount(lab, minlength=1).argmax()
    new = np.cumsum(keep) - 1
    e = e[keep[e[:, 0]]]
    return int(keep.sum()), new[e]


def call(dataset, name, filt='degree', hks_time=10, mode='PI', num_models=5, gn=0, save_dir=None, store=None, hks_backend='host',
         struct_backend='host', hks_large='host', hks_sparse='host', pd_large='host'):
    """Reference signature (:228) plus keywords.  For the first `gn` graphs of `dataset` (PyG-like items with num_nodes and edge_index
    [2, m], or (n, edges[m, 2]) tuples): the largest connected component, relabelled (:246-248), through `compute_persistence_image`.
    Returns (total_time_PD, total_time_PI) like the reference (the times are 0 here).  The per-graph results go into the dict `store`
    if one is given, and are pickled to <save_dir>/<name>_<filt>_total_test.pkl if save_dir is given (the reference writes to a fixed
    path of its authors' machine, :264-266; here nothing is written by default).  The reference runs this on Cora, Citeseer, PubMed and
    SBM graphs (:324-325): with pd_large='device' such a component's diagrams come from `tlc_pd_wide`, not from one workgroup."""
    import os
    import pickle
    from .data_utils_LP import check_hks_sparse
    check_hks_sparse(hks_sparse)
    engine.check_pd_large(pd_large)
    dict_store = {} if store is None else store
    total_time_PD = total_time_PI = 0
    for tt in range(gn):
        data = dataset[tt]
        if hasattr(data, "edge_index"):
            n, e = int(data.num_nodes), np.asarray(data.edge_index.cpu()).T
        else:
            n, e = _edges_nodes(data)
        k, ce = largest_component(n, e)
        print("nodes: {}, edges: {}".format(k, len(ce)))
        dict_store[tt] = compute_persistence_image((k, ce), filt=filt, hks_time=hks_time, hop=2, ricci_curv=None, mode=mode,
                                                   num_models=num_models, hks_backend=hks_backend, struct_backend=struct_backend,
                                                   hks_large=hks_large, hks_sparse=hks_sparse, pd_large=pd_large)
        if len(dict_store[tt]) > 2:
            total_time_PD += dict_store[tt][-2]
            total_time_PI += dict_store[tt][-1]
    if save_dir is not None:
        with open(os.path.join(save_dir, name + '_' + filt + '_total_test.pkl'), 'wb') as f:
            pickle.dump(dict_store, f, pickle.HIGHEST_PROTOCOL)
    return total_time_PD, total_time_PI


def _bottleneck_to_exact(pd_hat, edge_ptr, exact, exact_ptr):
    """float64[n_kept]: d_B of every kept graph's predicted diagram (one point per edge) against its exact Ord0 ++ Ext1."""
    from .. import ops
    return ops.bottleneck_matching(edge_ptr, pd_hat.detach(), exact_ptr, exact)["dist"]


def evaluate_batch(model, samples, bottleneck=False):
    """The forward-only loop of train_Teacher_Model_GC.evaluate_time (:118-143) as ONE block-diagonal PDGNN forward.
    samples: list of 9-tuples / (None, None) as produced above; returns float32 CUDA [n_kept, 25] images + kept indices.
    bottleneck=True: a third value, float64 CUDA [n_kept]: the bottleneck distance of every kept graph's predicted diagram (the model's
    point per edge) against its exact one (the sample's Ord0 ++ Ext1), `ops.bottleneck_matching`."""
    import torch
    xs, eis, gptr, eptr, kept = [], [], [0], [0], []
    for si, data in enumerate(samples):
        if len(data) <= 2:                       # :127-128
            continue
        f, ei = np.asarray(data[3], dtype=np.float32), data[4]
        ei = ei[:, ei[0] != ei[1]]               # remove_self_loops (:132)
        eis.append(ei + gptr[-1])
        xs.append(f)
        gptr.append(gptr[-1] + len(f))
        eptr.append(eptr[-1] + ei.shape[1])
        kept.append(si)
    if not kept:
        empty = torch.zeros(0, 25, device="cuda")
        return (empty, kept, torch.zeros(0, dtype=torch.float64, device="cuda")) if bottleneck else (empty, kept)
    n = gptr[-1]
    loops = torch.arange(n)
    edge_index = torch.cat([torch.cat(eis, dim=1), torch.stack([loops, loops])], dim=1).cuda()       # add_self_loops (:133)
    x = torch.from_numpy(np.concatenate(xs)).view(-1, 1).cuda()
    edge_ptr = torch.tensor(eptr).cuda()
    with torch.no_grad():
        pd_hat, img, *_ = model(x, edge_index, None, compute_loss=False, grad_PI=False, graph_ptr=torch.tensor(gptr).cuda(),
                                edge_ptr=edge_ptr)
    if not bottleneck:
        return img, kept
    exact = [np.concatenate([np.asarray(samples[si][0], dtype=np.float64).reshape(-1, 2), np.asarray(samples[si][1], dtype=np.float64).reshape(-1, 2)])
             for si in kept]
    exact_ptr = np.concatenate([[0], np.cumsum([len(e) for e in exact])]).astype(np.int64)
    return img, kept, _bottleneck_to_exact(pd_hat, edge_ptr, torch.from_numpy(np.concatenate(exact)).cuda(), torch.from_numpy(exact_ptr).cuda())


# ---- the packed route: tensors in, tensors out, nothing per graph ---------------------------------------------------------------------
COMPONENTS = ("largest", "whole")
PACKED_FILTS = ("degree", "centrality", "clustering", "hks", "ricci")


def _item(data):
    if hasattr(data, "edge_index"):
        return int(data.num_nodes), np.asarray(data.edge_index.cpu()).T.reshape(-1, 2)
    return _edges_nodes(data)


def pack_dataset(dataset, gn=None):
    """The first `gn` items of `dataset` (None: all) -- PyG-like items with num_nodes and edge_index [2, m], or (n, edges[m, 2]) tuples,
    mixed as they come -- as one packed batch on the device: (node_ptr int64[B + 1], edge_ptr int64[B + 1], edges int32[sum m, 2]), the
    edges RAW, exactly as the items hold them.  One concatenation on the host and three copies; no device op per graph."""
    import torch
    items = [_item(dataset[t]) for t in range(len(dataset) if gn is None else gn)]
    node_ptr = np.zeros(len(items) + 1, dtype=np.int64)
    edge_ptr = np.zeros(len(items) + 1, dtype=np.int64)
    np.cumsum(np.asarray([n for n, _ in items], dtype=np.int64), out=node_ptr[1:])
    np.cumsum(np.asarray([len(e) for _, e in items], dtype=np.int64), out=edge_ptr[1:])
    edges = np.concatenate([e for _, e in items] + [np.zeros((0, 2), dtype=np.int64)]).astype(np.int32)
    return torch.from_numpy(node_ptr).cuda(), torch.from_numpy(edge_ptr).cuda(), torch.from_numpy(edges).cuda()


class PackedGroundTruth:
    """What `ground_truth_packed` returns; every field a tensor on the device.  For a batch of B graphs of which S are ok:
      ok [B] bool                                  the graphs that have a ground truth (the others are the reference's (None, None))
      node_ptr, edge_ptr int64[S + 1]              the extracted batch of the ok graphs, in their order: the chosen component of each,
      edges int32[sum m, 2], old_id int64[sum k]   renumbered, rows (lo, hi) ascending; old_id = the input's local id of every node
      f float64[sum k]                             the filtration on the extracted batch
      d0, d1 float64[., 2], o0, o1 int64[S + 1]    Ord0 and Ext1 of the ok graphs, packed: d0[o0[i] : o0[i + 1]] is graph i's
      img, PI0, PI1 float64[B, 25]                 the images (Ord0 ++ Ext1, Ord0, Ext1), rows of zeros where not ok"""
    FIELDS = ("ok", "node_ptr", "edge_ptr", "edges", "old_id", "f", "d0", "o0", "d1", "o1", "img", "PI0", "PI1")

    def __init__(self, **fields):
        assert set(fields) == set(self.FIELDS)
        self.__dict__.update(fields)

    def tuples(self):
        """The reference's 9-tuple per ok graph (:166) and (None, None) per other one, on the host: the list
        `compute_persistence_image_batch` returns.  The only place of the packed route that loops over graphs."""
        import torch
        h = {k: getattr(self, k).cpu().numpy() for k in self.FIELDS}
        out = [(None, None)] * len(h["ok"])
        for i, gi in enumerate(np.flatnonzero(h["ok"])):
            n0, n1, e0, e1 = h["node_ptr"][i], h["node_ptr"][i + 1], h["edge_ptr"][i], h["edge_ptr"][i + 1]
            edge_index = torch.from_numpy(h["edges"][e0:e1].T.astype(np.int64))
            out[gi] = (h["d0"][h["o0"][i]:h["o0"][i + 1]], h["d1"][h["o1"][i]:h["o1"][i + 1]], h["img"][gi], h["f"][n0:n1].tolist(), edge_index,
                       h["PI0"][gi], h["PI1"][gi], 0.0, 0.0)
        return out


def ground_truth_packed(node_ptr, edge_ptr, edges, filt='degree', hks_time=10, component='largest', filtrations=None, hks_large='host', hks_sparse='host',
                        pd_large='host', kappa=None):
    """The ground truth of a packed batch of RAW graphs (`pack_dataset`) without a loop over graphs -> `PackedGroundTruth`.
    component='largest': `call`'s semantics -- the largest connected component of every graph, renumbered (`largest_component`, here
    `engine.graph_components`), a ground truth where it has an edge.  component='whole': `compute_persistence_image_batch`'s semantics on
    the deduplicated graph -- a ground truth where the graph is connected and has an edge (the component then IS the graph).
    filt 'degree' / 'centrality' / 'clustering': `engine.struct_batch` on the extracted batch; 'hks': `data_utils_LP.hks_filtration_device`
    at hks_time (hks_large as there); `filtrations`: a packed float64 tensor over the ORIGINAL nodes instead, gathered through old_id.
    filt='ricci' with kappa float64[sum m], one curvature per RAW packed edge (rows that repeat a pair carry the same value; the first
    one in the input's order is read): `ricci_filtration_device` on the extracted batch with the weights kappa + 1 and the root new id 0.
    Diagrams from `engine.pd_from_filtration` (zero-persistence pairs kept; pd_large as there), the three images from `engine.pi_raster`
    with the batch function's rule for an empty Ord0 or Ext1 (:128-137).  The values are those of `compute_persistence_image_batch` with
    the device backends on the same graphs, bit for bit: the same kernels on the same packed input.
    Host reads, per call and never per graph: the input's totals (one read), the status together with the extracted batch's totals (one
    read), and what `hks_filtration_device`, `pd_from_filtration` and the two `autograd.pack_rows` read themselves.  A graph the kernel
    refuses (offsets out of order, an id outside 0 .. n-1) raises RuntimeError naming the first one."""
    import torch
    from ..autograd import pack_rows
    from .data_utils_LP import STRUCT_DEVICE_FILTS, check_hks_large, check_hks_sparse, hks_filtration_device
    if component not in COMPONENTS:
        raise ValueError("component should be one of %s, not %r" % (COMPONENTS, component))
    check_hks_large(hks_large)
    check_hks_sparse(hks_sparse)
    engine.check_pd_large(pd_large)
    if filtrations is None and filt not in PACKED_FILTS:
        raise NotImplementedError("data_utils_GC (HIP): filt is one of %s here; pass `filtrations` for anything else" % (PACKED_FILTS,))
    if filtrations is None and filt == 'ricci' and kappa is None:
        raise _need_curvature("kappa: a float64 tensor with one value per packed edge")
    dev, B = node_ptr.device, node_ptr.numel() - 1
    i64 = dict(dtype=torch.int64, device=dev)
    zero, ar = torch.zeros(1, **i64), torch.arange(B, **i64)
    n_g = node_ptr[1:] - node_ptr[:-1]
    tot_n, max_n = torch.stack([node_ptr[-1], n_g.max()]).tolist() if B else (0, 0)
    cc = engine.graph_components(node_ptr, edge_ptr, edges, total_nodes=tot_n, max_nodes=max_n)
    k, m, c, s = cc["info"].to(torch.int64).unbind(1)
    bad = cc["status"] != _lib.ST_OK
    ok = ((m > 0) if component == 'largest' else ((c == 1) & (s > 0))) & ~bad
    first_bad, S, K, M = torch.stack([torch.where(bad, ar, B).min() if B else zero[0], ok.sum(), (k * ok).sum(), (m * ok).sum()]).tolist()
    if first_bad < B:
        raise RuntimeError("ground_truth_packed: graph %d: TLC_ST_BAD_INPUT (offsets out of order or beyond the totals, or an edge id "
                           "outside 0 .. n-1); no graph of the batch is returned" % first_bad)
    # the ok graphs in ascending order, and the offsets of the batch their components form
    sel = torch.argsort(~ok, stable=True)[:S]
    ks, ms = k[sel], m[sel]
    node_ptr2, edge_ptr2 = torch.cat([zero, ks.cumsum(0)]), torch.cat([zero, ms.cumsum(0)])
    # every kept node of an ok graph writes its old local id to where its new id puts it (the others into a spare last entry)
    owner = torch.repeat_interleave(ar, n_g, output_size=tot_n)
    new_id = cc["new_id"].to(torch.int64)
    slot = node_ptr2[(torch.cumsum(ok, 0) - 1).clamp(min=0)]
    dest = torch.where(ok[owner] & (new_id >= 0), slot[owner] + new_id, K)
    old_id = torch.empty(K + 1, **i64)
    old_id[dest] = torch.arange(tot_n, **i64) - node_ptr[owner]
    old_id = old_id[:K]
    gn = torch.repeat_interleave(torch.arange(S, **i64), ks, output_size=K)
    ge = torch.repeat_interleave(torch.arange(S, **i64), ms, output_size=M)
    edges2 = cc["out_edges"][torch.arange(M, **i64) - edge_ptr2[ge] + edge_ptr[sel][ge]].reshape(-1, 2).contiguous()
    img, PI0, PI1 = (torch.zeros((B, 25), dtype=torch.float64, device=dev) for _ in range(3))
    if S == 0:
        e2, e1 = torch.zeros((0, 2), dtype=torch.float64, device=dev), torch.zeros(0, dtype=torch.float64, device=dev)
        return PackedGroundTruth(ok=ok, node_ptr=node_ptr2, edge_ptr=edge_ptr2, edges=edges2, old_id=old_id, f=e1, d0=e2, o0=zero, d1=e2, o1=zero,
                                 img=img, PI0=PI0, PI1=PI1)
    if filtrations is not None:
        f = filtrations.to(torch.float64)[node_ptr[sel][gn] + old_id].contiguous()
    elif filt == 'ricci':
        # the raw row of every extracted edge: both as keys (lo, hi) over the input's node numbers, the raw ones sorted (stable: the
        # first of equal rows), the extracted ones looked up
        base = node_ptr[torch.repeat_interleave(ar, edge_ptr[1:] - edge_ptr[:-1], output_size=edges.shape[0])]
        raw = edges.to(torch.int64)
        raw_key = (base + raw.min(1).values) * (tot_n + 1) + base + raw.max(1).values
        raw_key, raw_row = torch.sort(raw_key, stable=True)
        e2 = old_id[node_ptr2[ge][:, None] + edges2.to(torch.int64)] + node_ptr[sel][ge][:, None]
        row = raw_row[torch.searchsorted(raw_key, e2.min(1).values * (tot_n + 1) + e2.max(1).values)]
        f = ricci_filtration_device(node_ptr2, edge_ptr2, edges2, (kappa.to(torch.float64)[row] + 1.0).contiguous(), K)
    elif filt == 'hks':
        f = hks_filtration_device(node_ptr2, edge_ptr2, edges2, hks_time, K, hks_large=hks_large, hks_sparse=hks_sparse)
    else:
        # the extracted batch is simple and in range by construction: the status byte is not read back (a refused graph would be NaN)
        f = engine.struct_batch(node_ptr2, edge_ptr2, edges2, filt, normalise=True, total_nodes=K)[0][0]
    r = engine.pd_from_filtration(node_ptr2, edge_ptr2, edges2, f, _lib.KEEP_ZERO_PERS, want_rank=False, pd_large=pd_large)
    c0, c1 = r["counts"][:, 0].to(torch.int64).clamp(min=0), r["counts"][:, 2].to(torch.int64).clamp(min=0)
    d0, o0 = pack_rows(r["up"], node_ptr2[:-1], c0)
    d1, o1 = pack_rows(r["one"], edge_ptr2[:-1], c1)
    # Ord0 ++ Ext1 per graph (:163): row j of graph i comes from d0 while j < c0[i], from d1 behind it
    T = d0.shape[0] + d1.shape[0]
    ob = o0 + o1
    own = torch.repeat_interleave(torch.arange(S, **i64), c0 + c1, output_size=T)
    pos = torch.arange(T, **i64) - ob[own]
    both = torch.cat((d0, d1))[torch.where(pos < c0[own], o0[own] + pos, d0.shape[0] + o1[own] + pos - c0[own])]
    has0, has1 = (c0 > 0)[:, None], (c1 > 0)[:, None]
    pi0 = torch.where(has0, engine.pi_raster(o0, d0, 5), 0.0)
    pi1 = torch.where(has1, engine.pi_raster(o1, d1, 5), 0.0)
    img[sel] = torch.where(has0, torch.where(has1, engine.pi_raster(ob, both, 5), pi0), pi1)
    PI0[sel], PI1[sel] = pi0, pi1
    return PackedGroundTruth(ok=ok, node_ptr=node_ptr2, edge_ptr=edge_ptr2, edges=edges2, old_id=old_id, f=f, d0=d0, o0=o0, d1=d1, o1=o1,
                             img=img, PI0=PI0, PI1=PI1)


def call_packed(dataset, name, filt='degree', hks_time=10, gn=0, save_dir=None, store=None, hks_large='host', hks_sparse='host', pd_large='host'):
    """`call` through the packed route: the first `gn` graphs of `dataset` in one `pack_dataset` and one `ground_truth_packed`
    (component='largest').  Leaves in `store`, and in <save_dir>/<name>_<filt>_total_test.pkl, what `call` leaves with the device
    backends; returns (0, 0) like it, and prints nothing per graph."""
    import os
    import pickle
    from .data_utils_LP import check_hks_large, check_hks_sparse
    check_hks_large(hks_large)
    check_hks_sparse(hks_sparse)
    engine.check_pd_large(pd_large)
    gt = ground_truth_packed(*pack_dataset(dataset, gn), filt=filt, hks_time=hks_time, component='largest', hks_large=hks_large, hks_sparse=hks_sparse, pd_large=pd_large)
    dict_store = {} if store is None else store
    dict_store.update(enumerate(gt.tuples()))
    if save_dir is not None:
        with open(os.path.join(save_dir, name + '_' + filt + '_total_test.pkl'), 'wb') as f:
            pickle.dump(dict_store, f, pickle.HIGHEST_PROTOCOL)
    return 0, 0


def evaluate_packed(model, gt, bottleneck=False):
    """`evaluate_batch` on a `PackedGroundTruth` without the per-sample loop: the block-diagonal edge_index (the real edges, then one self
    loop per node), x = f.float(), graph_ptr and edge_ptr straight from gt's tensors.  Returns float32 CUDA [n_kept, 25] images + kept
    indices (one read: the ok flags).  bottleneck=True: a third value, float64 CUDA [n_kept]: d_B of every kept graph's predicted diagram
    against gt's exact Ord0 ++ Ext1, as `evaluate_batch` returns it."""
    import torch
    kept = torch.nonzero(gt.ok).flatten().tolist()
    if not kept:
        empty = torch.zeros(0, 25, device="cuda")
        return (empty, kept, torch.zeros(0, dtype=torch.float64, device="cuda")) if bottleneck else (empty, kept)
    K = gt.f.numel()
    base = torch.repeat_interleave(gt.node_ptr[:-1], gt.edge_ptr[1:] - gt.edge_ptr[:-1], output_size=gt.edges.shape[0])
    loops = torch.arange(K, dtype=torch.int64, device=gt.f.device)
    edge_index = torch.cat([(gt.edges.to(torch.int64) + base[:, None]).t(), torch.stack([loops, loops])], dim=1)
    with torch.no_grad():
        pd_hat, img, *_ = model(gt.f.float().view(-1, 1), edge_index, None, compute_loss=False, grad_PI=False, graph_ptr=gt.node_ptr,
                                edge_ptr=gt.edge_ptr)
    if not bottleneck:
        return img, kept
    # Ord0 ++ Ext1 per graph: two slots per graph in the concatenation of the two packed arrays
    from ..autograd import pack_rows
    starts = torch.stack([gt.o0[:-1], gt.o1[:-1] + gt.d0.shape[0]], 1).flatten()
    cnt = torch.stack([gt.o0[1:] - gt.o0[:-1], gt.o1[1:] - gt.o1[:-1]], 1).flatten()
    exact, offs = pack_rows(torch.cat([gt.d0, gt.d1]), starts, cnt)
    return img, kept, _bottleneck_to_exact(pd_hat, gt.edge_ptr, exact, offs[::2].contiguous())

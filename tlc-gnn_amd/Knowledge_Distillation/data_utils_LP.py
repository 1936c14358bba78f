"""Drop-in for the vicinity / filtration part of the reference's Knowledge_Distillation/data_utils_LP.py (PDGNN, link
prediction), filt='ricci'.

  ricci_filtration.build_fv :35-65, compute_persistence_image :105-200 (modes 'filtration' and 'PI').

Differences from the TLC-GNN vicinity (sg2dgm/riccidist2dgm.py) that the HIP kernels take as flags: the two roots are always
part of the subgraph (:111), there is no connectivity assert (an unreachable root costs the sentinel 100, :41-49) and the
normalisation divides by max + 1e-10 (:64).  Node labels of a vicinity are positions in ASCENDING original id (the reference's
`convert_node_labels_to_integers` order is arbitrary); edges are listed once, lower label first.
filt='degree' (:131-133) and 'hks' (:128-130, the signature's default): the same vicinities, f from `structural_filtration` (host side:
networkx's arithmetic, scipy's eigh); hks_backend='device': 'hks' from `tlc_hks_batch` instead (a Jacobi eigensolver in HIP, values to rounding),
and with hks_large='device' the vicinities above its 256-node cap from `tlc_hks_large_batch` (exp(-tL) by fp64 matrix products) instead of the host;
struct_backend='device': 'degree' / 'centrality' / 'clustering' from `tlc_struct_batch` instead (integer counting in HIP, the same bits).  The CBGNN cycle helpers (:256-448, dead code in the reference) and `call` are not reproduced.
"""
import sys

import numpy as np

from .. import engine, _lib

KD_LP_FLAGS = _lib.INCLUDE_ROOTS | _lib.NORM_EPS | _lib.UNREACHABLE_100


STRUCTURAL_FILTS = ("degree", "centrality", "clustering", "hks")
HKS_BACKENDS = ("host", "device")
STRUCT_BACKENDS = ("host", "device")
STRUCT_DEVICE_FILTS = ("degree", "centrality", "clustering")      # what struct_backend='device' computes with tlc_struct_batch
# graphs of the most recent hks_backend='device' computation (this module's, data_utils_NC's or data_utils_GC's) that the device did not
# take -- more than _lib.HKS_NMAX nodes, or no convergence -- and that `hks_signature` computed on the host instead
hks_host_fallback = 0
# hks_large: who computes the graphs `tlc_hks_batch` leaves at TLC_ST_TOO_LARGE -- 'host' (`hks_signature`, the default) or 'device'
# (`engine.hks_large_batch`, up to _lib.HKS_LARGE_NMAX nodes and hks_time inside [0, _lib.HKS_LARGE_TIME_MAX]; values to rounding)
HKS_LARGE = ("host", "device")
# graphs of the most recent hks_backend='device' computation that the large tier (hks_large='device') computed
hks_large_device = 0
# hks_sparse: who computes what is still TLC_ST_TOO_LARGE after the large tier (more than _lib.HKS_LARGE_NMAX nodes, or hks_large='host')
# -- 'host' (`hks_signature`, the default) or 'device' (`engine.hks_sparse_batch`: no node cap, hks_time inside
# [0, _lib.HKS_SPARSE_TIME_MAX]; values to rounding)
HKS_SPARSE = ("host", "device")
# graphs of the most recent hks_backend='device' computation that the sparse tier (hks_sparse='device') computed
hks_sparse_device = 0


def check_hks_backend(hks_backend):
    if hks_backend not in HKS_BACKENDS:
        raise ValueError("hks_backend should be one of %s, not %r" % (HKS_BACKENDS, hks_backend))


def check_hks_large(hks_large):
    if hks_large not in HKS_LARGE:
        raise ValueError("hks_large should be one of %s, not %r" % (HKS_LARGE, hks_large))


def check_hks_sparse(hks_sparse):
    if hks_sparse not in HKS_SPARSE:
        raise ValueError("hks_sparse should be one of %s, not %r" % (HKS_SPARSE, hks_sparse))


def check_struct_backend(struct_backend):
    if struct_backend not in STRUCT_BACKENDS:
        raise ValueError("struct_backend should be one of %s, not %r" % (STRUCT_BACKENDS, struct_backend))


def hks_signature(n, edges, time):
    """hks_signature of the reference (data_utils_LP.py:96-100, data_utils_NC.py:88-92, data_utils_GC.py:90-94): the heat-kernel
    signature sum_k exp(-t lambda_k) phi_k(x)^2 of the normalised Laplacian -- the same scipy calls on the same kind of matrix
    (`csgraph.laplacian(A, normed=True)`, dense `eigh`), n nodes, edges int[m, 2] local ids.  Host side: a dense symmetric
    eigenproblem per graph.  Node order: ascending id here, networkx's subgraph order there -- the values of a node agree to
    rounding (1e-12), bit for bit when the orders coincide (data_utils_GC: nodes 0..n-1)."""
    import scipy.sparse as sp
    from scipy.sparse import csgraph
    from scipy.linalg import eigh
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    A = sp.csr_matrix((np.ones(2 * len(e), dtype=np.int64), (np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]]))), shape=(n, n))
    L = csgraph.laplacian(A, normed=True)
    egvals, egvectors = eigh(L.toarray())
    return np.square(egvectors).dot(np.diag(np.exp(-time * egvals))).sum(axis=1)


def structural_filtration(kind, node_ptr, edge_ptr, edges, hks_time=0.1):
    """The node functions of the induced subgraph that the reference computes with networkx (data_utils_LP.py:131-133 'degree';
    data_utils_NC.py:124-135 'centrality', 'clustering', 'degree'), each divided by (max + 1e-10), for a packed batch of
    vicinities: node_ptr / edge_ptr int64[B+1], edges int[sum m, 2] local ids -> float64[sum n].  Host side (numpy + scipy.sparse):
    they are functions of a few hundred nodes; the vicinities themselves come from the device.  Same operations in the same
    order as networkx, so the values are the reference's bit for bit -- for SIMPLE graphs, which is what the extraction hands over
    (graph2pi strips self loops): an edge (a, a) would count into `degree` and the triangle counts here, networkx's clustering drops
    it; a one-node vicinity gets centrality 1 like nx.degree_centrality (not the division by n - 1 = 0):
      degree      d                                  (subgraph.degree())
      centrality  d * (1.0 / (n - 1.0))              (nx.degree_centrality)
      clustering  t / (d * (d - 1)), t = sum over the neighbours w of |N(v) & N(w)| (each triangle twice), 0 where t == 0
                                                      (nx.clustering, unweighted)
      hks         `hks_signature` at time hks_time    (a dense eigenproblem per vicinity)"""
    import scipy.sparse as sp
    if kind not in STRUCTURAL_FILTS:
        raise ValueError("filt should be one of %s" % (STRUCTURAL_FILTS,))
    node_ptr = np.asarray(node_ptr, dtype=np.int64)
    edge_ptr = np.asarray(edge_ptr, dtype=np.int64)
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    N = int(node_ptr[-1])
    if kind == "hks":                                        # (:128-130 / :120-122: hks_signature, then /= max + 1e-10, per graph)
        out = np.zeros(N, dtype=np.float64)
        for k in range(len(node_ptr) - 1):
            a, b = int(node_ptr[k]), int(node_ptr[k + 1])
            if b > a:
                v = hks_signature(b - a, edges[int(edge_ptr[k]):int(edge_ptr[k + 1])], hks_time)
                out[a:b] = v / (max(v) + 1e-10)
        return out
    owner = np.repeat(np.arange(len(node_ptr) - 1), np.diff(node_ptr))
    base = np.repeat(node_ptr[:-1], np.diff(edge_ptr))
    a, b = edges[:, 0] + base, edges[:, 1] + base
    deg = np.bincount(np.concatenate([a, b]), minlength=N).astype(np.int64)
    if kind == "degree":
        raw = deg.astype(np.float64)
    elif kind == "centrality":
        n_of = np.diff(node_ptr)[owner].astype(np.float64)
        raw = np.where(n_of > 1.0, deg.astype(np.float64) * (1.0 / np.where(n_of > 1.0, n_of - 1.0, 1.0)), 1.0)   # (n == 1: nx returns 1)
    else:
        A = sp.csr_matrix((np.ones(2 * len(a), dtype=np.int64), (np.concatenate([a, b]), np.concatenate([b, a]))), shape=(N, N))
        t = np.asarray((A @ A).multiply(A).sum(axis=1)).reshape(-1).astype(np.int64)
        den = (deg * (deg - 1)).astype(np.float64)
        raw = np.where(t > 0, t.astype(np.float64) / np.where(den > 0, den, 1.0), 0.0)
    mx = np.zeros(len(node_ptr) - 1, dtype=np.float64)
    if N:
        np.maximum.at(mx, owner, raw)
    return raw / (mx[owner] + 1e-10) if N else raw


def hks_filtration_device(node_ptr, edge_ptr, edges, hks_time, total_nodes, hks_large='host', hks_sparse='host'):
    """The 'hks' case of `structural_filtration` on the device: `engine.hks_batch` (tlc_hks_batch) on the CUDA tensors of a packed batch
    -> CUDA float64[sum n], normalised per graph.  Offsets and edges stay on the device.  Graphs the kernel does not take (status
    TLC_ST_TOO_LARGE: more than _lib.HKS_NMAX nodes; TLC_ST_NOT_CONVERGED) are computed by `hks_signature` on the host and scattered
    in -- one extra copy, only when there are any; their number is left in the module's `hks_host_fallback`.
    hks_large='device' (and 0 <= hks_time <= _lib.HKS_LARGE_TIME_MAX): the TLC_ST_TOO_LARGE graphs of at most _lib.HKS_LARGE_NMAX nodes go
    through `engine.hks_large_batch` (tlc_hks_large_batch) into the same tensor first -- their sizes come from the status and offsets
    read-back; their number is left in the module's `hks_large_device` -- and only what is still not TLC_ST_OK afterwards takes the host.
    The device takes SIMPLE graphs, each undirected edge listed once: TLC_ST_BAD_INPUT (offsets out of order, an id outside 0 .. n-1, a
    self loop, an unordered pair listed twice -- in the same or in both directions) raises RuntimeError; nothing is returned for such a
    batch.  The host route differs there: scipy sums repeated entries into a weighted multigraph.
    hks_sparse='device' (and 0 <= hks_time <= _lib.HKS_SPARSE_TIME_MAX): what is still TLC_ST_TOO_LARGE after that -- any node count --
    goes through `engine.hks_sparse_batch` (tlc_hks_sparse_batch), with the edge offsets read back as well; the number of graphs it
    computed is left in the module's `hks_sparse_device`.  The default 'host' changes nothing."""
    global hks_host_fallback, hks_large_device, hks_sparse_device
    import torch
    check_hks_large(hks_large)
    check_hks_sparse(hks_sparse)
    f2, st = engine.hks_batch(node_ptr, edge_ptr, edges, [hks_time], normalise=True, total_nodes=total_nodes)
    f = f2[0]
    rest = torch.nonzero(st != _lib.ST_OK).reshape(-1).cpu().numpy()
    hks_host_fallback = len(rest)
    hks_large_device = 0
    hks_sparse_device = 0
    if len(rest):
        bad = ("hks_backend='device': a graph has offsets out of order, an edge id out of range, a self loop or a repeated "
               "edge (the device wants each undirected edge once; hks_backend='host' sums repeated edges into weights)")
        st_h = st.cpu().numpy()
        if (st_h[rest] == _lib.ST_BAD_INPUT).any():
            raise RuntimeError(bad)
        nptr = node_ptr.cpu().numpy()
        if hks_large == 'device' and 0.0 <= float(hks_time) <= _lib.HKS_LARGE_TIME_MAX:
            sizes = nptr[rest + 1] - nptr[rest]
            take = (st_h[rest] == _lib.ST_TOO_LARGE) & (sizes <= _lib.HKS_LARGE_NMAX)
            if take.any():
                engine.hks_large_batch(node_ptr, edge_ptr, edges, rest[take].tolist(), sizes[take].tolist(), [hks_time], normalise=True,
                                       total_nodes=total_nodes, out=f2, status=st)
                st_l = st.cpu().numpy()[rest[take]]
                if (st_l == _lib.ST_BAD_INPUT).any():
                    raise RuntimeError(bad)
                hks_large_device = int((st_l == _lib.ST_OK).sum())
                rest = np.concatenate([rest[~take], rest[take][st_l != _lib.ST_OK]])
                rest.sort()
                hks_host_fallback = len(rest)
        if hks_sparse == 'device' and 0.0 <= float(hks_time) <= _lib.HKS_SPARSE_TIME_MAX and len(rest):
            take = st.cpu().numpy()[rest] == _lib.ST_TOO_LARGE
            if take.any():
                eptr = edge_ptr.cpu().numpy()
                sel = rest[take]
                engine.hks_sparse_batch(node_ptr, edge_ptr, edges, sel.tolist(), (nptr[sel + 1] - nptr[sel]).tolist(),
                                        (eptr[sel + 1] - eptr[sel]).tolist(), [hks_time], normalise=True, total_nodes=total_nodes, out=f2, status=st)
                st_s = st.cpu().numpy()[sel]
                if (st_s == _lib.ST_BAD_INPUT).any():
                    raise RuntimeError(bad)
                hks_sparse_device = int((st_s == _lib.ST_OK).sum())
                rest = np.concatenate([rest[~take], sel[st_s != _lib.ST_OK]])
                rest.sort()
                hks_host_fallback = len(rest)
    if len(rest):
        eptr, e = edge_ptr.cpu().numpy(), edges.cpu().numpy()
        idx, val = [], []
        for k in rest:
            a, b = int(nptr[k]), int(nptr[k + 1])
            v = hks_signature(b - a, e[int(eptr[k]):int(eptr[k + 1])], hks_time)
            idx.append(np.arange(a, b))
            val.append(v / (max(v) + 1e-10))
        f[torch.from_numpy(np.concatenate(idx)).to(f.device)] = torch.from_numpy(np.concatenate(val)).to(f.device)
    return f


def struct_filtration_device(kind, node_ptr, edge_ptr, edges, total_nodes):
    """The 'degree' / 'centrality' / 'clustering' cases of `structural_filtration` on the device: `engine.struct_batch` (tlc_struct_batch)
    on the CUDA tensors of a packed batch -> CUDA float64[sum n], normalised per graph, the host function's values bit for bit.  Offsets
    and edges stay on the device; one byte comes back, whether any graph was refused.  There is no size cap and no host fallback.
    The device takes SIMPLE graphs, each undirected edge listed once: TLC_ST_BAD_INPUT (offsets out of order, an id outside 0 .. n-1, a
    self loop, an unordered pair listed twice -- in the same or in both directions) raises RuntimeError; nothing is returned for such a
    batch.  The host route differs there: it counts repeated entries into a multigraph's degrees."""
    f, st = engine.struct_batch(node_ptr, edge_ptr, edges, kind, normalise=True, total_nodes=total_nodes)
    if bool((st != _lib.ST_OK).any()):
        raise RuntimeError("struct_backend='device': a graph has offsets out of order, an edge id out of range, a self loop or a repeated "
                           "edge (the device wants each undirected edge once; struct_backend='host' counts repeated edges into the degrees)")
    return f[0]


class Vicinities:
    """Device-resident weighted graph for PDGNN's edge-centred vicinities; build once, query many pairs.
    ricci_curv=None: no curvature (the structural filtrations need only the vicinities): unit edge weights."""

    def __init__(self, g, ricci_curv):
        from ..sg2dgm.riccidist2dgm import graph2pi, _edge_array
        if ricci_curv is None:
            e = _edge_array(g)
            ricci_curv = np.concatenate([np.concatenate([e, e[:, ::-1]]).astype(np.float64), np.zeros((2 * len(e), 1))], axis=1)
        self._g2p = graph2pi(g, ricci_curv, keep_labels=True)   # kappa+1 weights (riccidist2dgm.py:216-226)
        self.dict_node = self._g2p.dict_node
        self.inv = np.arange(self._g2p.n_nodes, dtype=np.int64)
        for old, new in self.dict_node.items():
            self.inv[new] = old

    def batch(self, pairs, hop, node_cap=None, edge_cap=None, flags=None, filt='ricci', hks_time=0.1, hks_backend='host', struct_backend='host',
              hks_large='host', hks_sparse='host'):
        """pairs: [E,2] original labels -> dict of CUDA tensors: node_ptr int64[E+1], edge_ptr int64[E+1], ids int64 (original
        labels, ascending inside a vicinity), f float64, edges int32 [sum m, 2] (local ids, lower first), status uint8[E].
        Vicinities without an edge have empty slices (the reference returns (None, None) for them, :117-118).
        filt: 'ricci' (the weighted-distance filtration of the device kernels) or one of STRUCTURAL_FILTS (f replaced by
        `structural_filtration` of the extracted vicinities).
        hks_backend: 'host' (scipy's eigh per vicinity on copies of offsets and edges) or 'device' (`hks_filtration_device` on the tensors
        the extraction produced; the dict then also has hks_host_fallback and hks_large_device); it matters for filt='hks' only.
        hks_large: 'host' or 'device', who computes the vicinities above _lib.HKS_NMAX nodes (`hks_filtration_device`); it matters for
        filt='hks' with hks_backend='device' only.
        struct_backend: 'host' (`structural_filtration` on copies of offsets and edges) or 'device' (`struct_filtration_device` on the tensors
        the extraction produced: the same bits, no copy of offsets or edges); it matters for filt 'degree' / 'centrality' / 'clustering' only.
        node_cap / edge_cap: per-pair capacities of an intermediate layout (one extraction; raises if a vicinity is larger); neither
        given: sizes first, exact offsets, two extractions (`tlc_vicinity_sizes` + `tlc_pack_offsets`)."""
        import torch
        check_hks_backend(hks_backend)
        check_struct_backend(struct_backend)
        check_hks_large(hks_large)
        check_hks_sparse(hks_sparse)
        dev_graph = self._g2p._device_graph()
        mapped = torch.from_numpy(self._g2p._map_pairs(pairs)).cuda()
        fl = KD_LP_FLAGS if flags is None else flags
        if getattr(self, "_inv_dev", None) is None or self._inv_dev.device != mapped.device:
            self._inv_dev = torch.from_numpy(self.inv).to(mapped.device)
        if node_cap is None and edge_cap is None:
            # no capacities given: sizes first (the extraction alone), exact offsets from them, then the filtration writes the packed
            # batch directly -- nothing to guess, nothing to overflow (a capacity of "whole graph" per pair would be 60 GB for 100 000
            # PubMed pairs), at the price of extracting twice
            n0, m0 = dev_graph.vicinity_sizes(mapped, hop, flags=fl)
            node_ptr, edge_ptr, totals = engine.pack_offsets(n0, m0)
            E = len(n0)
            lo_n, _, tot_n, tot_m = totals.tolist() if E else (0, 0, 0, 0)
            if lo_n < 0:
                raise RuntimeError("a vicinity has more nodes than the packed local ids hold (status TLC_ST_TOO_LARGE)")
            _, ids, f, n, st, _, edges, m = dev_graph.vicinity_filtration(mapped, hop, flags=fl, zero=False,
                                                                         offsets=(node_ptr, edge_ptr, tot_n, tot_m))
            counts_n, counts_m = node_ptr[1:] - node_ptr[:-1], edge_ptr[1:] - edge_ptr[:-1]
            # the second pass wrote what the first one counted?  (a vicinity that fails inside the tier kernel writes no edges: its
            # slice of the exact-size arrays would be uninitialised memory)
            ok_n = torch.where(edge_ptr[1:] > edge_ptr[:-1], n.long() == counts_n, torch.ones_like(counts_n, dtype=torch.bool))
            if E and not bool((ok_n & (m.long() == counts_m)).all()):
                raise RuntimeError("Vicinities.batch: the filtration pass wrote other sizes than the sizes pass counted "
                                   "(a vicinity failed in its tier kernel, or the graph has self loops / one-sided entries)")
            owner = torch.arange(E, device=mapped.device)
            pn = torch.repeat_interleave(owner, counts_n, output_size=int(tot_n))
            pe = torch.repeat_interleave(owner, counts_m, output_size=int(tot_m))
            out_ids, out_f, out_e = self._inv_dev[ids[:int(tot_n)].long()], f[:int(tot_n)], edges[:int(tot_m)]
            if filt == 'hks' and hks_backend == 'device':
                out_f = hks_filtration_device(node_ptr, edge_ptr, out_e, hks_time, int(tot_n), hks_large=hks_large, hks_sparse=hks_sparse)
                return dict(node_ptr=node_ptr, edge_ptr=edge_ptr, ids=out_ids, f=out_f, edges=out_e, status=st, pair_of_node=pn, pair_of_edge=pe,
                            hks_host_fallback=hks_host_fallback, hks_large_device=hks_large_device, hks_sparse_device=hks_sparse_device)
            if filt in STRUCT_DEVICE_FILTS and struct_backend == 'device':
                out_f = struct_filtration_device(filt, node_ptr, edge_ptr, out_e, int(tot_n))
            elif filt != 'ricci':
                out_f = torch.from_numpy(structural_filtration(filt, node_ptr.cpu().numpy(), edge_ptr.cpu().numpy(), out_e.cpu().numpy(),
                                                               hks_time=hks_time)).to(out_f.device)
            return dict(node_ptr=node_ptr, edge_ptr=edge_ptr, ids=out_ids, f=out_f, edges=out_e, status=st, pair_of_node=pn, pair_of_edge=pe)
        n_cap = dev_graph.n_nodes if node_cap is None else int(node_cap)
        e_cap = max(dev_graph.nnz // 2, 1) if edge_cap is None else int(edge_cap)
        offs, ids, f, n, st, eoffs, edges, m = dev_graph.vicinity_filtration(mapped, hop, flags=fl, cap=n_cap, edge_cap=e_cap, zero=False)
        # packed offsets on the device (one kernel; no edge -> (None, None): an empty slice); ONE host read: the two totals (to size
        # the packed arrays) and the two capacity checks
        E = len(n)
        node_ptr, edge_ptr, totals = engine.pack_offsets(n, m)
        lo_n, lo_m, tot_n, tot_m = totals.tolist() if E else (0, 0, 0, 0)
        if lo_n < 0 or lo_m < 0:
            raise RuntimeError("vicinity larger than the requested node_cap / edge_cap")
        out_ids, out_f, out_e, pn, pe = engine.pack_vicinities(offs, ids, f, eoffs, edges, node_ptr, edge_ptr, int(tot_n), int(tot_m),
                                                               label=self._inv_dev)
        if filt == 'hks' and hks_backend == 'device':
            out_f = hks_filtration_device(node_ptr, edge_ptr, out_e, hks_time, int(tot_n), hks_large=hks_large, hks_sparse=hks_sparse)
            return dict(node_ptr=node_ptr, edge_ptr=edge_ptr, ids=out_ids, f=out_f, edges=out_e, status=st, pair_of_node=pn, pair_of_edge=pe,
                        hks_host_fallback=hks_host_fallback, hks_large_device=hks_large_device, hks_sparse_device=hks_sparse_device)
        if filt in STRUCT_DEVICE_FILTS and struct_backend == 'device':
            out_f = struct_filtration_device(filt, node_ptr, edge_ptr, out_e, int(tot_n))
        elif filt != 'ricci':
            out_f = torch.from_numpy(structural_filtration(filt, node_ptr.cpu().numpy(), edge_ptr.cpu().numpy(), out_e.cpu().numpy(),
                                                           hks_time=hks_time)).to(out_f.device)
        return dict(node_ptr=node_ptr, edge_ptr=edge_ptr, ids=out_ids, f=out_f, edges=out_e, status=st, pair_of_node=pn, pair_of_edge=pe)


def stacked(batch):
    """A `Vicinities.batch` result -> (x float32 [n,1], edge_index int64 [2, m+n]): all vicinities as ONE block-diagonal input of
    Teacher_Model.forward (pass graph_ptr=batch['node_ptr'], edge_ptr=batch['edge_ptr']) -- what gcn_LP_GIN.Net.compute_PI (:43-64)
    builds per candidate edge: the vicinity's edge_index plus self loops (last), its filtration as a float32 column."""
    ei, x = engine.stack_batch(batch["node_ptr"], batch["edge_ptr"], batch["edges"], batch["f"])
    return x, ei


_CACHE = {}


def _vicinities(g, ricci_curv):
    """One device graph kept between calls, reused only for the SAME graph and curvature objects (held here, so their ids
    cannot pass to other objects) with an unchanged content stamp -- the rule of data_utils_NC._vicinities."""
    from .data_utils_NC import _graph_stamp
    ent = _CACHE.get("entry")
    stamp = _graph_stamp(g, ricci_curv)
    if ent is None or ent[0] is not g or ent[1] is not ricci_curv or ent[2] != stamp:
        _CACHE["entry"] = ent = (g, ricci_curv, stamp, Vicinities(g, ricci_curv))
    return ent[3]


def compute_persistence_image(g, u, v, filt='hks', hks_time=0.1, hop=2, ricci_curv=None, mode='PI', num_models=5,
                              max_loop_len=10, cycle_the=2, hks_backend='host', struct_backend='host', hks_large='host', hks_sparse='host', pd_large='host'):
    """Reference signature (:105).  filt='hks' (:128-130), 'degree' (:131-133) or 'ricci'; mode 'filtration' -> (filtration_val
    list, edge_index LongTensor[2,m]) or (None, None); mode 'PI' -> the reference's 9-tuple (times are 0).
    hks_backend, struct_backend, hks_large (not in the reference): 'host' or 'device', see `Vicinities.batch`.
    pd_large (not in the reference): 'host' or 'device': a vicinity of the HUGE class through `tlc_pd_wide` (`engine.pd_from_filtration`)."""
    import torch
    check_hks_backend(hks_backend)
    check_struct_backend(struct_backend)
    check_hks_large(hks_large)
    check_hks_sparse(hks_sparse)
    engine.check_pd_large(pd_large)
    if filt not in ('ricci', 'degree', 'hks'):
        print("Error: 'filt' should be 'hks', 'degree' or 'ricci'! ")          # :152-153
        sys.exit()
    b = _vicinities(g, ricci_curv).batch([[u, v]], hop, filt=filt, hks_time=hks_time, hks_backend=hks_backend, struct_backend=struct_backend,
                                         hks_large=hks_large, hks_sparse=hks_sparse)
    if int(b["edge_ptr"][-1]) == 0:
        return None, None
    fv = b["f"].cpu().numpy()
    edge_index = b["edges"].t().contiguous().long().cpu()
    if mode == 'filtration':
        return fv.tolist(), edge_index
    if mode != 'PI':
        raise ValueError("mode must be 'PI' or 'filtration'")
    return diagrams_and_images(b, fv, edge_index, pd_large=pd_large)


def diagrams_and_images(b, fv, edge_index, pd_large='host'):
    """mode 'PI' tail shared by the edge- and node-centred vicinities (data_utils_LP.py:178-197, data_utils_NC.py:155-183):
    original_extended_persistence (Knowledge_Distillation fork: zero-persistence pairs kept) -> Ord0, Ext1, then the three
    images PI(Ord0 ++ Ext1), PI0, PI1; the reference's 9-tuple (times are 0).  pd_large: see `engine.pd_from_filtration`."""
    import torch
    n, m = len(fv), edge_index.shape[1]
    r = engine.pd_from_filtration(torch.tensor([0, n], dtype=torch.int64, device="cuda"),
                                  torch.tensor([0, m], dtype=torch.int64, device="cuda"),
                                  b["edges"].contiguous(), b["f"].contiguous(), _lib.KEEP_ZERO_PERS, pd_large=pd_large)
    c = r["counts"][0].cpu().numpy()
    if c[3] != 1 and int(c[2]) != m - n + int(c[3]):
        # not connected, and a Pos edge lies outside the component of the tree's root: Parent[...] of the reference's walk has no
        # such node (accelerated_PD.py:132-148, KeyError).  (Components without a cycle -- the isolated roots of a far pair -- are
        # no obstacle there either: every one of the m - n + #components Pos edges was walked.)
        raise KeyError("vicinity is not connected and a cycle lies outside the root's component: the reference's Accelerate_PD raises "
                       "here (accelerated_PD.py:132-148)")
    ord0, ext1 = r["up"][:c[0]], r["one"][:c[2]]

    def img(pts):
        if pts.shape[0] == 0:
            return np.zeros(25)
        return engine.pi_raster(torch.tensor([0, pts.shape[0]], dtype=torch.int64, device="cuda"), pts.contiguous(), 5)[0].cpu().numpy()
    PI0, PI1 = img(ord0), img(ext1)
    both = torch.cat((ord0, ext1))
    pers_img = PI1 if c[0] == 0 else (PI0 if c[2] == 0 else img(both))
    return ord0.cpu().numpy(), ext1.cpu().numpy(), pers_img, fv.tolist(), edge_index, PI0, PI1, 0.0, 0.0


def load_ricci_file(filename):
    """The reference's curvature cache: one `u v kappa` line per directed edge (data_utils_LP.py:233-240 writes it)."""
    ricci_list = []
    with open(filename) as f:
        for line in f:
            a, b, k = line.split()
            ricci_list.append([int(a), int(b), float(k)])
    return ricci_list


def compute_ricci_curvature(data, data_name, cache_dir='./data/curvature', method="Sinkhorn"):
    """data_utils_LP.py:202-242: Ollivier-Ricci curvature (alpha 0.5, Sinkhorn) of data.edge_index, cached as a text file of
    `u v kappa` lines.  The reference delegates to GraphRicciCurvature and writes under a hard-wired absolute path; here the
    curvature comes from the GPU (loaddatas.compute_ricci_curvature -> tlc_ollivier_ricci_sinkhorn) and the path is a
    parameter (None disables the cache).  method="OTD": the exact transport distance instead (tlc_ollivier_ricci_otd, see
    loaddatas.compute_ricci_curvature), cached under a name of its own (suffix `_otd`), so neither method is ever served the other's
    file; not reproduced there: the library's nbr_topk cut, weighted graphs, directed graphs."""
    import os
    from ..loaddatas import compute_ricci_curvature as _compute, RICCI_METHODS
    if method not in RICCI_METHODS:
        raise ValueError("compute_ricci_curvature: method must be 'Sinkhorn' or 'OTD', got %r" % (method,))
    stem = 'graph_' + data_name + '_removevaltest' + ('_otd' if method == "OTD" else '')
    filename = os.path.join(cache_dir, stem + '.edge_list') if cache_dir else None
    if filename and os.path.exists(filename):
        print("curvature file exists, directly loading")
        return load_ricci_file(filename)
    ricci_list = _compute(data, method=method)
    if filename:
        os.makedirs(os.path.dirname(filename), exist_ok=True)
        with open(filename, 'w') as f:
            for a, b, k in ricci_list:
                f.write(str(a) + " " + str(b) + " " + repr(float(k)) + "\n")
    return ricci_list

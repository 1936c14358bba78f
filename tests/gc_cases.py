"""Graphs and the reference shared by tests/test_cpu_gc_packed_host.py and tests/test_gpu_gc_packed.py (tlc_graph_components and the
packed route of data_utils_GC).  A graph is (n, edges int64[m, 2]) with RAW edges: both orientations, repeats and self loops as they come.

`restate` is the contract of include/tlcgnn.h restated in numpy, written from the header's text: it does not call
`data_utils_GC.largest_component` (the CPU test compares the two)."""
import functools

import numpy as np

E0 = np.zeros((0, 2), dtype=np.int64)


# ---- the contract ---------------------------------------------------------------------------------------------------------------------
def restate(n, edges):
    """-> dict(k, m, c, s, new_id int32[n], out_edges int32[m, 2]) of one graph, as the header states them."""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    assert n >= 0 and (len(e) == 0 or (e.min() >= 0 and e.max() < n)), "the contract refuses such a graph"
    if n == 0:
        return dict(k=0, m=0, c=0, s=0, new_id=np.zeros(0, dtype=np.int32), out_edges=np.zeros((0, 2), dtype=np.int32))
    e = e[e[:, 0] != e[:, 1]]                                          # the simple graph: no loops,
    key = np.unique(np.minimum(e[:, 0], e[:, 1]) * n + np.maximum(e[:, 0], e[:, 1]))      # each unordered pair once, (lo, hi) ascending
    lo, hi = key // n, key % n
    parent = list(range(n))                                            # union-find; the label of a component is its lowest id

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in zip(lo.tolist(), hi.tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    label = np.array([find(v) for v in range(n)], dtype=np.int64)
    size = np.bincount(label, minlength=n)
    winner = int(np.argmax(size))                                      # most nodes; argmax takes the first of equals: the lowest label
    keep = label == winner
    new_id = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
    sel = keep[lo]
    out = np.stack([new_id[lo[sel]], new_id[hi[sel]]], 1).astype(np.int32).reshape(-1, 2)
    return dict(k=int(keep.sum()), m=int(sel.sum()), c=int((label == np.arange(n)).sum()), s=int(len(key)), new_id=new_id, out_edges=out)


def dedup(n, edges):
    """the simple graph itself: rows (lo, hi), ascending"""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    e = e[e[:, 0] != e[:, 1]]
    return n, np.unique(np.sort(e, 1), axis=0).reshape(-1, 2)


# ---- generators -----------------------------------------------------------------------------------------------------------------------
def raw(edges, seed, loops=0, n=None):
    """both orientations of every edge, some rows twice, `loops` self loops, shuffled"""
    rs = np.random.RandomState(seed)
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    parts = [e, e[:, ::-1], e[rs.random_sample(len(e)) < 0.3]]
    if loops:
        parts.append(np.repeat(rs.randint(0, n, size=loops), 2).reshape(-1, 2))
    e = np.concatenate(parts)
    return e[rs.permutation(len(e))]


def sparse(n, m, seed):
    rs = np.random.RandomState(seed)
    return n, (rs.randint(0, n, size=(m, 2)).astype(np.int64) if n else E0)


def path(n, seed):
    """a path through all n nodes under a random relabelling: diameter n - 1"""
    p = np.random.RandomState(seed).permutation(n)
    return n, np.stack([p[:-1], p[1:]], 1).astype(np.int64)


def star(n, seed):
    p = np.random.RandomState(seed).permutation(n)
    return n, np.stack([np.full(n - 1, p[0]), p[1:]], 1).astype(np.int64)


def complete_both(n):
    i, j = np.nonzero(~np.eye(n, dtype=bool))
    return n, np.stack([i, j], 1).astype(np.int64)


def disjoint_edges(k, seed):
    """k disjoint edges on 2 k nodes, relabelled so that node 0 does not sit in the first edge listed"""
    p = np.random.RandomState(seed).permutation(2 * k)
    e = p.reshape(k, 2).astype(np.int64)
    first = int(np.flatnonzero((e == 0).any(1))[0])
    if first == 0:
        e = np.roll(e, 1, axis=0)
    return 2 * k, e


def fourfold_with_loops(n, m, seed):
    """every edge four times in mixed orientation, plus a self loop on every node"""
    rs = np.random.RandomState(seed)
    e = rs.randint(0, n, size=(m, 2)).astype(np.int64)
    e = np.concatenate([e, e[:, ::-1], e, e[:, ::-1], np.repeat(np.arange(n), 2).reshape(-1, 2)])
    return n, e[rs.permutation(len(e))]


def strict_subset(n, seed):
    """a sparse random graph (about 0.8 n random pairs, raw): many components, the largest a strict subset"""
    n_, e = sparse(n, int(0.8 * n), seed)
    return n, raw(e, seed + 1, loops=n // 50, n=n)


FIVE = (5, np.array([[3, 1], [1, 3], [2, 0], [4, 4]], dtype=np.int64))      # {0, 2} and {1, 3}: the lower id is in the later-listed one


@functools.lru_cache(maxsize=None)
def cases():
    """[(name, (n, edges))]: the list of the issue, every case once per session"""
    out = [("n%d" % n, (n, raw(sparse(n, n + n // 2, 10 + n)[1], 20 + n, loops=min(n, 3), n=n) if n else E0)) for n in (0, 1, 2, 63, 64, 65, 66, 129, 1025, 70000)]
    out += [("edgeless5", (5, E0)), ("edgeless100", (100, E0)), ("K64 both", complete_both(64)),
            ("path64", path(64, 1)), ("path70000", path(70000, 2)), ("star70000", star(70000, 3)),
            ("isolated64", (64, E0)), ("isolated3000", (3000, E0)),
            ("pairs32", disjoint_edges(32, 4)), ("pairs35000", disjoint_edges(35000, 5)),
            ("five", FIVE), ("two equal wide", (200, np.array([[150 + i, 151 + i] for i in range(49)] + [[i, i + 1] for i in range(49)], dtype=np.int64))),
            ("fourfold40", fourfold_with_loops(40, 60, 6)), ("fourfold300", fourfold_with_loops(300, 500, 7)),
            ("subset200", strict_subset(200, 8)), ("subset1500", strict_subset(1500, 9)), ("subset70000", strict_subset(70000, 10))]
    twin = strict_subset(500, 11)
    out += [("twin a", twin), ("twin b", twin), ("edgeless wide", (300, E0)), ("after the edgeless", strict_subset(400, 12))]
    return out


@functools.lru_cache(maxsize=None)
def references():
    """{name: restate(graph)}, computed once"""
    return {name: restate(*g) for name, g in cases()}


def pack(graphs):
    node_ptr = np.concatenate([[0], np.cumsum([g[0] for g in graphs])]).astype(np.int64)
    edge_ptr = np.concatenate([[0], np.cumsum([len(g[1]) for g in graphs])]).astype(np.int64)
    edges = np.concatenate([np.asarray(g[1], dtype=np.int64).reshape(-1, 2) for g in graphs] + [E0]).astype(np.int32)
    return node_ptr, edge_ptr, edges


def expected(packed, refs, sentinel=-1):
    """the four outputs of a packed batch from its graphs' references (None: a refused graph), slots prefilled with `sentinel`"""
    node_ptr, edge_ptr, edges = packed
    info = np.full((len(refs), 4), sentinel, dtype=np.int32)
    new_id = np.full(int(node_ptr[-1]), sentinel, dtype=np.int32)
    out_edges = np.full((len(edges), 2), sentinel, dtype=np.int32)
    for g, r in enumerate(refs):
        if r is None:
            continue
        info[g] = (r["k"], r["m"], r["c"], r["s"])
        new_id[node_ptr[g]:node_ptr[g + 1]] = r["new_id"]
        out_edges[edge_ptr[g]:edge_ptr[g] + r["m"]] = r["out_edges"]
    return info, new_id, out_edges


@functools.lru_cache(maxsize=None)
def many_small_batch(n_graphs=20000, seed=5):
    """20 000 random raw graphs of at most 16 nodes (more than any grid: every wavefront draws several tickets) with three WIDE ones
    sprinkled in -> (graphs, packed)"""
    rs = np.random.RandomState(seed)
    sizes = rs.randint(0, 17, size=n_graphs)
    counts = rs.randint(0, 40, size=n_graphs)
    graphs = [(int(n), rs.randint(0, n, size=(int(m), 2)).astype(np.int64) if n else E0) for n, m in zip(sizes, counts)]
    for pos, g in ((137, strict_subset(700, 40)), (9999, path(3000, 41)), (19990, strict_subset(65, 42))):
        graphs[pos] = g
    return graphs, pack(graphs)


def route_graphs(seed=77, n_graphs=300):
    """about 300 raw graphs for the packed route: molecule-like trees with chords, edgeless and single-node graphs, disconnected ones,
    a few above 64 nodes, everything in both orientations with repeats and loops"""
    rs = np.random.RandomState(seed)
    out = []
    for i in range(n_graphs):
        kind = i % 10
        if kind == 7:
            out.append((int(rs.randint(1, 6)), E0))                                  # edgeless (single-node among them)
            continue
        n = int(rs.randint(70, 200)) if kind == 3 else int(rs.randint(2, 40))
        par = np.array([rs.randint(0, v) for v in range(1, n)], dtype=np.int64)
        e = np.stack([par, np.arange(1, n)], 1).reshape(-1, 2)
        e = np.concatenate([e, rs.randint(0, n, size=(int(rs.randint(0, 4)), 2))])
        if kind in (5, 8) and n > 4:                                                 # cut into components: drop the edges across a split
            cut = int(rs.randint(1, n - 1))
            e = e[(e[:, 0] < cut) == (e[:, 1] < cut)]
        p = rs.permutation(n)
        out.append((n, raw(p[e], int(rs.randint(1 << 30)), loops=int(rs.randint(0, 3)), n=n)))
    out[1] = (1, E0)
    out[2] = (1, np.array([[0, 0]], dtype=np.int64))
    return out

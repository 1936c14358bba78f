"""Graphs and references shared by tests/test_cpu_struct_host.py and tests/test_gpu_struct.py (the degree / centrality / clustering
filtrations).  A graph is (n, edges int64[m, 2]): simple, each undirected edge once, lower id first."""
import functools

import numpy as np

KINDS = ("degree", "centrality", "clustering")
EPS = 1e-10


def _canon(pairs):
    e = np.asarray(sorted({(min(a, b), max(a, b)) for a, b in pairs if a != b}), dtype=np.int64).reshape(-1, 2)
    return e


def complete(n):
    i, j = np.triu_indices(n, 1)
    return n, np.stack([i, j], 1).astype(np.int64)


def star(n):
    """hub 0, n - 1 leaves"""
    return n, np.stack([np.zeros(n - 1, dtype=np.int64), np.arange(1, n, dtype=np.int64)], 1)


def bipartite(a, b):
    i, j = np.meshgrid(np.arange(a), a + np.arange(b), indexing="ij")
    return a + b, np.stack([i.reshape(-1), j.reshape(-1)], 1).astype(np.int64)


def gnp(n, p, seed):
    rs = np.random.RandomState(seed)
    if n <= 2048:
        i, j = np.nonzero(np.triu(rs.random_sample((n, n)) < p, 1))
        return n, np.stack([i, j], 1).astype(np.int64)
    m = int(p * n * (n - 1) / 2)                              # a large sparse graph: about m distinct random pairs
    a, b = rs.randint(n, size=m), rs.randint(n, size=m)
    keep = a != b
    lo, hi = np.minimum(a, b)[keep], np.maximum(a, b)[keep]
    key = np.unique(lo * n + hi)
    return n, np.stack([key // n, key % n], 1).astype(np.int64)


def planted_clique(n, k, seed, p=None):
    """a sparse random graph on n nodes in which k nodes spread over the whole id range are made a clique AND cut off from the rest:
    each of them has d = k - 1 and t = (k - 1)(k - 2), clustering exactly 1.0 before normalisation"""
    n_, e = gnp(n, (4.0 / n) if p is None else p, seed)
    members = np.unique(np.linspace(0, n - 1, k).astype(np.int64))
    assert len(members) == k
    inside = np.isin(e[:, 0], members) | np.isin(e[:, 1], members)
    i, j = np.triu_indices(k, 1)
    e = np.concatenate([e[~inside], np.stack([members[i], members[j]], 1)])
    return n, e[np.lexsort((e[:, 1], e[:, 0]))], members


def two_components_and_isolated(n, seed):
    """a random connected part on the first third, a cycle on the second third, the rest isolated (at least one node)"""
    a, b = max(n // 3, 1), max(2 * n // 3, 2)
    rs = np.random.RandomState(seed)
    pairs = [(int(rs.randint(i)), i) for i in range(1, a)] + [(int(x), int(y)) for x, y in rs.randint(a, size=(a, 2))]
    if b - a >= 3:
        pairs += [(a + i, a + (i + 1) % (b - a)) for i in range(b - a)]
    elif b - a == 2:
        pairs += [(a, a + 1)]
    return n, _canon(pairs)


def pack(graphs):
    node_ptr = np.concatenate([[0], np.cumsum([g[0] for g in graphs])]).astype(np.int64)
    edge_ptr = np.concatenate([[0], np.cumsum([len(g[1]) for g in graphs])]).astype(np.int64)
    edges = np.concatenate([np.asarray(g[1], dtype=np.int64).reshape(-1, 2) for g in graphs] + [np.zeros((0, 2), dtype=np.int64)]).astype(np.int32)
    return node_ptr, edge_ptr, edges


def host(kind, packed):
    from tlc_gnn_amd.Knowledge_Distillation.data_utils_LP import structural_filtration
    return structural_filtration(kind, *packed)


# ---- closed forms: (name, graph, {kind: raw values}) -- exact in fp64 ---------------------------------------------------------------
def closed_form_cases():
    k23 = bipartite(2, 3)
    return [
        ("K5", complete(5), dict(degree=[4.0] * 5, centrality=[4 * (1.0 / 4.0)] * 5, clustering=[12.0 / 12.0] * 5)),
        ("star7", star(7), dict(degree=[6.0] + [1.0] * 6, centrality=[6 * (1.0 / 6.0)] + [1 * (1.0 / 6.0)] * 6, clustering=[0.0] * 7)),
        ("K2,3", k23, dict(degree=[3.0, 3.0, 2.0, 2.0, 2.0], centrality=[3 * (1.0 / 4.0)] * 2 + [2 * (1.0 / 4.0)] * 3, clustering=[0.0] * 5)),
        ("one node", (1, np.zeros((0, 2), dtype=np.int64)), dict(degree=[0.0], centrality=[1.0], clustering=[0.0])),
        ("three isolated", (3, np.zeros((0, 2), dtype=np.int64)), dict(degree=[0.0] * 3, centrality=[0.0] * 3, clustering=[0.0] * 3)),
    ]


def normalised(raw):
    raw = np.asarray(raw, dtype=np.float64)
    return raw / (raw.max() + EPS)


# ---- tier edges -----------------------------------------------------------------------------------------------------------------------
def tier_edge_graphs(N):
    """the graphs of one tier boundary N: N - 1, N, N + 1 nodes each as G(n, p), a complete graph (n <= 65) or a planted clique, a star,
    a complete bipartite graph, and two components plus isolated nodes.  Above 2 048 nodes (the neighbour-bitmap window) the star and
    the bipartite graph are left to the smaller boundaries: their reference is a dense n x n product on the host."""
    out = []
    for n in (N - 1, N, N + 1):
        big = n > 2048
        out.append(("gnp%d" % n, gnp(n, 8.0 / n if big else min(0.5, 24.0 / n), 100 + n)))
        if n <= 65:
            out.append(("K%d" % n, complete(n)))
        else:
            k = 40 if not big else 70
            n_, e, members = planted_clique(n, k, 200 + n)
            out.append(("clique%d in %d" % (k, n), (n_, e), members))
        if not big:
            out.append(("star%d" % n, star(n)))
            out.append(("K%d,%d" % (n // 2, n - n // 2), bipartite(n // 2, n - n // 2)))
        out.append(("parts%d" % n, two_components_and_isolated(n, 300 + n)))
    return out


@functools.lru_cache(maxsize=None)
def tier_edge_batch(N):
    """-> (cases, packed, {kind: host values}) of one boundary, the reference computed once per session"""
    cases = tier_edge_graphs(N)
    packed = pack([c[1] for c in cases])
    return cases, packed, {k: host(k, packed) for k in KINDS}


@functools.lru_cache(maxsize=None)
def many_small_batch(n_graphs=20000, seed=5):
    """20 000 random graphs of 1 .. 39 nodes (every grid takes several per unit), a few larger ones of the other tiers sprinkled in"""
    rs = np.random.RandomState(seed)
    sizes = rs.randint(1, 40, size=n_graphs)
    graphs = [gnp(int(n), float(rs.uniform(0.05, 0.9)), int(rs.randint(1 << 30))) for n in sizes]
    for pos, (n, p) in ((137, (70, 0.2)), (4001, (300, 0.05)), (9999, (1100, 0.01)), (15000, (200, 0.3)), (19990, (65, 0.5)), (12345, (1500, 0.004))):
        graphs[pos] = gnp(n, p, 7000 + pos)
    packed = pack(graphs)
    return graphs, packed, {k: host(k, packed) for k in KINDS}

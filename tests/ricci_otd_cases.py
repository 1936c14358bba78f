"""Graphs, closed forms and the exact reference shared by tests/test_cpu_ricci_otd_host.py and tests/test_gpu_ricci_otd.py (the
Ollivier-Ricci curvature with the exact transport distance, method "OTD").  A graph is (n, edges int64[m, 2]): simple, each
undirected edge once, lower id first.  Curvatures are Fractions: kappa = 1 - W / D with D = den * deg(s) * deg(t) and W the integer
minimum cost of the transportation problem scaled by D."""
from fractions import Fraction

import numpy as np

_ADJ = {}
_WD = {}


def _canon(pairs):
    return np.asarray(sorted({(min(a, b), max(a, b)) for a, b in pairs if a != b}), dtype=np.int64).reshape(-1, 2)


# ---- graphs ----------------------------------------------------------------------------------------------------------------
def complete(n):
    i, j = np.triu_indices(n, 1)
    return n, np.stack([i, j], 1).astype(np.int64)


def cycle(n):
    return n, _canon([(k, (k + 1) % n) for k in range(n)])


def star(d):
    """hub 0 with d leaves"""
    return d + 1, np.stack([np.zeros(d, dtype=np.int64), np.arange(1, d + 1, dtype=np.int64)], 1)


def bipartite(p, q):
    i, j = np.meshgrid(np.arange(p), p + np.arange(q), indexing="ij")
    return p + q, np.stack([i.reshape(-1), j.reshape(-1)], 1).astype(np.int64)


def path(n):
    return n, np.stack([np.arange(n - 1), np.arange(1, n)], 1).astype(np.int64)


def gnp(n, p, seed):
    rs = np.random.RandomState(seed)
    i, j = np.nonzero(np.triu(rs.random_sample((n, n)) < p, 1))
    return n, np.stack([i, j], 1).astype(np.int64)


def random_tree(n, seed):
    rs = np.random.RandomState(seed)
    par = np.array([rs.randint(0, k) for k in range(1, n)])
    return n, _canon(zip(par.tolist(), range(1, n)))


def two_hubs(ds, dt, c, m=0, cross=0, outside=0, seed=0):
    """Adjacent hubs s = 0 (degree ds) and t = 1 (degree dt) with c common neighbours and ds - 1 - c / dt - 1 - c private leaves;
    m disjoint leaf-leaf edges between the two private sides (the closed form's family); `cross` further random leaf-leaf edges and
    `outside` extra nodes each joined to three random leaves of either side, so that all of the hop distances 0, 1, 2, 3 occur between
    the supports.  The supports of (0, 1) have ds + 1 and dt + 1 entries whatever the extras."""
    ps, pt = ds - 1 - c, dt - 1 - c
    assert ps >= 0 and pt >= 0 and m <= min(ps, pt)
    com = list(range(2, 2 + c))
    la = list(range(2 + c, 2 + c + ps))
    lb = list(range(2 + c + ps, 2 + c + ps + pt))
    n = 2 + c + ps + pt
    e = [(0, 1)] + [(0, k) for k in com + la] + [(1, k) for k in com + lb] + [(la[k], lb[k]) for k in range(m)]
    rs = np.random.RandomState(seed)
    if ps and pt:
        for _ in range(cross):
            e.append((la[rs.randint(ps)], lb[rs.randint(pt)]))
        for _ in range(outside):
            z = n
            n += 1
            e += [(z, la[k]) for k in rs.randint(ps, size=3)] + [(z, lb[k]) for k in rs.randint(pt, size=3)]
    return n, _canon(e)


# ---- closed forms at alpha = 1/2 (Fractions) -------------------------------------------------------------------------------
def kappa_complete(n):
    return Fraction(n, 2 * (n - 1))


def kappa_cycle(n):
    return {3: Fraction(3, 4), 4: Fraction(1, 2), 5: Fraction(1, 4)}.get(n, Fraction(0))


def kappa_star(d):
    return Fraction(1, d)


def kappa_bipartite(p, q):
    return Fraction(1, max(p, q))


def kappa_path(n, k):
    """edge (k, k + 1) of the path on n >= 3 nodes: an end edge 1/2, an inner edge 0"""
    return Fraction(1, 2) if k in (0, n - 2) else Fraction(0)


def kappa_two_hubs(d, c, m):
    """the hub-hub edge of two_hubs(d, d, c, m)"""
    p = d - 1 - c
    return 1 - Fraction(d - 1 + 3 * p - 2 * m, 2 * d)


# ---- the exact reference -----------------------------------------------------------------------------------------------------
def _adjacency(n, edges):
    import scipy.sparse as sp
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    key = (int(n), edges.tobytes())
    if key not in _ADJ:
        a = sp.coo_matrix((np.ones(len(edges)), (edges[:, 0], edges[:, 1])), shape=(n, n))
        _ADJ[key] = ((a + a.T) > 0).astype(np.float64).tocsr()
    return key, _ADJ[key]


def exact_wd(n, edges, s, t, num, den):
    """(W, D) as Python ints for the adjacent pair (s, t) at alpha = num / den: D = den * deg(s) * deg(t); W = the minimum of
    sum flow * hop distance over the plans that move num*deg(s)*deg(t) at s and (den-num)*deg(t) on each neighbour of s onto
    num*deg(s)*deg(t) at t and (den-num)*deg(s) on each neighbour of t.  scipy's HiGHS LP on the integer problem (its optimum is
    integral: asserted), cross-checked against networkx's network simplex where the supports are small."""
    import scipy.sparse as sp
    from scipy.optimize import linprog
    from scipy.sparse.csgraph import shortest_path
    key, adj = _adjacency(n, edges)
    key = key + (int(s), int(t), int(num), int(den))
    if key in _WD:
        return _WD[key]
    xs = np.concatenate([adj.indices[adj.indptr[s]:adj.indptr[s + 1]], [s]])
    ys = np.concatenate([adj.indices[adj.indptr[t]:adj.indptr[t + 1]], [t]])
    ds, dt = len(xs) - 1, len(ys) - 1
    assert ds >= 1 and dt >= 1 and adj[s, t] != 0
    a = np.array([(den - num) * dt] * ds + [num * ds * dt], dtype=np.int64)
    b = np.array([(den - num) * ds] * dt + [num * ds * dt], dtype=np.int64)
    if len(xs) <= len(ys):                                        # searches from the smaller support
        dist = shortest_path(adj, method="D", unweighted=True, indices=xs)[:, ys]
    else:
        dist = shortest_path(adj, method="D", unweighted=True, indices=ys)[:, xs].T
    assert np.isfinite(dist).all() and dist.max() <= 3
    cost = dist.astype(np.int64)
    na, nb = len(xs), len(ys)
    A = sp.vstack([sp.kron(sp.eye(na), np.ones((1, nb))), sp.kron(np.ones((1, na)), sp.eye(nb))]).tocsr()
    res = linprog(cost.ravel().astype(np.float64), A_eq=A, b_eq=np.concatenate([a, b]).astype(np.float64), method="highs")
    assert res.status == 0, res.message
    assert abs(res.fun - round(res.fun)) < 1e-6, res.fun
    W = int(round(res.fun))
    if na * nb <= 2500:
        import networkx as nx
        g = nx.DiGraph()
        for i in range(na):
            g.add_node(("a", i), demand=-int(a[i]))
        for j in range(nb):
            g.add_node(("b", j), demand=int(b[j]))
        for i in range(na):
            for j in range(nb):
                g.add_edge(("a", i), ("b", j), weight=int(cost[i, j]))
        flow_cost, _ = nx.network_simplex(g)
        assert flow_cost == W, (flow_cost, W)
    _WD[key] = (W, den * ds * dt)
    return _WD[key]


def exact_kappa(n, edges, pairs, num=1, den=2):
    """(kappa float64, W int64, D int64) of the pairs: kappa = 1.0 - W / D in Python (int / int true division is correctly rounded)"""
    wd = [exact_wd(n, edges, int(s), int(t), num, den) for s, t in np.asarray(pairs).reshape(-1, 2).tolist()]
    W = np.array([w for w, _ in wd], dtype=np.int64)
    D = np.array([d for _, d in wd], dtype=np.int64)
    return np.array([1.0 - w / d for w, d in wd], dtype=np.float64), W, D


def reduced_problem(n, edges, s, t, num=1, den=2):
    """(excess int64[na], deficit int64[nb], hop codes int64[na, nb]) of the pair (s, t) after the mass of the nodes of both supports
    has been cancelled in place: what csrc/ricci_otd_solve.h is handed by the kernels"""
    from scipy.sparse.csgraph import shortest_path
    _, adj = _adjacency(n, edges)
    xs = np.concatenate([adj.indices[adj.indptr[s]:adj.indptr[s + 1]], [s]])
    ys = np.concatenate([adj.indices[adj.indptr[t]:adj.indptr[t + 1]], [t]])
    ds, dt = len(xs) - 1, len(ys) - 1
    a = np.array([(den - num) * dt] * ds + [num * ds * dt], dtype=np.int64)
    b = np.array([(den - num) * ds] * dt + [num * ds * dt], dtype=np.int64)
    if len(xs) <= len(ys):
        dist = shortest_path(adj, method="D", unweighted=True, indices=xs)[:, ys]
    else:
        dist = shortest_path(adj, method="D", unweighted=True, indices=ys)[:, xs].T
    pos = {int(y): j for j, y in enumerate(ys)}
    for i, x in enumerate(xs.tolist()):
        j = pos.get(x)
        if j is not None:
            c = min(a[i], b[j])
            a[i] -= c
            b[j] -= c
    return a, b, dist.astype(np.int64)

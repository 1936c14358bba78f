"""A numpy restatement of the heat-kernel signature and of its derivative in the diffusion time: the oracle of
tests/test_gpu_hks_dt.py, checked on the CPU by tests/test_cpu_hks_dt_host.py.

    L = I' - D^-1/2 A D^-1/2    (I': a node of degree 0 has diagonal 0, as scipy.sparse.csgraph.laplacian(normed=True))
    hks_t(v)      =   sum_k exp(-t lambda_k) phi_k(v)^2
    d/dt hks_t(v) = - sum_k lambda_k exp(-t lambda_k) phi_k(v)^2
    f = hks / (mx + 1e-10), mx = hks(a) at the LOWEST index a of the maximum:  d f(v) / d t = (hks'(v) - f(v) hks'(a)) / (mx + 1e-10)

A graph is (n, edges): edges int64[m, 2] local ids, each undirected edge once."""
import numpy as np


def _edges(pairs):
    return np.array(sorted(pairs), dtype=np.int64).reshape(-1, 2)


def complete(n):
    return n, _edges((i, j) for i in range(n) for j in range(i + 1, n))


def star(n):
    """K(1, n - 1): node 0 is the centre (n = 1: one isolated node)"""
    return n, _edges((0, i) for i in range(1, n))


def cycle(n):
    """C_n, n >= 3"""
    assert n >= 3
    return n, _edges([(i, i + 1) for i in range(n - 1)] + [(0, n - 1)])


def path_plus_isolated(n):
    """a path on the first max(n - 2, 0) nodes; the last two nodes (all of them for n <= 3) have degree 0"""
    return n, _edges((i, i + 1) for i in range(n - 3))


def gnp(n, p, seed):
    """G(n, p): every pair independently; isolated nodes and several components are welcome"""
    rs = np.random.RandomState(seed)
    iu, ju = np.triu_indices(n, 1)
    keep = rs.random_sample(len(iu)) < p
    return n, np.stack([iu[keep], ju[keep]], 1).astype(np.int64).reshape(-1, 2)


def random_connected(n, seed, extra=None):
    """a random tree plus about `extra` (default n) further edges: simple, connected, each edge once"""
    rs = np.random.RandomState(seed)
    es = {(int(rs.randint(i)), i) for i in range(1, n)}
    for _ in range((n if extra is None else extra) if n > 2 else 0):
        a, b = (int(x) for x in rs.randint(n, size=2))
        if a != b:
            es.add((min(a, b), max(a, b)))
    return n, _edges(es)


def bipartite(a, b):
    return a + b, _edges((i, a + j) for i in range(a) for j in range(b))


def laplacian(n, edges):
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    A = np.zeros((n, n))
    A[e[:, 0], e[:, 1]] = 1.0
    A[e[:, 1], e[:, 0]] = 1.0
    deg = A.sum(1)
    s = np.where(deg > 0, 1.0 / np.sqrt(np.where(deg > 0, deg, 1.0)), 0.0)
    return np.diag((deg > 0).astype(np.float64)) - s[:, None] * A * s[None, :]


def eigenpairs(n, edges):
    if n == 0:
        return np.zeros(0), np.zeros((0, 0))
    return np.linalg.eigh(laplacian(n, edges))


def eigen_form(n, edges, t, pairs=None):
    """(hks_t, d/dt hks_t), float64[n] each, from one eigh (pairs: what `eigenpairs` returned, to share it among times)"""
    lam, phi = eigenpairs(n, edges) if pairs is None else pairs
    w = np.exp(-t * lam)
    return (phi * phi) @ w, -((phi * phi) @ (lam * w))


def neighbour_form(n, edges, t):
    """d/dt hks_t(v) = -[K_t]_vv + sum over the neighbours u of v of [K_t]_uv / sqrt(d_u d_v), K_t = exp(-t L): what the large tier sums"""
    lam, phi = eigenpairs(n, edges)
    K = (phi * np.exp(-t * lam)) @ phi.T
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    deg = np.bincount(e.reshape(-1), minlength=n).astype(np.float64)
    out = -np.diag(K).copy()
    for a, b in e:
        w = K[a, b] / np.sqrt(deg[a] * deg[b])
        out[a] += w
        out[b] += w
    out[deg == 0] = 0.0
    return out


def quotient(val, dval):
    """(f, d f / d t) of the normalised signature; np.argmax returns the first index of the maximum"""
    if len(val) == 0:
        return val.copy(), dval.copy()
    a = int(np.argmax(val))
    den = val[a] + 1e-10
    f = val / den
    return f, (dval - f * dval[a]) / den


# ---- closed forms of d/dt hks_t, float64[n] ----------------------------------------------------------------------------------------------
def d_complete(n, t):
    return np.zeros(1) if n == 1 else np.full(n, -np.exp(-t * n / (n - 1.0)))


def d_star(n, t):
    """K(1, k), k = n - 1 >= 1: centre -exp(-2t); leaf -((k - 1) / k exp(-t) + exp(-2t) / k)"""
    if n == 1:
        return np.zeros(1)
    k = n - 1.0
    out = np.full(n, -((k - 1.0) / k * np.exp(-t) + np.exp(-2.0 * t) / k))
    out[0] = -np.exp(-2.0 * t)
    return out


def d_cycle(n, t):
    lam = 1.0 - np.cos(2.0 * np.pi * np.arange(n) / n)
    return np.full(n, -(lam * np.exp(-t * lam)).sum() / n)


def d_bipartite(a, b, t):
    """K(a, b): a node of the side of size s has -((1 - 1/s) exp(-t) + exp(-2t) / s)"""
    side = lambda s: -((1.0 - 1.0 / s) * np.exp(-t) + np.exp(-2.0 * t) / s)
    return np.concatenate([np.full(a, side(float(a))), np.full(b, side(float(b)))])


def pack(graphs):
    """-> (node_ptr int64[B + 1], edge_ptr int64[B + 1], edges int32[sum m, 2]) numpy arrays of a list of (n, edges)"""
    node_ptr = np.concatenate([[0], np.cumsum([n for n, _ in graphs])]).astype(np.int64)
    edge_ptr = np.concatenate([[0], np.cumsum([len(e) for _, e in graphs])]).astype(np.int64)
    edges = np.concatenate([np.zeros((0, 2), dtype=np.int64)] + [np.asarray(e, dtype=np.int64).reshape(-1, 2) for _, e in graphs])
    return node_ptr, edge_ptr, edges.astype(np.int32).reshape(-1, 2)

"""Shared helpers for the parity tests."""
import numpy as np


def sorted_points(a):
    """Diagram as a sorted multiset: point order carries no meaning."""
    a = np.asarray(a, dtype=np.float64).reshape(-1, 2)
    if len(a) == 0:
        return a
    return a[np.lexsort((a[:, 1], a[:, 0]))]


def same_multiset(a, b):
    a, b = sorted_points(a), sorted_points(b)
    return a.shape == b.shape and np.array_equal(a, b)


def ragged_slice(flat, offs, i):
    return flat[offs[i]:offs[i + 1]]


def rel_err(a, b, floor=1e-300):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return np.abs(a - b) / np.maximum(np.abs(b), floor)


def random_connected(n, seed):
    """a random tree plus about 2n extra edges: simple, connected, each edge once (lower id first)"""
    rs = np.random.RandomState(seed)
    es = {(int(rs.randint(i)), i) for i in range(1, n)}
    for _ in range(2 * n if n > 1 else 0):
        a, b = (int(x) for x in rs.randint(n, size=2))
        if a != b:
            es.add((min(a, b), max(a, b)))
    return np.array(sorted(es), dtype=np.int64).reshape(-1, 2)


# ---- heat-kernel signatures in closed form (un-normalised: sum_k exp(-t lambda_k) phi_k(x)^2 of the normalised Laplacian) ----------
# Each family's spectrum is known by hand, so these values depend on no eigensolver: the device kernel and the host route (scipy's
# eigh) are both measured against them.
HKS_CLOSED_FORM_SIZES = (2, 3, 31, 32, 33, 64, 65, 96, 97, 255, 256)
HKS_CLOSED_FORM_TIMES = (0.0, 0.01, 0.1, 1.0, 10.0, 100.0, 1000.0, 0.5)


def hks_bound(t):
    """1e-11 (the bound the project tests up to t = 10) scaled by the linear-in-t error model t * p(n) * u * ||L|| of a backward-stable
    eigensolver (tests/test_gpu_hks.py's docstring)"""
    return 1e-11 * max(1.0, t / 10.0)


def _complete(n):
    """K_n: eigenvalue 0 once, n/(n-1) with multiplicity n - 1; vertex transitive"""
    e = np.array([(i, j) for i in range(n) for j in range(i + 1, n)], dtype=np.int64).reshape(-1, 2)
    return e, lambda t: np.full(n, 1.0 / n + (1.0 - 1.0 / n) * np.exp(-t * n / (n - 1.0)))


def _star(n):
    """K(1,m), m = n - 1, centre 0: eigenvalues 0, 1 (m - 1 times, supported on the leaves), 2"""
    m = n - 1
    e = np.array([(0, i) for i in range(1, n)], dtype=np.int64).reshape(-1, 2)

    def f(t):
        v = np.full(n, 1.0 / (2 * m) + (m - 1.0) / m * np.exp(-t) + np.exp(-2.0 * t) / (2 * m))
        v[0] = 0.5 + np.exp(-2.0 * t) / 2
        return v
    return e, f


def _cycle(n):
    """C_n (n >= 3): eigenvalues 1 - cos(2 pi k / n), k = 0 .. n-1; vertex transitive"""
    e = np.array([(i, i + 1) for i in range(n - 1)] + [(0, n - 1)], dtype=np.int64).reshape(-1, 2)
    lam = 1.0 - np.cos(2.0 * np.pi * np.arange(n) / n)
    return e, lambda t: np.full(n, np.exp(-t * lam).mean())


def _bipartite(n):
    """K(a,b), a = n // 3 (at least 1: n = 2 is K(1,1)), b = n - a: eigenvalues 0, 1 (n - 2 times), 2"""
    a = max(1, n // 3)
    b = n - a
    e = np.array([(i, a + j) for i in range(a) for j in range(b)], dtype=np.int64).reshape(-1, 2)

    def f(t):
        side = lambda s: (1.0 + np.exp(-2.0 * t)) / (2 * s) + (1.0 - 1.0 / s) * np.exp(-t)
        return np.concatenate([np.full(a, side(a)), np.full(b, side(b))])
    return e, f


def hks_closed_form_cases(sizes=HKS_CLOSED_FORM_SIZES):
    """[(name, n, edges int64[m, 2] each edge once, f)]: f(t) -> the n un-normalised signatures at time t"""
    cases = []
    for n in sizes:
        for name, make in (("complete", _complete), ("star", _star), ("cycle", _cycle), ("bipartite", _bipartite)):
            if name == "cycle" and n < 3:
                continue
            e, f = make(n)
            cases.append(("%s%d" % (name, n), n, e, f))
    return cases


def hks_stationary(n, edges):
    """the t -> infinity limit on a connected graph, deg(x) / (2m): only the eigenvalue 0 survives, phi_0(x)^2 = deg(x) / (2m)"""
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    return np.bincount(edges.reshape(-1), minlength=n).astype(np.float64) / (2.0 * len(edges))


def csr_from_golden(d):
    from tlc_gnn_amd import synth
    return synth.edges_to_csr(int(d["n_nodes"]), d["edges"], d["kappa"])

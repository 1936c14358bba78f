"""The sparse heat-kernel-signature tier (tlc_hks_sparse_batch, csrc/hks_sparse.hip) restated in numpy, operation for operation as
include/tlcgnn.h states it, and closed forms with their derivatives in t.  Shared by tests/test_cpu_hks_sparse_host.py and
tests/test_gpu_hks_sparse.py; nothing here needs a GPU or the library.

numpy's + and * on float64 arrays are the IEEE operations (no fused multiply-add), so an array expression is the kernel's lane-wise
arithmetic; r_u, exp(-tau) and tau / k are formed with `math` on Python floats, as the kernel's host side and its per-row sqrt do."""
import math

import numpy as np

PANEL, TIME_MAX = 64, 64.0


def terms(t):
    """tlc_hks_sparse_terms, operation for operation."""
    t = float(t)
    if not 0.0 <= t <= TIME_MAX:
        return -1
    tau = t * 0.5
    if tau == 0.0:
        return 0
    E = term = 1.0
    for j in range(1, 401):
        term = term * tau / float(j)
        E = E + term
    bound, slack = 1.0 / 18446744073709551616.0, 1.0 + 1.0 / 1099511627776.0
    term = 1.0
    for k in range(1000):
        term = term * tau / float(k + 1)
        if float(k + 2) > tau and term / (1.0 - tau / float(k + 2)) / E * slack <= bound:
            return k
    return -1


class Csr:
    """symmetric CSR with ascending neighbours, and the ordered row sum R_u(x) for every u at once"""

    def __init__(self, n, edges):
        e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
        a, b = np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]])
        order = np.lexsort((b, a))
        self.n, self.col = n, b[order]
        self.rowptr = np.searchsorted(a[order], np.arange(n + 1))
        self.deg = np.diff(self.rowptr)
        self.r = np.array([1.0 / math.sqrt(float(d)) if d else 0.0 for d in self.deg], dtype=np.float64)
        self.levels = []                                       # chunk j of every row that has one: (rows, columns padded, lengths)
        j = 0
        while True:
            rows = np.nonzero(self.deg > PANEL * j)[0]
            if not len(rows):
                break
            lens = np.minimum(self.deg[rows] - PANEL * j, PANEL)
            idx = np.zeros((len(rows), PANEL), dtype=np.int64)
            for i in range(PANEL):
                has = lens > i
                idx[has, i] = self.col[self.rowptr[rows[has]] + PANEL * j + i]
            self.levels.append((rows, idx, lens))
            j += 1

    def row_sums(self, x):
        """x float64[n, C] -> R(x)[n, C]: per row, chunks of 64 neighbours ascending from +0.0, then the chunks' sums ascending from +0.0"""
        tot = np.zeros_like(x)
        for rows, idx, lens in self.levels:
            part = np.zeros((len(rows), x.shape[1]), dtype=np.float64)
            for i in range(int(lens.max())):
                has = lens > i
                part[has] = part[has] + x[idx[has, i]]
            tot[rows] = tot[rows] + part
        return tot


def _block_sums(a):
    """sum over the rows of a[n, C]: blocks of 64 consecutive rows from +0.0 ascending, then the blocks ascending from +0.0.  (The padding
    rows add +0.0 to a non-negative partial sum: no change.)"""
    n, C = a.shape
    nb = (n + PANEL - 1) // PANEL
    p = np.zeros((nb * PANEL, C), dtype=np.float64)
    p[:n] = a
    p = p.reshape(nb, PANEL, C)
    part = np.zeros((nb, C), dtype=np.float64)
    for i in range(PANEL):
        part = part + p[:, i, :]
    tot = np.zeros(C, dtype=np.float64)
    for b in range(nb):
        tot = tot + part[b]
    return tot


def restate(n, edges, t, cols=None, csr=None):
    """-> (hks_t, d hks_t / dt) float64[len(cols)] of the nodes `cols` (default: all), raw (not normalised), the kernel's bits."""
    csr = Csr(n, edges) if csr is None else csr
    cols = np.arange(n) if cols is None else np.asarray(cols, dtype=np.int64)
    C = len(cols)
    if n == 0 or C == 0:
        return np.zeros(0), np.zeros(0)
    tau = float(t) * 0.5
    factor, K = math.exp(-tau), terms(t)
    r = csr.r[:, None]
    S = np.zeros((n, C), dtype=np.float64)
    S[cols, np.arange(C)] = 1.0
    s = np.zeros((n, C), dtype=np.float64)
    s[cols, np.arange(C)] = csr.r[cols]
    for k in range(1, K + 1):
        ck = tau / float(k)
        z = (ck * r) * csr.row_sums(s)
        S = S + z
        s = r * z
    y = factor * S
    q = r * y
    val = _block_sums(y * y)
    quad = _block_sums(q * csr.row_sums(q))
    iso = csr.deg[cols] == 0
    return np.where(iso, 1.0, val), np.where(iso, 0.0, quad - val)


def normalise(val, dval):
    """TLC_HKS_NORMALISE on one graph: f = v / (mx + 1e-10), mx at its lowest index a; f' = (v' - f v'(a)) / (mx + 1e-10)"""
    a = int(np.argmax(val))                                    # (numpy's argmax: the first of equal maxima)
    mx = val[a]
    f = val / (mx + 1e-10)
    return f, (dval - f * dval[a]) / (mx + 1e-10)


# ---- graphs -----------------------------------------------------------------------------------------------------------------------------
def star(leaves):
    return leaves + 1, np.array([(0, i) for i in range(1, leaves + 1)], dtype=np.int64).reshape(-1, 2)


def cycle(n):
    return n, np.array([(i, i + 1) for i in range(n - 1)] + [(0, n - 1)], dtype=np.int64)


def bipartite(a, b):
    return a + b, np.array([(i, a + j) for i in range(a) for j in range(b)], dtype=np.int64)


def union(*graphs, isolated=0):
    """disjoint union, then `isolated` nodes without an edge"""
    n, es = 0, []
    for k, e in graphs:
        es.append(np.asarray(e, dtype=np.int64).reshape(-1, 2) + n)
        n += k
    return n + isolated, (np.concatenate(es) if es else np.zeros((0, 2), dtype=np.int64))


def random_connected(n, seed, extra=None):
    """a random tree plus about 2n extra edges: simple, connected, each edge once (lower id first)"""
    rs = np.random.RandomState(seed)
    es = {(int(rs.randint(i)), i) for i in range(1, n)}
    for _ in range((2 * n if extra is None else extra) if n > 1 else 0):
        a, b = (int(x) for x in rs.randint(n, size=2))
        if a != b:
            es.add((min(a, b), max(a, b)))
    return np.array(sorted(es), dtype=np.int64).reshape(-1, 2)


# ---- closed forms: (hks_t, d hks_t / dt) per node -----------------------------------------------------------------------------------------
def bipartite_closed(a, b, t):
    """K(a, b): the normalised Laplacian has the eigenvalues 0 and 2 (phi(v)^2 = deg(v) / 2m each) and 1 (a + b - 2 times)"""
    def side(k):
        return ((1.0 + math.exp(-2.0 * t)) / (2.0 * k) + (1.0 - 1.0 / k) * math.exp(-t),
                -2.0 * math.exp(-2.0 * t) / (2.0 * k) - (1.0 - 1.0 / k) * math.exp(-t))
    va, vb = side(a), side(b)
    return (np.concatenate([np.full(a, va[0]), np.full(b, vb[0])]), np.concatenate([np.full(a, va[1]), np.full(b, vb[1])]))


def star_closed(leaves, t):
    return bipartite_closed(1, leaves, t)


def cycle_closed(n, t):
    """C_n: the eigenvalues 1 - cos(2 pi k / n), every node the same"""
    lam = [1.0 - math.cos(2.0 * math.pi * k / n) for k in range(n)]
    v = math.fsum(math.exp(-t * x) for x in lam) / n
    d = -math.fsum(x * math.exp(-t * x) for x in lam) / n
    return np.full(n, v), np.full(n, d)


def union_closed(parts, isolated=0):
    """parts: the (value, derivative) pairs of the components; isolated nodes have value 1, derivative 0"""
    return (np.concatenate([p[0] for p in parts] + [np.ones(isolated)]), np.concatenate([p[1] for p in parts] + [np.zeros(isolated)]))


def eigh_reference(n, edges, t):
    """(hks_t, d hks_t / dt) from a dense eigendecomposition of the normalised Laplacian (diagonal 0 for a node of degree 0)"""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    A = np.zeros((n, n))
    A[e[:, 0], e[:, 1]] = 1.0
    A[e[:, 1], e[:, 0]] = 1.0
    d = A.sum(1)
    r = np.where(d > 0, 1.0 / np.sqrt(np.where(d > 0, d, 1.0)), 0.0)
    L = np.diag((d > 0).astype(np.float64)) - r[:, None] * A * r[None, :]
    w, V = np.linalg.eigh(L)
    V2 = V * V
    return V2 @ np.exp(-t * w), -(V2 @ (w * np.exp(-t * w)))

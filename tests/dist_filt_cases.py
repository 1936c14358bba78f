"""A numpy restatement of tlc_dist_filtration and tlc_dist_filtration_vjp, written from the text of include/tlcgnn.h, and the small
graphs the distance-filtration tests share.  No GPU, no library.

Value: the node-sourced Bellman-Ford, all sources at once -- D[s, y] = the minimum over paths s -> y of the left-to-right fp64 sum that
starts at s (row r of it is also the root-sourced fixpoint R_r)."""
import numpy as np

INCLUDE_ROOTS, NORM_EPS, UNREACHABLE_100, DESC_MIN, DESC_MAX, DESC_ROOT1, NO_NORM = 0x02, 0x04, 0x20, 0x40, 0x80, 0xC0, 0x100
ST_OK, ST_DISCONNECTED, ST_ZERO_RANGE, ST_BAD_INPUT = 0, 2, 3, 7


def all_sources(n, edges, w, sources=None):
    """D[k, y] for the sources given (default: every node), +inf where there is no path."""
    edges = np.asarray(edges, np.int64).reshape(-1, 2)
    w = np.asarray(w, np.float64)
    sources = np.arange(n) if sources is None else np.asarray(sources, np.int64)
    T = np.full((n, len(sources)), np.inf)                       # T[y, k] = D[k, y]: rows gather and reduce contiguously
    T[sources, np.arange(len(sources))] = 0.0
    if len(edges) == 0:
        return np.ascontiguousarray(T.T)
    src = np.concatenate([edges[:, 0], edges[:, 1]])
    dst = np.concatenate([edges[:, 1], edges[:, 0]])
    wd = np.concatenate([w, w])
    order = np.argsort(dst, kind="stable")
    src, dst, wd = src[order], dst[order], wd[order]
    heads = np.flatnonzero(np.r_[True, dst[1:] != dst[:-1]])
    targets = dst[heads]
    for _ in range(max(n - 1, 1)):
        best = np.minimum.reduceat(T[src] + wd[:, None], heads, axis=0)
        new = np.minimum(T[targets], best)
        if np.array_equal(new, T[targets]):
            break
        T[targets] = new
    return np.ascontiguousarray(T.T)


def _desc(flags, single, d0, d1):
    desc = flags & DESC_ROOT1
    if single:
        return d0.copy()
    if desc == 0:
        return d0 + d1
    return np.where(d1 < d0, d1, d0) if desc == DESC_MIN else np.where(d1 > d0, d1, d0)


def _norm(flags, q, dm):
    """(f, status) of the raw values q and the values dm whose maximum divides."""
    den0 = max(0.0, float(dm.max())) if len(dm) else 0.0
    if flags & NO_NORM:
        return q.copy(), ST_OK
    if flags & NORM_EPS:
        return q / (den0 + 1e-10), ST_OK
    if den0 == 0.0:
        return None, ST_ZERO_RANGE
    return q / den0, ST_OK


def forward(n, edges, w, r0, r1, flags, D=None):
    """-> (f float64[n] or None, status, parent int32[2, n])."""
    single = r1 < 0 or (flags & DESC_ROOT1) == DESC_ROOT1
    rr1 = r0 if single else r1
    if D is None:
        D = all_sources(n, edges, w)
    parent = np.stack([tree(n, edges, w, D[r0]), np.full(n, -1, np.int32) if single else tree(n, edges, w, D[r1])])
    if np.isinf(D[r0]).any() and not flags & UNREACHABLE_100:
        return None, ST_DISCONNECTED, parent
    d0 = np.where(np.isinf(D[:, r0]), 100.0, D[:, r0])
    d1 = np.where(np.isinf(D[:, rr1]), 100.0, D[:, rr1])
    q = _desc(flags, single, d0, d1)
    dm = np.where(d1 > d0, d1, d0) if ((flags & DESC_ROOT1) == DESC_MIN and not single) else q.copy()
    q[[r0, rr1]] = 0.0
    dm[[r0, rr1]] = 0.0
    f, st = _norm(flags, q, dm)
    return f, st, parent


def tree(n, edges, w, R):
    """P[x] = the lowest neighbour y with R[y] < R[x] and fl(R[y] + w) == R[x]; -1 for the root, unreachable nodes, nodes without one."""
    P = np.full(n, np.iinfo(np.int64).max, np.int64)
    edges = np.asarray(edges, np.int64).reshape(-1, 2)
    w = np.asarray(w, np.float64)
    for x, y in ((edges[:, 0], edges[:, 1]), (edges[:, 1], edges[:, 0])):
        with np.errstate(invalid="ignore"):
            ok = (R[y] < R[x]) & np.isfinite(R[x]) & (R[y] + w == R[x])
        np.minimum.at(P, x[ok], y[ok])
    P[P == np.iinfo(np.int64).max] = -1
    return P.astype(np.int32)


def vjp(n, edges, w, r0, r1, flags, parent, g):
    """-> (grad_w float64[m] or None, status): the header's specification, operation for operation."""
    edges = np.asarray(edges, np.int64).reshape(-1, 2)
    w = np.asarray(w, np.float64)
    g = np.asarray(g, np.float64)
    m = len(edges)
    desc = flags & DESC_ROOT1
    single = r1 < 0 or desc == DESC_ROOT1
    roots = [r0] if single else [r0, r1]
    nr = len(roots)
    edge_of = {}
    for e, (a, b) in enumerate(edges):
        edge_of[(int(a), int(b))] = e
        edge_of[(int(b), int(a))] = e
    pe = np.full((nr, n), -1, np.int64)
    T = np.zeros((2, n))
    depth = np.zeros((nr, n), np.int64)
    arrives = np.zeros((nr, n), bool)
    for r in range(nr):
        for x in range(n):
            p = int(parent[r][x])
            if p >= 0 and (x, p) in edge_of:
                pe[r, x] = edge_of[(x, p)]
        for x in range(n):
            t, c, steps = 0.0, x, 0
            while pe[r, c] >= 0 and steps < n:
                t = t + w[pe[r, c]]
                c = int(parent[r][c])
                steps += 1
            arrives[r, x] = c == roots[r]
            T[r, x] = t if arrives[r, x] else 100.0
            depth[r, x] = steps
    isroot = np.zeros(n, bool)
    isroot[roots] = True
    q = _desc(flags, single, T[0], T[1])
    dm = np.where(T[1] > T[0], T[1], T[0]) if (desc == DESC_MIN and not single) else q.copy()
    q[isroot] = 0.0
    dm[isroot] = 0.0
    den0 = max(0.0, float(dm.max()))
    normed = not flags & NO_NORM
    if not normed:
        den = 1.0
    elif flags & NORM_EPS:
        den = den0 + 1e-10
    elif den0 == 0.0:
        return None, ST_ZERO_RANGE
    else:
        den = den0
    xstar = int(np.flatnonzero(dm == den0)[0])
    a = g / den
    corr = 0.0
    if normed:
        s = 0.0
        for x in range(n):
            s = s + g[x] * q[x]
        corr = s / (den * den)
    S = np.zeros((nr, n))
    for r in range(nr):
        for x in range(n):
            if single or desc == 0:
                sel = dsel = True
            elif desc == DESC_MIN:
                sel = r == (1 if T[1, x] < T[0, x] else 0)
                dsel = r == (1 if T[1, x] > T[0, x] else 0)
            else:
                sel = dsel = r == (1 if T[1, x] > T[0, x] else 0)
            ok = arrives[r, x] and not isroot[x]
            c = a[x] if (ok and sel) else 0.0
            if normed and x == xstar and ok and dsel:
                c = c - corr
            S[r, x] = c
        children = [[] for _ in range(n)]
        for z in range(n):                               # ascending z: every list ascending
            if pe[r, z] >= 0:
                children[int(parent[r][z])].append(z)
        for lev in range(int(depth[r].max()) if n else 0, -1, -1):
            for x in np.flatnonzero(depth[r] == lev):
                s = S[r, x]
                for z in children[x]:
                    s = s + S[r, z]
                S[r, x] = s
    gw = np.zeros(m)
    for e, (p, k) in enumerate(edges):
        v = 0.0
        for r in range(nr):
            if pe[r, p] == e:
                v = v + S[r, p]
            elif pe[r, k] == e:
                v = v + S[r, k]
        gw[e] = v
    return gw, ST_OK


# ---- graphs ---------------------------------------------------------------------------------------------------------------------------
def random_connected(rng, n, m):
    """A connected simple graph: a random tree plus random extra pairs, m edges in all (m >= n - 1)."""
    pairs = set()
    perm = rng.permutation(n)
    for i in range(1, n):
        a, b = int(perm[i]), int(perm[rng.integers(0, i)])
        pairs.add((min(a, b), max(a, b)))
    limit = n * (n - 1) // 2
    while len(pairs) < min(m, limit):
        a, b = (int(v) for v in rng.integers(0, n, 2))
        if a != b:
            pairs.add((min(a, b), max(a, b)))
    e = np.array(sorted(pairs), np.int32).reshape(-1, 2)
    flip = rng.random(len(e)) < 0.5
    e[flip] = e[flip][:, ::-1]
    return e[rng.permutation(len(e))]


def path(n):
    return np.stack([np.arange(n - 1), np.arange(1, n)], 1).astype(np.int32).reshape(-1, 2)


def cycle(n):
    return np.stack([np.arange(n), (np.arange(n) + 1) % n], 1).astype(np.int32)


def star(n):
    return np.stack([np.zeros(n - 1), np.arange(1, n)], 1).astype(np.int32)


def grid(a, b):
    idx = np.arange(a * b).reshape(a, b)
    return np.concatenate([np.stack([idx[:, :-1].ravel(), idx[:, 1:].ravel()], 1), np.stack([idx[:-1].ravel(), idx[1:].ravel()], 1)]).astype(np.int32)


def generic_weights(rng, m):
    return rng.uniform(0.5, 1.9, m)


def tie_weights(rng, m):
    return rng.integers(5, 20, m) * 0.1


def pack(graphs):
    """graphs: a list of (n, edges, w, r0, r1) -> node_offs, edge_offs int64[B + 1], edges int32[M, 2], w float64[M], roots int32[B, 2]."""
    no = np.zeros(len(graphs) + 1, np.int64)
    eo = np.zeros(len(graphs) + 1, np.int64)
    for i, (n, e, w, r0, r1) in enumerate(graphs):
        no[i + 1] = no[i] + n
        eo[i + 1] = eo[i] + len(e)
    E = np.concatenate([np.asarray(gr[1], np.int32).reshape(-1, 2) for gr in graphs]) if graphs else np.zeros((0, 2), np.int32)
    W = np.concatenate([np.asarray(gr[2], np.float64).reshape(-1) for gr in graphs]) if graphs else np.zeros(0)
    R = np.array([[gr[3], gr[4]] for gr in graphs], np.int32).reshape(-1, 2)
    return no, eo, np.ascontiguousarray(E, np.int32), W, R

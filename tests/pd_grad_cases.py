"""Shared by tests/test_gpu_pd_grad.py: the graphs, and the numpy restatement of the rule and of the fixed summation order of
tlc_pd_point_vertices / tlc_pd_filtration_grad (include/tlcgnn.h).  Nothing here touches a device."""
import numpy as np

SENTINEL = 12345                 # what the tests fill the id arrays with before a call: rows the entry must not write keep it
ST_OK, ST_TOO_LARGE, ST_BAD_INPUT = 0, 5, 7
KEYS = ("up", "down", "one", "ext0")

_PAIRS = {}


def _pairs(n):
    if n not in _PAIRS:
        a, b = np.triu_indices(n, 1)
        _PAIRS[n] = np.stack([a, b], 1).astype(np.int32)
    return _PAIRS[n]


def small_graph(rs, n):
    """a random connected simple graph of n <= 16 nodes with about 1.5 n edges (fewer where the complete graph has fewer): a random
    recursive tree plus distinct further pairs"""
    if n < 2:
        return np.zeros((0, 2), dtype=np.int32)
    par = (rs.random_sample(n - 1) * np.arange(1, n)).astype(np.int64)
    child = np.arange(1, n)
    pairs = _pairs(n)
    # index of the pair (a < b) in the row-major upper triangle
    tree_idx = par * n - par * (par + 1) // 2 + (child - par - 1)
    rest = np.setdiff1d(np.arange(len(pairs)), tree_idx, assume_unique=False)
    extra = rs.permutation(rest)[:min(len(rest), n // 2)]
    E = pairs[np.concatenate([tree_idx, extra])]
    return E[rs.permutation(len(E))]


def chord_graph(rs, n, m, base="tree"):
    """n nodes, m distinct edges: a random recursive tree (or the cycle 0-1-...-n-1-0) plus random chords, orientation and order random"""
    if base == "cycle":
        first = np.stack([np.arange(n), (np.arange(n) + 1) % n], 1)
    else:
        par = (rs.random_sample(n - 1) * np.arange(1, n)).astype(np.int64)
        first = np.stack([par, np.arange(1, n)], 1)
    lo, hi = first.min(1), first.max(1)
    have = set((lo * n + hi).tolist())
    extra = []
    while len(first) + len(extra) < m:
        a = rs.randint(0, n, size=2 * (m - len(first) - len(extra)) + 8)
        b = rs.randint(0, n, size=len(a))
        for x, y in zip(np.minimum(a, b).tolist(), np.maximum(a, b).tolist()):
            if x != y and x * n + y not in have and len(first) + len(extra) < m:
                have.add(x * n + y)
                extra.append((x, y))
    E = np.concatenate([first, np.array(extra, dtype=np.int64).reshape(-1, 2)])
    flip = rs.randint(0, 2, size=len(E)).astype(bool)
    E[flip] = E[flip][:, ::-1]
    return E[rs.permutation(len(E))].astype(np.int32)


def star(n):
    return np.stack([np.zeros(n - 1, dtype=np.int32), np.arange(1, n, dtype=np.int32)], 1)


def distinct_values(rs, n):
    """n pairwise distinct values in [0, 1)"""
    return (rs.permutation(n) + rs.random_sample(n) * 0.5) / max(n, 1)


def tied_values(rs, n, mode):
    if mode == 0:
        return np.full(n, 0.25)                                   # all equal: every id is 0
    if mode == 1:
        return np.where(rs.randint(0, 2, size=n) > 0, 0.75, 0.125)     # two distinct values
    if mode == 2:
        return rs.randint(0, 4, size=n) / 3.0                     # multiples of 1/3
    v = np.array([-0.0, 0.0, 0.5])[rs.randint(0, 3, size=n)]     # both zeros: a +0.0 coordinate of vertex 1 belongs to vertex 0
    v[:2] = (-0.0, 0.0)[:n]
    return v


def mixed_batch(seed=0, n_small=20000):
    """-> (graphs [(n, E)], named {label: index}): every size class, more wavefronts than the wave tier's grid holds"""
    rs = np.random.RandomState(seed)
    graphs = [(n, small_graph(rs, n)) for n in rs.randint(1, 17, size=n_small).tolist()]
    named = {}

    def put(label, n, E, at=None):
        at = len(graphs) if at is None else at
        graphs.insert(at, (n, np.asarray(E, dtype=np.int32).reshape(-1, 2)))
        for k in named:
            if named[k] >= at:
                named[k] += 1
        named[label] = at

    put("empty", 0, [], at=n_small // 2)
    put("one", 1, [])
    put("two", 2, [[1, 0]])
    put("triangle", 3, [[0, 1], [2, 1], [0, 2]])
    put("apart", 8, [[0, 1], [1, 2], [2, 0], [3, 4], [4, 5], [5, 3], [6, 7]])          # three components
    put("star64", 64, star(64))
    for n in (63, 64, 65, 2047, 2048):
        put("n%d" % n, n, chord_graph(rs, n, n - 1 + n // 2))
    return graphs, named


def pack(graphs, fs):
    no = np.concatenate([[0], np.cumsum([g[0] for g in graphs])]).astype(np.int64)
    eo = np.concatenate([[0], np.cumsum([len(g[1]) for g in graphs])]).astype(np.int64)
    E = np.concatenate([np.asarray(g[1], dtype=np.int32).reshape(-1, 2) for g in graphs] + [np.zeros((0, 2), dtype=np.int32)])
    f = np.concatenate([np.asarray(x, dtype=np.float64).reshape(-1) for x in fs] + [np.zeros(0)])
    return no, eo, E.astype(np.int32), f


def _first_equal(fg, coords):
    """the rule: np.flatnonzero(fg == c)[0] for every c of coords, -1 where no vertex holds c (chunked, so that a big graph's
    comparison matrix stays small)"""
    out = np.empty(len(coords), dtype=np.int32)
    step = max(1, (1 << 22) // max(len(fg), 1))
    for a in range(0, len(coords), step):
        eq = fg[None, :] == coords[a:a + step, None]
        out[a:a + step] = np.where(eq.any(1), eq.argmax(1), -1)
    return out


def slots(no, eo, counts, g):
    """(key, first row, point rows, slot rows) of graph g's three slots"""
    n, m = int(no[g + 1] - no[g]), int(eo[g + 1] - eo[g])
    return (("up", int(no[g]), int(counts[g, 0]), n), ("down", int(no[g]), int(counts[g, 1]), n), ("one", int(eo[g]), int(counts[g, 2]), m))


def ref_vertices(no, eo, f, pd, which=None):
    """The restatement of tlc_pd_point_vertices for graphs whose counts rows are valid: id arrays filled with SENTINEL where the entry
    writes nothing, and the status bytes.  pd: numpy arrays up, down, one, ext0, counts."""
    B = len(no) - 1
    out = {k: np.full(pd[k].shape, SENTINEL, dtype=np.int32) for k in KEYS}
    status = np.zeros(B, dtype=np.uint8)
    for g in (range(B) if which is None else which):
        fg = f[no[g]:no[g + 1]]
        if len(fg) == 0:
            continue
        if pd["counts"][g, 0] < 0:
            status[g] = ST_TOO_LARGE if pd["counts"][g, 0] == -1 else ST_BAD_INPUT
            continue
        for key, base, cnt, rows in slots(no, eo, pd["counts"], g):
            out[key][base:base + rows] = -1
            ids = _first_equal(fg, pd[key][base:base + cnt].reshape(-1))
            out[key][base:base + cnt] = ids.reshape(-1, 2)
            if (ids < 0).any():
                status[g] = ST_BAD_INPUT
        ids = _first_equal(fg, pd["ext0"][g])
        out["ext0"][g] = ids
        if (ids < 0).any():
            status[g] = ST_BAD_INPUT
    return out, status


def ref_grad(no, eo, counts, verts, status, grads, which=None, fill=0.0):
    """The restatement of tlc_pd_filtration_grad: per vertex the sum, from +0.0, left to right over up rows (birth, death), down rows,
    one rows, ext0, of the gradients of the coordinates whose vertex it is.  grads[key] may be None (zeros).  Slices of graphs that are
    not OK keep `fill`."""
    B = len(no) - 1
    out = np.full(int(no[-1]), fill, dtype=np.float64)
    for g in (range(B) if which is None else which):
        n = int(no[g + 1] - no[g])
        if n == 0 or status[g] != ST_OK:
            continue
        acc = [0.0] * n
        parts = [(key, verts[key][base:base + cnt], None if grads[key] is None else grads[key][base:base + cnt])
                 for key, base, cnt, _ in slots(no, eo, counts, g)]
        parts.append(("ext0", verts["ext0"][g:g + 1], None if grads["ext0"] is None else grads["ext0"][g:g + 1]))
        for _, ids, gr in parts:
            ids = ids.reshape(-1).tolist()
            vals = [0.0] * len(ids) if gr is None else gr.reshape(-1).tolist()
            for v, x in zip(ids, vals):
                acc[v] += x
        out[no[g]:no[g + 1]] = acc
    return out

"""The bottleneck distance of include/tlcgnn.h (tlc_bottleneck_matching) restated in numpy + scipy, operation for operation: the cost
matrix, d_B by a threshold search, the rule that names the attaining pair of a given matching, and the gradient rule.  No GPU.
Shared by tests/test_cpu_bottleneck_host.py, tests/test_gpu_bottleneck.py and tools/time_bottleneck.py (its host route)."""
import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import maximum_bipartite_matching


def _pts(P):
    return np.asarray(P, dtype=np.float64).reshape(-1, 2)


def cost_matrix(X, Y):
    """[N, N], N = n + m: rows = X's points then m diagonal copies, columns = Y's points then n diagonal copies; fp64 subtract, abs,
    max and multiply only."""
    X, Y = _pts(X), _pts(Y)
    n, m = len(X), len(Y)
    C = np.zeros((n + m, n + m), dtype=np.float64)
    if n and m:
        C[:n, :m] = np.maximum(np.abs(X[:, None, 0] - Y[None, :, 0]), np.abs(X[:, None, 1] - Y[None, :, 1]))
    if n:
        C[:n, m:] = (np.abs(X[:, 1] - X[:, 0]) * 0.5)[:, None]
    if m:
        C[n:, :m] = (np.abs(Y[:, 1] - Y[:, 0]) * 0.5)[None, :]
    return C


def has_perfect_matching(C, t):
    N = len(C)
    if N == 0:
        return True
    match = maximum_bipartite_matching(csr_matrix(C <= t), perm_type="column")
    return bool((match >= 0).all())


def bottleneck(X, Y, upper=None):
    """d_B: the least entry t of the cost matrix for which the entries <= t hold a perfect matching (binary search over the sorted
    distinct costs); +0.0 for two empty diagrams.  The search starts at the largest row or column minimum (every row and every column
    takes some entry).  upper: a value the caller knows a perfect matching for (checked here with scipy) -- it only shortens the search."""
    C = cost_matrix(X, Y)
    if len(C) == 0:
        return np.float64(0.0)
    vals = np.unique(C)
    lo, hi = 0, len(vals) - 1                      # (the largest cost always admits one)
    lo = int(np.searchsorted(vals, max(C.min(1).max(), C.min(0).max())))
    if upper is not None:
        assert has_perfect_matching(C, upper)
        hi = int(np.searchsorted(vals, upper, side="right")) - 1
    while lo < hi:
        mid = (lo + hi) // 2
        if has_perfect_matching(C, vals[mid]):
            hi = mid
        else:
            lo = mid + 1
    return np.float64(vals[lo])


def pairs_of(assign_x, assign_y):
    """The pairs (i, j) that name a point, from the two maps: (i, j), (i, -1) and (-1, j)."""
    out = [(i, int(j)) for i, j in enumerate(assign_x)]
    out += [(-1, j) for j, i in enumerate(assign_y) if i < 0]
    return out


def pair_cost(X, Y, i, j):
    X, Y = _pts(X), _pts(Y)
    if i >= 0 and j >= 0:
        return np.maximum(np.abs(X[i, 0] - Y[j, 0]), np.abs(X[i, 1] - Y[j, 1]))
    if i >= 0:
        return np.abs(X[i, 1] - X[i, 0]) * 0.5
    return np.abs(Y[j, 1] - Y[j, 0]) * 0.5


def check_matching(X, Y, assign_x, assign_y):
    """The two maps are inverse to each other and in range; -> the largest cost of the matching they describe (+0.0 when empty)."""
    n, m = len(_pts(X)), len(_pts(Y))
    ax, ay = np.asarray(assign_x), np.asarray(assign_y)
    assert ax.shape == (n,) and ay.shape == (m,)
    assert ((ax >= -1) & (ax < max(m, 1))).all() and ((ay >= -1) & (ay < max(n, 1))).all()
    on = np.flatnonzero(ax >= 0)
    assert (ay[ax[on]] == on).all() and int((ay >= 0).sum()) == len(on)
    worst = np.float64(0.0)
    for i, j in pairs_of(ax, ay):
        worst = np.maximum(worst, pair_cost(X, Y, i, j))
    return worst


def arg_of(X, Y, assign_x, assign_y):
    """(i, j) of the header's rule for the given matching: among the pairs whose cost equals the matching's largest, the lowest
    predicted index (a point sent to the diagonal under its own index), else the pair (-1, j) of the lowest j; (-1, -1) without points."""
    pairs = pairs_of(assign_x, assign_y)
    if not pairs:
        return (-1, -1)
    worst = check_matching(X, Y, assign_x, assign_y)
    hit = [(i, j) for i, j in pairs if pair_cost(X, Y, i, j) == worst]
    real = [q for q in hit if q[0] >= 0]
    return min(real) if real else min(hit, key=lambda q: q[1])


def gradients(X, Y, arg):
    """(gradX [n, 2], gradY [m, 2]) of the header's rule for the attaining pair `arg`."""
    X, Y = _pts(X), _pts(Y)
    gx, gy = np.zeros_like(X), np.zeros_like(Y)
    i, j = int(arg[0]), int(arg[1])
    if i >= 0 and j >= 0:
        e = X[i] - Y[j]
        k = 0 if np.abs(e[0]) >= np.abs(e[1]) else 1
        gx[i, k] = np.sign(e[k])
        gy[j, k] = -np.sign(e[k])
    elif i >= 0:
        gx[i] = np.array([-0.5, 0.5]) * np.sign(X[i, 1] - X[i, 0])
    elif j >= 0:
        gy[j] = np.array([-0.5, 0.5]) * np.sign(Y[j, 1] - Y[j, 0])
    return gx + 0.0, gy + 0.0                      # (-0.0 -> +0.0)


def brute_force(X, Y):
    """min over all permutations of the largest cost (N <= 7 or so)."""
    from itertools import permutations
    C = cost_matrix(X, Y)
    N = len(C)
    if N == 0:
        return np.float64(0.0)
    rows = np.arange(N)
    return np.float64(min(C[rows, list(p)].max() for p in permutations(range(N))))


def pair(rs, n, m, style="random"):
    """The clouds of tests/test_gpu_w2_large.py: continuous coordinates with a few predicted points below the diagonal, or a coarse grid
    (coordinates k / 5: many tied costs)."""
    if style == "grid":
        return rs.randint(0, 6, size=(n, 2)) / 5.0, rs.randint(0, 6, size=(m, 2)) / 5.0
    b0 = rs.rand(n)
    X = np.stack([b0, b0 + rs.uniform(-0.1, 0.6, size=n)], 1)
    b1 = rs.rand(m)
    Y = np.stack([b1, b1 + rs.uniform(0.0, 0.7, size=m)], 1)
    return X.astype(np.float64), Y.astype(np.float64)

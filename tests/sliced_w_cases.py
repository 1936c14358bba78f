"""Shared by tests/test_gpu_sliced_w.py and tests/test_cpu_sliced_w_host.py: a numpy restatement of the sliced Wasserstein loss and of
the one sequence of roundings of its gradient (include/tlcgnn.h, "The sliced Wasserstein diagram loss"), and the generators of the
test problems.  Nothing here touches a device."""
import numpy as np

WAVE_NMAX, LDS_NMAX, MAX_DIRS = 64, 2048, 128          # TLC_SW_* (tests/test_cpu_sliced_w_host.py checks them against the header)

EXACT_DIRS = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0], [-1.0, 2.0]])
EXACT_SCALE = 0.25


def lists(X, Y, l0, l1):
    """V1, V2 of one direction (each n + m values, in listing order)"""
    cx = np.abs(X[:, 0] + X[:, 1]) * 0.5
    cy = np.abs(Y[:, 0] + Y[:, 1]) * 0.5
    V1 = np.concatenate([l0 * X[:, 0] + l1 * X[:, 1], (l0 + l1) * cy])
    V2 = np.concatenate([l0 * Y[:, 0] + l1 * Y[:, 1], (l0 + l1) * cx])
    return V1, V2


def restate(X, Y, dirs, scale):
    """-> (loss, gradX [n, 2], gradY [m, 2]): stable argsort (numpy compares with <, so -0.0 ties with +0.0), the sign scatter, and the
    header's accumulation order -- per direction ascending, first the projection term, then the diagonal term.  The rank sum is
    numpy's pairwise sum: the loss is compared within a bound, the gradients bit for bit."""
    X = np.asarray(X, dtype=np.float64).reshape(-1, 2)
    Y = np.asarray(Y, dtype=np.float64).reshape(-1, 2)
    n, m = len(X), len(Y)
    gx, gy = np.zeros((n, 2)), np.zeros((m, 2))
    sig, tau = np.sign(X[:, 0] + X[:, 1]), np.sign(Y[:, 0] + Y[:, 1])
    loss = 0.0
    for l0, l1 in np.asarray(dirs, dtype=np.float64).tolist():
        V1, V2 = lists(X, Y, l0, l1)
        o1, o2 = np.argsort(V1, kind="stable"), np.argsort(V2, kind="stable")
        d = V1[o1] - V2[o2]
        s = np.sign(d)
        loss += scale * float(np.sum(np.abs(d)))
        sA, sB = np.empty(n + m), np.empty(n + m)
        sA[o1] = s
        sB[o2] = s
        u = scale * ((l0 + l1) * 0.5)
        for c, t in ((0, scale * l0), (1, scale * l1)):
            gx[:, c] += sA[:n] * t
            gx[:, c] -= sB[m:] * sig * u
            gy[:, c] -= sB[:m] * t
            gy[:, c] += sA[n:] * tau * u
    return loss, gx, gy


def assert_tie_free(X, Y, dirs):
    """for every direction: the keys of V1 are distinct, the keys of V2 are distinct, and no rank has V1_(k) == V2_(k)"""
    for l0, l1 in np.asarray(dirs, dtype=np.float64).tolist():
        V1, V2 = lists(X, Y, l0, l1)
        s1, s2 = np.sort(V1), np.sort(V2)
        assert len(np.unique(V1)) == len(V1), "equal keys in V1"
        assert len(np.unique(V2)) == len(V2), "equal keys in V2"
        assert not np.any(s1 == s2), "a rank with equal keys"


def tie_free(rs, n, m, dirs):
    """random diagrams (birth in [0, 1), death above it) of n and m points without a tie in any of `dirs` -- asserted here"""
    def dgm(k):
        b = rs.random_sample(k)
        return np.stack([b, b + rs.random_sample(k) + 1e-3], 1)
    X, Y = dgm(n), dgm(m)
    assert_tie_free(X, Y, dirs)
    return X, Y


def even_grid(rs, n, m, span=40):
    """small even integer coordinates (so |b + d| / 2 is an integer and every number of EXACT_DIRS / EXACT_SCALE is exact in fp64)"""
    X = 2.0 * rs.randint(-span, span + 1, size=(n, 2))
    Y = 2.0 * rs.randint(-span, span + 1, size=(m, 2))
    return X, Y


def exact_loss(X, Y):
    """the loss of EXACT_DIRS / EXACT_SCALE in Python integers -> the float it must equal"""
    xi = [(int(b), int(d)) for b, d in X.tolist()]
    yi = [(int(b), int(d)) for b, d in Y.tolist()]
    total = 0
    for l0, l1 in ((1, 0), (0, 1), (1, 1), (-1, 2)):
        V1 = sorted([l0 * b + l1 * d for b, d in xi] + [(l0 + l1) * (abs(b + d) // 2) for b, d in yi])
        V2 = sorted([l0 * b + l1 * d for b, d in yi] + [(l0 + l1) * (abs(b + d) // 2) for b, d in xi])
        total += sum(abs(a - b) for a, b in zip(V1, V2))
    assert total % 1 == 0 and total < 2 ** 50
    return total / 4                                        # EXACT_SCALE = 1/4: exact


def tied(rs, n, m):
    """integer-grid diagrams with many equal keys; points with b + d = 0 and a -0.0 coordinate among them"""
    X = rs.randint(-2, 3, size=(n, 2)).astype(np.float64)
    Y = rs.randint(-2, 3, size=(m, 2)).astype(np.float64)
    for P in (X, Y):
        if len(P) > 0:
            P[0] = (1.0, -1.0)                              # b + d == 0: sigma = 0
        if len(P) > 1:
            P[1] = (-0.0, 0.0)
        if len(P) > 2:
            P[2] = (0.0, -0.0)
    return X, Y


def pack(problems):
    """[(X, Y)] -> xoff, X, yoff, Y packed"""
    xoff = np.concatenate([[0], np.cumsum([len(p[0]) for p in problems])]).astype(np.int64)
    yoff = np.concatenate([[0], np.cumsum([len(p[1]) for p in problems])]).astype(np.int64)
    X = np.concatenate([np.asarray(p[0], dtype=np.float64).reshape(-1, 2) for p in problems] + [np.zeros((0, 2))])
    Y = np.concatenate([np.asarray(p[1], dtype=np.float64).reshape(-1, 2) for p in problems] + [np.zeros((0, 2))])
    return xoff, X, yoff, Y


def class_sizes():
    """(n, m) with n + m at every edge of the three classes, n != m; one with n = 0, one with m = 0"""
    L = LDS_NMAX
    return [(1, 0), (0, 2), (2, 0), (40, 23), (23, 41), (30, 35), (L // 2 - 10, L // 2 + 9), (L // 2 + 7, L // 2 - 7), (L // 2 - 3, L // 2 + 4),
            (3 * L // 2 + 11, 3 * L // 2 - 20)]

"""Shared by tests/test_gpu_landscape.py and tests/test_cpu_landscape_host.py: a numpy restatement of the persistence landscape and of
its gradient as include/tlcgnn.h defines them, and the case builders.  numpy's float64 subtraction and comparison are the device's, so
everything here is compared with ==."""
import numpy as np


def tents(pts, ts):
    """v[i, j] = min(t_j - birth_i, death_i - t_j) with min(a, b) = a < b ? a : b"""
    pts, ts = np.asarray(pts, dtype=np.float64).reshape(-1, 2), np.asarray(ts, dtype=np.float64)
    up, down = ts[None, :] - pts[:, :1], pts[:, 1:] - ts[None, :]
    return np.where(up < down, up, down)


def restate(pts, ts, K):
    """-> (out float64[K, T], winner int32[K, T], status): the present points (v > 0) of every sample by a stable argsort of -v over
    the ascending indices, i.e. (v descending, i ascending); absent cells +0.0 / -1; a NaN / Inf coordinate: NaN / -1 / status 3."""
    pts, ts = np.asarray(pts, dtype=np.float64).reshape(-1, 2), np.asarray(ts, dtype=np.float64)
    T = len(ts)
    out, win = np.zeros((K, T)), np.full((K, T), -1, dtype=np.int32)
    if not np.isfinite(pts).all():
        return np.full((K, T), np.nan), win, 3
    if len(pts) == 0:
        return out, win, 0
    v = tents(pts, ts)
    key = np.where(v > 0, -v, np.inf)                          # absent points behind every present one
    order = np.argsort(key, axis=0, kind="stable")[:K]         # [min(K, n), T]
    top = np.take_along_axis(v, order, 0)
    there = top > 0
    out[:len(order)][there] = top[there]
    win[:len(order)][there] = order[there]
    return out, win, 0


def brute(pts, ts, K):
    """the same by sorting every sample's list of (value, index) pairs in Python"""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 2)
    out, win = np.zeros((K, len(ts))), np.full((K, len(ts)), -1, dtype=np.int32)
    for j, t in enumerate(ts):
        cand = []
        for i, (b, d) in enumerate(pts):
            up, down = t - b, d - t
            v = up if up < down else down
            if v > 0:
                cand.append((v, i))
        cand.sort(key=lambda c: (-c[0], c[1]))
        for k, (v, i) in enumerate(cand[:K]):
            out[k, j], win[k, j] = v, i
    return out, win


def restate_vjp(pts, ts, winner, gout):
    """-> float64[n, 2]: the literal ordered loop.  Cell (k, j) with winner i adds -g to the birth of i when t - b <= d - t, else +g to
    its death (the other coordinate's contribution is 0: a sum that starts at +0.0 is never -0.0, so adding it changes no bit)."""
    pts, ts = np.asarray(pts, dtype=np.float64).reshape(-1, 2), np.asarray(ts, dtype=np.float64)
    g = np.zeros_like(pts)
    K, T = winner.shape
    for k in range(K):
        for j in range(T):
            i = int(winner[k, j])
            if i < 0:
                continue
            b, d, t = pts[i, 0], pts[i, 1], ts[j]
            if t - b <= d - t:
                g[i, 0] += -gout[k, j]
            else:
                g[i, 1] += gout[k, j]
    return g


def pack(dgms):
    """-> (offs int64[B + 1], pts float64[sum n, 2])"""
    offs = np.concatenate([[0], np.cumsum([len(d) for d in dgms])]).astype(np.int64)
    pts = np.concatenate([np.asarray(d, dtype=np.float64).reshape(-1, 2) for d in dgms] + [np.zeros((0, 2))])
    return offs, np.ascontiguousarray(pts)


def random_diagram(rs, n):
    """births in [0, 1), persistences in [-0.05, 0.6): about one point in thirteen is never present"""
    b = rs.random_sample(n)
    return np.stack([b, b + rs.random_sample(n) * 0.65 - 0.05], 1)


def class_sizes(wave_nmax, lds_nmax):
    """the diagram sizes of the class batch: both sides of both cuts, and three slices with a last slice of one point"""
    return (0, 1, 2, wave_nmax - 1, wave_nmax, wave_nmax + 1, lds_nmax - 1, lds_nmax, lds_nmax + 1, 2 * lds_nmax + 1)


def grid(T):
    """T samples across the diagrams of random_diagram, none of them special"""
    return np.linspace(-0.1, 1.7, T) if T > 1 else np.array([0.5])


def integer_diagram(rs, n, hi=8):
    """integer coordinates in [0, hi): duplicates, death == birth, death < birth, and on an integer grid samples on peaks, births and
    deaths; the first rows are the named ties, with -0.0 as a coordinate"""
    named = np.array([[1.0, 3.0], [1.0, 3.0], [-0.0, 2.0], [0.0, 2.0], [-2.0, -0.0], [2.0, 2.0], [3.0, 1.0], [1.0, 3.0]])
    d = np.concatenate([named, rs.randint(0, hi, size=(max(n - len(named), 0), 2)).astype(np.float64)])[:n]
    return d


def integer_grid(hi=8):
    """every integer and half-integer from -3 to hi, and -0.0 next to 0.0"""
    return np.concatenate([np.arange(-6, 2 * hi + 1) * 0.5, [-0.0]])


def nested(N):
    """the intervals (i, 2N - i), i = 0 .. N-1: at an integer sample t the k-th value is min(t, 2N - t) - k, won by point k"""
    i = np.arange(N, dtype=np.float64)
    return np.stack([i, 2.0 * N - i], 1)


def nested_closed_form(N, K):
    t = np.arange(2 * N + 1, dtype=np.float64)
    peak = np.minimum(t, 2.0 * N - t)
    out, win = np.zeros((K, len(t))), np.full((K, len(t)), -1, dtype=np.int32)
    for k in range(min(K, N)):
        v = peak - k
        out[k], win[k] = np.where(v > 0, v, 0.0), np.where(v > 0, k, -1)
    return t, out, win


GAP = 1e-3                                                     # a thousand of gradcheck's steps of 1e-6


def kink_free(pts_list, ts):
    """every pair of tent values at every sample, every |(t - b) - (d - t)| and every value against 0 further apart than GAP"""
    for pts in pts_list:
        v = tents(pts, ts)
        if np.abs(v).min() <= GAP:
            return False
        if np.abs((ts[None, :] - pts[:, :1]) - (pts[:, 1:] - ts[None, :])).min() <= GAP:
            return False
        for j in range(v.shape[1]):
            col = np.sort(v[:, j])
            if len(col) > 1 and np.diff(col).min() <= GAP:
                return False
    return True


def gradcheck_input(seed=5, sizes=(4, 3), T=4, draws=100):
    """-> (diagrams, ts, draws used): built by rejection, so that no finite difference of gradcheck crosses a kink"""
    rs = np.random.RandomState(seed)
    for draw in range(1, draws + 1):
        dgms = [random_diagram(rs, n) for n in sizes]
        ts = np.sort(rs.random_sample(T)) * 1.2
        if kink_free(dgms, ts):
            return dgms, ts, draw
    raise AssertionError("no kink-free input within %d draws for seed %d" % (draws, seed))

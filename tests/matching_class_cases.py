"""The problems of tests/test_gpu_w2_classes.py and tests/test_gpu_bottleneck_classes.py: every compile-time variant of the two LDS
matching solvers (csrc/w2_match.hip, csrc/bottleneck.hip) at its own capacity and the rows beside it, tied and degenerate clouds with
closed answers, and batches larger than the grid with hand-placed pairs of problems that share a wavefront.  Pure numpy, no GPU:
tests/test_cpu_matching_class_cases.py checks the lists, the builders and the closed forms against oracle/w2_ref.py.

The dispatch rule the lists are made for.  Both solvers have four wavefront variants, CPL = 1 / 2 / 4 / 8 columns per lane for at most
64 / 128 / 256 / 512 rows, and a 512-thread workgroup variant for 513 .. 4 096 rows; a row is a predicted point (training form of
w2_match) or a point of either diagram (evaluation form, bottleneck).  w2_match picks the wavefront variant from the caller's max_points;
bottleneck from the largest problem of the batch that has at most 512 rows."""
import numpy as np

CAPACITIES = (64, 128, 256, 512)                                     # rows of the wavefront variants CPL = 1, 2, 4, 8
GRID = 16384                                                         # the wavefront kernels' grid cap: problems b and b + GRID share a wavefront
SIZES = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513)  # the matrix dimension N: every cut c as c - 1, c, c + 1
THROUGH_SIZES = (1, 63, 64, 128, 256)                                # solved again by every larger variant
TIE_SIZES = (64, 65, 128, 129, 256, 257, 512, 513, 600)              # grid style; no more: a tied workgroup problem takes up to N^2 steps
CLOSED_SIZES = (64, 128, 129, 512, 513)
BN_CLASSES = {64: (1, 2, 63, 64), 128: (65, 127, 128), 256: (129, 255, 256), 512: (257, 511, 512)}
BN_SHARED = (63, 64)                                                 # solved again inside each larger batch
PLACED = (3, 50, 101, 202, 303, 404)                                 # first positions of the hand-placed pairs; the second is + GRID
BN_PLACED = (7, 60, 130, 200)


def capacity(N):
    """rows of the variant a problem of N rows belongs to; None: the workgroup"""
    for c in CAPACITIES:
        if N <= c:
            return c
    return None


def targets(N):
    return sorted({0, N // 3, N // 2, N})


def pair(rs, n, m, style="random"):
    """the clouds of tests/test_gpu_w2_large.py and tests/bottleneck_cases.py"""
    if style == "grid":                                              # coordinates on a coarse grid: many tied costs
        return rs.randint(0, 6, size=(n, 2)) / 5.0, rs.randint(0, 6, size=(m, 2)) / 5.0
    b0 = rs.rand(n)
    X = np.stack([b0, b0 + rs.uniform(-0.1, 0.6, size=n)], 1)        # a few predicted points BELOW the diagonal
    b1 = rs.rand(m)
    Y = np.stack([b1, b1 + rs.uniform(0.0, 0.7, size=m)], 1)
    return X.astype(np.float64), Y.astype(np.float64)


def form_pair(rs, N, m, infer, style="random"):
    """matrix dimension N: the training form has n = N predicted points, the evaluation form n = N - m"""
    return pair(rs, N - m if infer else N, m, style)


def _seed(*parts):
    s = 0
    for p in parts:
        s = s * 1009 + int(p)
    return s % (2 ** 31)


def class_batch(N, infer, order, style="random"):
    """one batch for the dimension N: m in {0, N/3, N/2, N}, then two fillers of 3 and of 0 rows -> list of (X, Y)"""
    rs = np.random.RandomState(_seed(N, infer, order, style == "grid"))
    out = [form_pair(rs, N, m, infer, style) for m in targets(N)]
    out.append(form_pair(rs, 3, 1, infer, style))
    out.append(form_pair(rs, 0, 0, infer, style))
    return out


def filler_600(infer):
    return form_pair(np.random.RandomState(600 + int(infer)), 600, 250, infer)


def small_hint_batch():
    """a 65-row problem between two of 20 rows (training form: n rows; evaluation form: n + m rows)"""
    rs = np.random.RandomState(65)
    return {False: [pair(rs, 20, 7), pair(rs, 65, 30), pair(rs, 20, 20)], True: [pair(rs, 13, 7), pair(rs, 35, 30), pair(rs, 10, 10)]}


# ---- the degenerate families with closed answers --------------------------------------------------------------------------------------
def permuted(rs, n):
    """n distinct points above the diagonal and the same points in another order -> (X, Y, assign) with Y[assign[i]] = X[i]"""
    b = rs.rand(n)
    X = np.stack([b, b + rs.uniform(0.05, 0.7, size=n)], 1)
    perm = rs.permutation(n)
    assign = np.empty(n, dtype=np.int64)
    assign[perm] = np.arange(n)
    return X, X[perm].copy(), assign


def nearer_to_its_copy_than_to_the_diagonal(X):
    """(trivially: the copy costs 0 and a point above the diagonal pays its half persistence > 0 there)"""
    return bool(((X[:, 1] - X[:, 0]) * 0.5 > 0.0).all())


REPEATED_X, REPEATED_Y = (0.2, 0.9), (0.3, 0.7)


def repeated(n, m):
    return np.tile(np.array([REPEATED_X]), (n, 1)).reshape(n, 2), np.tile(np.array([REPEATED_Y]), (m, 1)).reshape(m, 2)


def repeated_loss(n, m, order, infer):
    """every assignment costs the same in the training form (m points on targets, n - m on the diagonal); in the evaluation form a
    matched pair (0.2 ^ p) beats the two sent to the diagonal (0.35 ^ p + 0.2 ^ p), so min(n, m) pairs are matched"""
    x, y = np.array(REPEATED_X), np.array(REPEATED_Y)
    dxy = np.abs(x - y).max()
    dxd = abs((x[1] - x[0]) * 0.5)
    dyd = abs((y[1] - y[0]) * 0.5)
    k = min(n, m) if infer else m
    tot = k * dxy ** order + (n - k) * dxd ** order + ((m - k) * dyd ** order if infer else 0.0)
    return float(tot ** (1.0 / order))


def on_the_diagonal(rs, n, m):
    """predicted points with birth = death (every diagonal cost 0, every diagonal column's minimiser the same row), random targets"""
    a = rs.rand(n)
    return np.stack([a, a], 1), pair(rs, 0, m)[1]


def on_the_diagonal_eval_loss(Y, order):
    """evaluation form: a point (a, a) is at least (d - b) / 2 away from the target (b, d), what the target pays on the diagonal, and
    pays nothing there itself: the optimum is the total persistence of the targets"""
    d = np.abs((Y[:, 1] - Y[:, 0]) * 0.5)
    return float((d ** order).sum() ** (1.0 / order)) if len(Y) else 0.0


# ---- no output left unwritten ----------------------------------------------------------------------------------------------------------
def unwritten_batch(hint, infer):
    """-> (problems, status expected, max_points).  hint 64 .. 512: one wavefront variant; 600: the 512 batch with a 600-row problem for
    the workgroup and a 4 097-row one above the cap, max_points 4 097."""
    H = min(hint, 512)
    rs = np.random.RandomState(_seed(hint, infer, 4))
    problems, status = [], []

    def add(p, s):
        problems.append(p); status.append(s)
    add(form_pair(rs, H, H // 3, infer), 0)                          # fills the variant
    add(form_pair(rs, H // 2, 0, infer), 0)                          # m = 0
    add(pair(rs, H // 2, H // 2) if not infer else pair(rs, H // 4, H // 4), 0)      # n = m
    add(pair(rs, 0, 0), 0)
    add(pair(rs, 5, 9), 0 if infer else 1)                           # n < m: no training form
    bad = pair(rs, 12, 10)
    bad[0][5, 1] = np.nan
    add(bad, 3)
    bad = pair(rs, 12, 10)
    bad[1][9, 0] = np.nan
    add(bad, 3)
    if hint <= 512:
        add(form_pair(rs, H + 1, 3, infer), 2)                       # above the hint
        top = hint
    else:
        add(form_pair(rs, 600, 250, infer), 0)
        add(form_pair(rs, 4097, 1, infer), 2)
        top = 4097
    if infer:
        add(pair(rs, 0, 7), 0)
        add(pair(rs, 7, 0), 0)
    return problems, status, top


# ---- a batch larger than the grid --------------------------------------------------------------------------------------------------------
def beyond_the_grid(cap, extra, infer):
    """GRID + extra problems, most of at most 12 rows, every fifth on the grid; the pairs of `placed_pairs` at PLACED[k], PLACED[k] + GRID.
    -> (problems, tied: per problem whether its costs tie, status expected, the hand-placed indices)"""
    assert extra > max(PLACED)
    rs = np.random.RandomState(_seed(cap, extra, infer, 5))
    B = GRID + extra
    problems, tied = [], []
    for k in range(B):
        N = int(rs.randint(0, 13))
        m = int(rs.randint(0, N + 1))
        problems.append(form_pair(rs, N, m, infer, "grid" if k % 5 == 0 else "random"))
        tied.append(k % 5 == 0)
    status = [0] * B
    full = lambda style="random": form_pair(rs, cap, cap // 3, infer, style)
    good = lambda: form_pair(rs, (5 * cap) // 8, cap // 4, infer)
    nan = pair(rs, 12, 10)
    nan[0][3, 0] = np.nan
    pairs = [((full(), False, 0), (form_pair(rs, 3, 1, infer), False, 0)),
             ((form_pair(rs, 3, 1, infer), False, 0), (full(), False, 0)),
             ((nan, False, 3), (good(), False, 0)),
             ((pair(rs, 5, 9), False, 0 if infer else 1), (good(), False, 0)),
             ((pair(rs, 0, 0), False, 0), (good(), False, 0)),
             ((full("grid"), True, 0), (full(), False, 0))]
    placed = []
    for b, two in zip(PLACED, pairs):
        for at, (p, t, s) in zip((b, b + GRID), two):
            problems[at], tied[at], status[at] = p, t, s
            placed.append(at)
    return problems, tied, status, placed


def bn_beyond_the_grid(extra=256):
    """bottleneck: GRID + extra problems of at most 40 points, and pairs at BN_PLACED[k], BN_PLACED[k] + GRID with a 128-row problem in
    each half, so that CPL = 2 runs whole and split -> (problems, the hand-placed indices)"""
    assert extra > max(BN_PLACED)
    rs = np.random.RandomState(_seed(extra, 6))
    problems = []
    for k in range(GRID + extra):
        N = int(rs.randint(0, 41))
        m = int(rs.randint(0, N + 1))
        problems.append(pair(rs, N - m, m, "grid" if k % 5 == 0 else "random"))
    pairs = [(pair(rs, 70, 58), pair(rs, 2, 1)), (pair(rs, 1, 2), pair(rs, 64, 64)), (pair(rs, 50, 50, "grid"), pair(rs, 128, 0)),
             (pair(rs, 0, 0), pair(rs, 40, 88))]
    placed = []
    for b, two in zip(BN_PLACED, pairs):
        for at, p in zip((b, b + GRID), two):
            problems[at] = p
            placed.append(at)
    return problems, placed


# ---- bottleneck: a batch per wavefront variant ---------------------------------------------------------------------------------------------
def bn_shared(style):
    """the problems of 63 and 64 rows that every variant solves"""
    rs = np.random.RandomState(_seed(63, style == "grid"))
    return [pair(rs, N - m, m, style) for N in BN_SHARED for m in targets(N)]


def bn_class_batch(cap, style):
    """-> (problems, index: (N, m) -> position, shared: positions of bn_shared's problems).  The largest problem has 64 CPL rows or
    fewer and more than the next smaller variant takes: wave_max falls in the variant."""
    rs = np.random.RandomState(_seed(cap, style == "grid", 7))
    problems, index = [], {}
    for N in BN_CLASSES[cap]:
        for m in targets(N):
            index[(N, m)] = len(problems)
            problems.append(pair(rs, N - m, m, style))
    if cap == 64:
        shared = [index[(N, m)] for N in BN_SHARED for m in targets(N)]
        for k, p in zip(shared, bn_shared(style)):
            problems[k] = p
    else:
        shared = list(range(len(problems), len(problems) + sum(len(targets(N)) for N in BN_SHARED)))
        problems += bn_shared(style)
    return problems, index, shared

"""No GPU: the case lists and builders of tests/matching_class_cases.py -- the sizes hold every cut's neighbours, the builders are
deterministic, the closed forms of the degenerate families equal scipy's optimum (oracle/w2_ref.py), and the hand-placed problems of
the batches larger than the grid sit exactly one grid apart."""
import numpy as np
import pytest

import matching_class_cases as mc
from oracle import w2_ref

CUTS = (64, 128, 256, 512)


def _same(a, b):
    assert len(a) == len(b)
    for (x0, y0), (x1, y1) in zip(a, b):
        assert np.array_equal(x0, x1, equal_nan=True) and np.array_equal(y0, y1, equal_nan=True)
        assert x0.shape == (len(x0), 2) and y0.shape == (len(y0), 2) and x0.dtype == np.float64 and y0.dtype == np.float64


def test_the_size_lists_hold_every_cut_and_its_neighbours():
    assert mc.CAPACITIES == CUTS
    for c in CUTS:
        assert {c - 1, c, c + 1} <= set(mc.SIZES), c
        assert {c, c + 1} <= set(mc.TIE_SIZES), c
        assert mc.capacity(c) == c and mc.capacity(c - 1) == c and mc.capacity(c + 1) == (2 * c if c < 512 else None)
        assert max(mc.BN_CLASSES[c]) == c and min(mc.BN_CLASSES[c]) == (c // 2 + 1 if c > 64 else 1)
    assert 1 in mc.SIZES and max(mc.SIZES) == 513 and max(mc.TIE_SIZES) == 600
    assert set(mc.THROUGH_SIZES) <= set(mc.SIZES) and set(mc.BN_SHARED) <= set(mc.BN_CLASSES[64])
    assert {64, 128, 129, 512, 513} == set(mc.CLOSED_SIZES)
    assert mc.targets(513) == [0, 171, 256, 513] and mc.targets(1) == [0, 1]


@pytest.mark.parametrize("infer", [False, True])
def test_the_class_batches(infer):
    for N in mc.SIZES + mc.TIE_SIZES:
        for style in ("random", "grid"):
            a = mc.class_batch(N, infer, 2, style)
            _same(a, mc.class_batch(N, infer, 2, style))
            rows = [len(x) + (len(y) if infer else 0) for x, y in a]
            assert rows == [N] * len(mc.targets(N)) + [3, 0]                       # the batch's largest problem is N: max_points = N
            assert [len(y) for _, y in a[:-2]] == mc.targets(N) and all(len(x) >= len(y) or infer for x, y in a)
    assert not np.array_equal(mc.class_batch(64, infer, 2)[0][0], mc.class_batch(64, infer, 1)[0][0])
    _same([mc.filler_600(infer)], [mc.filler_600(infer)])
    f = mc.filler_600(infer)
    assert len(f[0]) + (len(f[1]) if infer else 0) == 600
    three = mc.small_hint_batch()[infer]
    _same(three, mc.small_hint_batch()[infer])
    assert [len(x) + (len(y) if infer else 0) for x, y in three] == [20, 65, 20]


@pytest.mark.parametrize("infer", [False, True])
@pytest.mark.parametrize("hint", [64, 128, 256, 512, 600])
def test_the_batches_for_unwritten_outputs(hint, infer):
    problems, status, top = mc.unwritten_batch(hint, infer)
    again = mc.unwritten_batch(hint, infer)
    _same(problems, again[0])
    assert status == again[1] and len(status) == len(problems) and top == (hint if hint <= 512 else 4097)
    rows = [len(x) + (len(y) if infer else 0) for x, y in problems]
    H = min(hint, 512)
    assert rows[0] == H and mc.capacity(rows[0]) == H                              # a solved problem fills the variant
    assert len(problems[1][1]) == 0 and len(problems[2][0]) == len(problems[2][1]) > 0 and rows[3] == 0
    assert {1 - int(infer), 2, 3} <= set(status) | {0} and 2 in status and 3 in status
    for (x, y), s, r in zip(problems, status, rows):
        finite = bool(np.isfinite(x).all() and np.isfinite(y).all())
        above = r > (top if hint <= 512 else 4096)
        assert s == (3 if not finite and not above else 2 if above else 1 if (not infer and len(x) < len(y)) else 0)
    if hint > 512:
        assert 600 in rows
    if infer:
        assert (0, 7) in [(len(x), len(y)) for x, y in problems] and (7, 0) in [(len(x), len(y)) for x, y in problems]


@pytest.mark.parametrize("infer", [False, True])
@pytest.mark.parametrize("cap,extra", [(64, 4096), (512, 512)])
def test_the_batches_larger_than_the_grid(cap, extra, infer):
    problems, tied, status, placed = mc.beyond_the_grid(cap, extra, infer)
    again = mc.beyond_the_grid(cap, extra, infer)
    _same(problems, again[0])
    assert (tied, status, placed) == again[1:]
    assert len(problems) == len(tied) == len(status) == mc.GRID + extra and mc.GRID == 16384
    # the hand-placed pairs share a wavefront: exactly one grid apart
    assert len(placed) == 12 and all(b - a == 16384 for a, b in zip(placed[0::2], placed[1::2])) and max(placed) < len(problems)
    rows = lambda b: len(problems[b][0]) + (len(problems[b][1]) if infer else 0)
    assert max(rows(b) for b in range(len(problems))) == cap
    small = [rows(b) for b in range(len(problems)) if b not in placed]
    assert max(small) <= 12 and all(tied[b] == (b % 5 == 0) for b in range(len(problems)) if b not in placed)
    a = placed
    assert (rows(a[0]), rows(a[1])) == (cap, 3) and (rows(a[2]), rows(a[3])) == (3, cap)
    assert status[a[4]] == 3 and status[a[6]] == (0 if infer else 1) and rows(a[8]) == 0 and len(problems[a[8]][1]) == 0
    assert tied[a[10]] and rows(a[10]) == cap and not tied[a[11]] and rows(a[11]) == cap
    assert all(status[b] == 0 and rows(b) > 0 for b in a[1::2])
    assert sum(s != 0 for s in status) == (1 if infer else 2)


def test_the_bottleneck_batches():
    want = sum(len(mc.targets(N)) for N in mc.BN_SHARED)
    for style in ("random", "grid"):
        _same(mc.bn_shared(style), mc.bn_shared(style))
        for cap in mc.BN_CLASSES:
            problems, index, shared = mc.bn_class_batch(cap, style)
            _same(problems, mc.bn_class_batch(cap, style)[0])
            sizes = [len(x) + len(y) for x, y in problems]
            assert max(sizes) == cap and (cap == 64 or max(sizes) > cap // 2)
            assert sorted(index) == [(N, m) for N in mc.BN_CLASSES[cap] for m in mc.targets(N)]
            assert all((len(problems[b][0]) + len(problems[b][1]), len(problems[b][1])) == k for k, b in index.items())
            assert len(shared) == want
            _same([problems[b] for b in shared], mc.bn_shared(style))
    problems, placed = mc.bn_beyond_the_grid()
    _same(problems, mc.bn_beyond_the_grid()[0])
    sizes = [len(x) + len(y) for x, y in problems]
    assert len(problems) == 16384 + 256 and max(sizes[:16384]) == 128 and max(sizes[16384:]) == 128
    assert all(b - a == 16384 for a, b in zip(placed[0::2], placed[1::2]))
    assert max(s for b, s in enumerate(sizes) if b not in placed) <= 40


@pytest.mark.parametrize("order", [2, 1])
@pytest.mark.parametrize("N", [5, 64, 129])
def test_the_closed_forms_equal_scipy(N, order):
    """(N = 5 beside two of the sizes the GPU tests run: the closed forms do not depend on the size)"""
    # Y a permutation of X: cost 0, and the permutation is the matching
    X, Y, assign = mc.permuted(np.random.RandomState(N), N)
    assert np.array_equal(Y[assign], X) and sorted(assign.tolist()) == list(range(N)) and mc.nearer_to_its_copy_than_to_the_diagonal(X)
    assert len(np.unique(X, axis=0)) == N
    loss, wxy, wxd, a, cost = w2_ref.partial_matching(X, Y, order)
    assert (loss, wxy, wxd, cost) == (0.0, 0.0, 0.0, 0.0) and np.array_equal(a, assign)
    r = w2_ref.inference_matching(X, Y, order)
    assert r[:4] == (0.0, 0.0, 0.0, 0.0) and r[6] == 0.0 and np.array_equal(r[4], assign) and np.array_equal(r[5][assign], np.arange(N))
    # one point repeated
    for m in (0, N // 2, N):
        for infer in (False, True):
            X, Y = mc.repeated(N - m if infer else N, m)
            assert X.shape == (len(X), 2) and Y.shape == (m, 2)
            ref = (w2_ref.inference_matching if infer else w2_ref.partial_matching)(X, Y, order)[0]
            want = mc.repeated_loss(len(X), m, order, infer)
            assert abs(ref - want) <= 1e-12 * max(1.0, want), (N, m, infer, ref, want)
    # predicted points on the diagonal
    for m in mc.targets(N):
        rs = np.random.RandomState(N + m)
        X, Y = mc.on_the_diagonal(rs, N - m, m)
        assert (X[:, 0] == X[:, 1]).all() and (w2_ref.cost_matrix(X, Y, order)[:, m] == 0.0).all()
        r = w2_ref.inference_matching(X, Y, order)
        want = mc.on_the_diagonal_eval_loss(Y, order)
        assert abs(r[0] - want) <= 1e-12 * max(1.0, want) and r[2] == 0.0, (N, m, r[0], want)
        X, Y = mc.on_the_diagonal(rs, N, m)
        assert w2_ref.partial_matching(X, Y, order)[2] == 0.0

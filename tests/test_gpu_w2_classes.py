"""GPU: every compile-time variant of csrc/w2_match.hip's w2_solve<T, CPL, INFER> (tlc_w2_partial_matching, tlc_w2_inference_matching)
at its own capacity and the rows beside it, against scipy's assignment solver (oracle/w2_ref.py) through the checks of
tests/w2_checks.py.  Tolerances: those of tests/test_gpu_w2_large.py and tests/test_gpu_train.py -- 1e-9 relative on the cost against
scipy's optimum, 1e-12 on loss, parts and gradient against the restated expression and across variants, == on the closed forms that
are exactly zero, equal bits between a batch solved whole and in two calls.

The dispatch rule these tests rely on (dispatch_w2; tests/matching_class_cases.py): max_points <= 64 / 128 / 256 / 512 picks the
wavefront variant CPL = 1 / 2 / 4 / 8, one wavefront per problem, the problems by the grid's stride with the grid capped at 16 384;
above 512 the wavefront kernel CPL = 8 leaves the larger problems to a second launch, a 512-thread workgroup per problem of 513 ..
4 096 rows.  A problem above the variant's capacity gets status 2.  A row is a predicted point in the training form (N = n) and a
point of either diagram in the evaluation form (N = n + m).  Each size is solved in a batch of its own with max_points = N, so the
variant that runs is the one the size belongs to; the cuts are asserted from _lib, and a moved cut fails here instead of silently
testing another variant.

Ties are where the variants differ by design: among equal minima a wavefront takes the lowest lane (for CPL > 1 not the lowest column),
a workgroup the lowest column (w2_select).  No tied problem is larger than 600 rows: a workgroup needs up to N^2 steps of about 1.5 us
on tied input (the header of w2_match.hip)."""
import numpy as np
import pytest

import matching_class_cases as mc
import w2_checks as wc

pytestmark = pytest.mark.gpu

FORMS = [False, True]                                                 # infer: the training form, the evaluation form


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    from tlc_gnn_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    assert _lib.W2_LDS_NMAX == 4096 and mc.CAPACITIES == (64, 128, 256, 512) and mc.GRID == 16384
    return torch


_CACHE = {}


def _class_solved(torch, N, infer, order, style="random"):
    """the batch of the dimension N with max_points = N: solved once"""
    key = (N, infer, order, style)
    if key not in _CACHE:
        problems = mc.class_batch(N, infer, order, style)
        _CACHE[key] = (problems,) + wc.solve(torch, problems, infer, order, N)
    return _CACHE[key]


# ---- 1. every variant at its cuts ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [2, 1])
@pytest.mark.parametrize("infer", FORMS)
@pytest.mark.parametrize("N", mc.SIZES)
def test_every_variant_at_its_cuts(torch_cuda, N, infer, order):
    problems, xoff, yoff, h = _class_solved(torch_cuda, N, infer, order)
    assert h["status"].tolist() == [0] * len(problems), (N, h["status"])
    for b, p in enumerate(problems):
        wc.check_problem(torch_cuda, p, infer, order, h, xoff, yoff, b)


# ---- 2. one problem through every variant -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [2, 1])
@pytest.mark.parametrize("infer", FORMS)
@pytest.mark.parametrize("N", mc.THROUGH_SIZES)
def test_one_problem_through_every_variant(torch_cuda, N, infer, order):
    """the batch of part 1 again with max_points at every larger capacity, and once beside a 600-row problem (max_points 600: the
    wavefront kernel CPL = 8 solves it while the workgroup launch takes the 600 rows).  Order 2: the optimum is unique on continuous
    coordinates, so matching and gradient agree too; order 1: it is not (test_against_the_lds_kernels of tests/test_gpu_w2_large.py
    explains): two optimal matchings share the loss, not its parts, so only the loss is compared there."""
    torch = torch_cuda
    problems, xoff, yoff, base = _class_solved(torch, N, infer, order)
    B = len(problems)
    runs = [(hint, wc.solve(torch, problems, infer, order, hint)[2]) for hint in mc.CAPACITIES if hint > mc.capacity(N)]
    _, _, beside = wc.solve(torch, problems + [mc.filler_600(infer)], infer, order, 600)
    assert beside["status"].tolist() == [0] * (B + 1)
    runs.append((600, {k: v[:len(base[k])] for k, v in beside.items()}))
    assert len(runs) == 1 + sum(c > mc.capacity(N) for c in mc.CAPACITIES)
    close = lambda a, b: bool((np.abs(a - b) <= 1e-12 * np.maximum(1.0, np.abs(b))).all())
    for hint, h in runs:
        assert h["status"].tolist() == [0] * B, (hint, h["status"])
        print("N=%d order=%d max_points=%d: largest loss difference %.3g" % (N, order, hint, np.abs(h["loss"] - base["loss"]).max()))
        assert close(h["loss"], base["loss"]), hint
        if order == 2:
            for k in ("wxy", "wxd") + (("wyd",) if infer else ()):
                assert close(h[k], base[k]), (hint, k)
            assert np.array_equal(h["assign_x"], base["assign_x"]) and (not infer or np.array_equal(h["assign_y"], base["assign_y"])), hint
            assert np.abs(h["grad"] - base["grad"]).max() <= 1e-12, hint


@pytest.mark.parametrize("order", [2, 1])
@pytest.mark.parametrize("infer", FORMS)
def test_a_hint_that_is_too_small(torch_cuda, infer, order):
    """max_points = 64 for a 65-row problem between two of 20 rows: status 2 and w2_fail's outputs there, the neighbours solved"""
    problems = mc.small_hint_batch()[infer]
    xoff, yoff, h = wc.solve(torch_cuda, problems, infer, order, 64)
    assert h["status"].tolist() == [0, 2, 0]
    wc.check_refused(h, infer, xoff, yoff, 1, 2)
    for b in (0, 2):
        wc.check_problem(torch_cuda, problems[b], infer, order, h, xoff, yoff, b)


# ---- 3. ties in every variant, and the degenerate starts --------------------------------------------------------------------------------------
@pytest.mark.parametrize("infer", FORMS)
@pytest.mark.parametrize("N", mc.TIE_SIZES)
def test_ties_in_every_variant(torch_cuda, N, infer):
    """coordinates k / 5: many optimal matchings; the device's one is valid and its cost is scipy's optimum"""
    for order in (2, 1):
        problems, xoff, yoff, h = _class_solved(torch_cuda, N, infer, order, "grid")
        assert h["status"].tolist() == [0] * len(problems), (N, order, h["status"])
        for b, p in enumerate(problems):
            wc.check_problem(torch_cuda, p, infer, order, h, xoff, yoff, b, unique=False)


@pytest.mark.parametrize("infer", FORMS)
@pytest.mark.parametrize("N", mc.CLOSED_SIZES)
def test_target_a_permutation_of_the_prediction(torch_cuda, N, infer):
    """n = m = N (the evaluation form's matrix has 2 N rows; at 512 and 513 that is the workgroup): loss, wxy, wxd (wyd) exactly 0.0,
    a zero gradient, and at order 2 the permutation itself"""
    X, Y, assign = mc.permuted(np.random.RandomState(N), N)
    assert mc.nearer_to_its_copy_than_to_the_diagonal(X)
    for order in (2, 1):
        xoff, yoff, h = wc.solve(torch_cuda, [(X, Y)], infer, order, 2 * N if infer else N)
        wc.check_problem(torch_cuda, (X, Y), infer, order, h, xoff, yoff, 0, unique=False)
        assert h["loss"][0] == 0.0 and h["wxy"][0] == 0.0 and h["wxd"][0] == 0.0 and (not infer or h["wyd"][0] == 0.0), (order, h["loss"][0])
        assert (h["grad"] == 0.0).all()
        if order == 2:
            assert np.array_equal(h["assign_x"], assign)
            if infer:
                assert np.array_equal(h["assign_y"][assign], np.arange(N))


@pytest.mark.parametrize("infer", FORMS)
@pytest.mark.parametrize("N", mc.CLOSED_SIZES)
def test_one_point_repeated(torch_cuda, N, infer):
    """every cost between the two clouds is the same number: the matching is any valid one, the loss the closed form"""
    from oracle import w2_ref
    for order in (2, 1):
        ms = (0, N // 2, N)
        problems = [mc.repeated(N - m if infer else N, m) for m in ms]
        xoff, yoff, h = wc.solve(torch_cuda, problems, infer, order, N)
        for b, (p, m) in enumerate(zip(problems, ms)):
            wc.check_problem(torch_cuda, p, infer, order, h, xoff, yoff, b, unique=False)
            want = mc.repeated_loss(len(p[0]), m, order, infer)
            ref = (w2_ref.inference_matching if infer else w2_ref.partial_matching)(p[0], p[1], order)[0]
            print("one point repeated N=%d m=%d order=%d: device %.17g closed form %.17g scipy %.17g" % (N, m, order, h["loss"][b], want, ref))
            assert abs(ref - want) <= 1e-12 * max(1.0, want)
            assert abs(h["loss"][b] - want) <= 1e-12 * max(1.0, want), (N, m, order, h["loss"][b], want)


@pytest.mark.parametrize("infer", FORMS)
@pytest.mark.parametrize("N", mc.CLOSED_SIZES)
def test_predicted_points_on_the_diagonal(torch_cuda, N, infer):
    """birth = death: the diagonal costs every point nothing, and every diagonal column names row 0 in the column reduction.  Against
    scipy; wxd is exactly 0.0; in the evaluation form the loss is the targets' total persistence."""
    for order in (2, 1):
        rs = np.random.RandomState(7 * N + order)
        ms = mc.targets(N)
        problems = [mc.on_the_diagonal(rs, N - m if infer else N, m) for m in ms]
        xoff, yoff, h = wc.solve(torch_cuda, problems, infer, order, N)
        for b, p in enumerate(problems):
            if infer and len(p[1]) == 0:
                # against the empty diagram the loss itself is 0: the gradient's 0 / 0 is defined as 0 (w2_pair_grad)
                assert h["status"][b] == 0 and h["loss"][b] == 0.0 and h["wxy"][b] == 0.0 and h["wxd"][b] == 0.0 and h["wyd"][b] == 0.0
                assert (h["assign_x"][xoff[b]:xoff[b + 1]] == -1).all() and (h["grad"][xoff[b]:xoff[b + 1]] == 0.0).all()
                continue
            wc.check_problem(torch_cuda, p, infer, order, h, xoff, yoff, b, unique=False)
            assert h["wxd"][b] == 0.0, (N, b, h["wxd"][b])
            if infer:
                want = mc.on_the_diagonal_eval_loss(p[1], order)
                assert abs(h["loss"][b] - want) <= 1e-12 * max(1.0, want), (N, b, order, h["loss"][b], want)


# ---- 4. no output element left unwritten ------------------------------------------------------------------------------------------------------
def _raw_batch(torch, problems, infer):
    xoff, yoff, dxo, dX, dyo, dY = wc._pack(torch, [p[0] for p in problems], [p[1] for p in problems])
    return xoff, yoff, (dxo, dX, dyo, dY)


def _to_host(o):
    h = {k: v.cpu().numpy() for k, v in o.items()}
    for v in h.values():
        v.setflags(write=False)
    return h


@pytest.mark.parametrize("infer", FORMS)
@pytest.mark.parametrize("hint", [64, 128, 256, 512, 600])
def test_no_output_element_is_left_unwritten(torch_cuda, hint, infer):
    """the C entries on outputs pre-filled with -7.0 / -7 / 77 (the wrappers of ops pre-fill with exactly what w2_fail writes, which
    would hide an element the kernel forgot): one batch per variant of solved, empty and refused problems; 600: the CPL = 8 batch with a
    600-row problem for the workgroup launch and a 4 097-row one above the cap"""
    torch = torch_cuda
    problems, status, top = mc.unwritten_batch(hint, infer)
    xoff, yoff, dev = _raw_batch(torch, problems, infer)
    for order in (2, 1):
        o = wc._raw_outputs(torch, infer, len(problems), int(xoff[-1]), int(yoff[-1]))
        wc._raw_call(o, infer, *dev, 0, len(problems), order, top)
        torch.cuda.synchronize()
        h = _to_host(o)
        assert h["status"].tolist() == status, (hint, h["status"], status)
        for k, v in h.items():
            sentinel = wc.STATUS_SENTINEL if k == "status" else (wc.INT_SENTINEL if v.dtype == np.int32 else wc.DOUBLE_SENTINEL)
            left = np.flatnonzero((v == sentinel).reshape(len(v), -1).any(1))
            assert left.size == 0, "%s keeps the sentinel at %s (hint %d, order %d)" % (k, left[:8].tolist(), hint, order)
        for b, (p, s) in enumerate(zip(problems, status)):
            if s:
                wc.check_refused(h, infer, xoff, yoff, b, s)
            else:
                wc.check_problem(torch, p, infer, order, h, xoff, yoff, b)


# ---- 5. a batch larger than the grid ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("infer", FORMS)
@pytest.mark.parametrize("cap,extra", [(64, 4096), (512, 512)])
def test_a_batch_larger_than_the_grid(torch_cuda, cap, extra, infer):
    """16 384 + extra problems, max_points = cap: the wavefronts of the first `extra` blocks solve a second problem on the LDS a first
    one left behind -- a full one after a small one and the reverse, a good one after a refused, an empty and a tied one.  The batch
    whole equals, bit for bit, the batch in two calls on [0, 16 384) and [16 384, B), where every wavefront starts fresh; a sample and
    the hand-placed problems against scipy."""
    torch = torch_cuda
    problems, tied, status, placed = mc.beyond_the_grid(cap, extra, infer)
    B = len(problems)
    assert B == mc.GRID + extra and len(placed) == 2 * len(mc.PLACED)
    xoff, yoff, dev = _raw_batch(torch, problems, infer)
    nx, ny = int(xoff[-1]), int(yoff[-1])
    whole, split = wc._raw_outputs(torch, infer, B, nx, ny), wc._raw_outputs(torch, infer, B, nx, ny)
    wc._raw_call(whole, infer, *dev, 0, B, 2, cap)
    wc._raw_call(split, infer, *dev, 0, mc.GRID, 2, cap)
    wc._raw_call(split, infer, *dev, mc.GRID, extra, 2, cap)
    torch.cuda.synchronize()
    for k in whole:
        assert wc.same_bits(torch, whole[k], split[k]), k
    h = _to_host(whole)
    assert h["status"].tolist() == status
    rs = np.random.RandomState(cap)
    for b in sorted(set(rs.randint(0, B, size=200).tolist() + placed + [mc.GRID - 1, mc.GRID, B - 1])):
        if status[b]:
            wc.check_refused(h, infer, xoff, yoff, b, status[b])
        else:
            wc.check_problem(torch, problems[b], infer, 2, h, xoff, yoff, b, unique=not tied[b])

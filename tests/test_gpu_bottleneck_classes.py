"""GPU: the four wavefront variants of csrc/bottleneck.hip (tlc_bn_wave_kernel<CPL>, CPL = 1 / 2 / 4 / 8) each at its own capacity and
the rows beside it, against the numpy + scipy restatement of tests/bottleneck_cases.py through the checks of
tests/bottleneck_checks.py.  d_B is one entry of the cost matrix: every value is compared with ==, a batch solved whole and in two
calls with torch.equal.

The dispatch rule these tests rely on (the end of tlc_bottleneck_matching; tests/matching_class_cases.py): the problems of at most 512
rows (N = n + m) get one wavefront each, and the variant is picked from the largest of THEM in the batch -- wave_max <= 64 / 128 / 256
/ else: CPL = 1 / 2 / 4 / 8; the problems by the grid's stride with the grid capped at 16 384.  Problems of 513 .. 4 096 rows get a
512-thread workgroup each in a second launch.  So each variant has a batch of its own here, whose largest problem falls in it; the
cuts are asserted from _lib, and a moved cut fails here instead of silently testing another variant.  The selection rule names
columns, not lanes, so all variants give the same bits: the problems of 63 and 64 rows ride in every batch."""
import numpy as np
import pytest

import bottleneck_cases as cases
import matching_class_cases as mc
from bottleneck_checks import _check_witness, _pack, _raw_call, _raw_outputs, _solve

pytestmark = pytest.mark.gpu

CAPS = sorted(mc.BN_CLASSES)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    from tlc_gnn_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    assert _lib.BN_WAVE_NMAX == 512 and _lib.BN_NMAX == 4096 and tuple(CAPS) == mc.CAPACITIES and mc.GRID == 16384
    return torch


_CACHE = {}


def _solved(torch, cap, style):
    """the batch of one variant: solved once, the restatement computed once"""
    if (cap, style) not in _CACHE:
        problems, index, shared = mc.bn_class_batch(cap, style)
        sizes = [len(x) + len(y) for x, y in problems]
        assert max(sizes) == cap and (cap == 64 or max(sizes) > cap // 2)          # wave_max falls in this variant
        xoff, yoff, h = _solve(torch, problems)
        want = [cases.bottleneck(X, Y) for X, Y in problems]
        _CACHE[(cap, style)] = dict(problems=problems, index=index, shared=shared, xoff=xoff, yoff=yoff, h=h, want=want)
    return _CACHE[(cap, style)]


@pytest.mark.parametrize("cap", CAPS)
def test_values_and_witness_in_every_variant(torch_cuda, cap):
    s = _solved(torch_cuda, cap, "random")
    for b in list(s["index"].values()) + s["shared"]:
        _check_witness(*s["problems"][b], s["h"], s["xoff"], s["yoff"], b, s["want"][b])


@pytest.mark.parametrize("cap", CAPS)
def test_ties_in_every_variant(torch_cuda, cap):
    """coordinates k / 5: the value stays exact; the matching is one of many, valid and attaining the value"""
    s = _solved(torch_cuda, cap, "grid")
    h, xoff, yoff = s["h"], s["xoff"], s["yoff"]
    for b in sorted(set(s["index"].values()) | set(s["shared"])):
        X, Y = s["problems"][b]
        N = len(X) + len(Y)
        assert h["status"][b] == 0 and h["dist"][b] == s["want"][b] and not np.signbit(h["dist"][b]), (N, len(Y), h["dist"][b], s["want"][b])
        ax, ay = h["assign_x"][xoff[b]:xoff[b + 1]], h["assign_y"][yoff[b]:yoff[b + 1]]
        assert cases.check_matching(X, Y, ax, ay) == h["dist"][b]
        # the pair named is one of the matching's and attains the value
        i, j = h["arg"][b].tolist()
        assert (i, j) in cases.pairs_of(ax, ay) and cases.pair_cost(X, Y, i, j) == h["dist"][b]
        assert (i, j) == cases.arg_of(X, Y, ax, ay)


@pytest.mark.parametrize("style", ["random", "grid"])
def test_the_variants_give_the_same_bits(torch_cuda, style):
    """the problems of 63 and 64 rows, solved by CPL = 1 in their own batch and by CPL = 2, 4 and 8 in the others"""
    runs = [_solved(torch_cuda, cap, style) for cap in CAPS]
    base = runs[0]
    want = mc.bn_shared(style)
    for s in runs:
        assert len(s["shared"]) == len(want)
        for k, b in enumerate(s["shared"]):
            assert np.array_equal(s["problems"][b][0], want[k][0]) and np.array_equal(s["problems"][b][1], want[k][1])
            d0, d = base["h"]["dist"][base["shared"][k]:][:1], s["h"]["dist"][b:b + 1]
            assert np.array_equal(d0.view(np.int64), d.view(np.int64)), (k, d0, d)


def test_a_batch_larger_than_the_grid_on_two_columns_per_lane(torch_cuda):
    """16 384 + 256 problems of at most 40 points and, in each half, one of 128: CPL = 2, and the wavefronts of the first 256 blocks
    solve a second problem on the LDS a first one left behind.  Whole against the two halves alone, where every wavefront starts fresh."""
    torch = torch_cuda
    problems, placed = mc.bn_beyond_the_grid()
    B = len(problems)
    sizes = [len(x) + len(y) for x, y in problems]
    assert B == mc.GRID + 256 and max(sizes[:mc.GRID]) == 128 and max(sizes[mc.GRID:]) == 128
    xoff, yoff, (dxo, dX, dyo, dY) = _pack(torch, problems)
    nx, ny = int(xoff[-1]), int(yoff[-1])
    whole, split = _raw_outputs(torch, B, nx, ny), _raw_outputs(torch, B, nx, ny)
    _raw_call(whole, dxo, dX, dyo, dY, 0, B, 128)
    _raw_call(split, dxo, dX, dyo, dY, 0, mc.GRID, 128)
    _raw_call(split, dxo, dX, dyo, dY, mc.GRID, B - mc.GRID, 128)
    torch.cuda.synchronize()
    for k in whole:
        assert torch.equal(whole[k], split[k]), k
    assert int(whole["status"].max()) == 0 and float(whole["dist"].min()) >= 0.0
    d = whole["dist"].cpu().numpy()
    rs = np.random.RandomState(11)
    for b in rs.randint(0, B, size=100).tolist() + placed + [mc.GRID - 1, mc.GRID, B - 1]:
        assert d[b] == cases.bottleneck(*problems[b]), b

"""No GPU: the numpy restatement of tlc_dist_filtration (tests/dist_filt_cases.py) against the reference's recorded values
(tests/golden/dist_filt_ref.npz, made by make_golden_dist_filt.py from the imported reference), the tree rule on a hand-made tie, the
VJP restatement against central differences, and the host arithmetic of the workspace size."""
import ctypes as C
import os

import numpy as np
import pytest

import dist_filt_cases as dc

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_restatement_equals_the_reference_bit_for_bit():
    z = np.load(os.path.join(G, "dist_filt_ref.npz"))
    no, eo = z["node_offs"], z["edge_offs"]
    assert 50 <= len(no) - 1 and (no[1:] - no[:-1]).min() == 2 and (no[1:] - no[:-1]).max() == 200
    for g in range(len(no) - 1):
        n, e, w = int(no[g + 1] - no[g]), z["edges"][eo[g]:eo[g + 1]], z["w"][eo[g]:eo[g + 1]]
        r0, r1 = (int(v) for v in z["roots"][g])
        D = dc.all_sources(n, e, w)
        f, st, _ = dc.forward(n, e, w, r0, -1, dc.NORM_EPS, D)                  # data_utils_NC ricci_filtration.build_fv(norm=True)
        assert st == dc.ST_OK and np.array_equal(f, z["f_one"][no[g]:no[g + 1]]), g
        for name, flag in (("f_sum", 0), ("f_min", dc.DESC_MIN), ("f_max", dc.DESC_MAX)):     # riccidist2dgm filtration.build_fv
            f, st, _ = dc.forward(n, e, w, r0, r1, flag, D)
            assert st == z["st_two"][g], (g, name)
            if st == dc.ST_OK:
                assert np.array_equal(f, z[name][no[g]:no[g + 1]]), (g, name)
    assert (z["st_two"] == dc.ST_ZERO_RANGE).sum() >= 1                         # the graph that is its two roots


def test_tree_rule_on_a_hand_made_tie():
    """A square 0-1-3-2-0 with unit weights, root 0: node 3 has two equal paths and takes the LOWEST neighbour, 1; a heavier edge 0-3
    ties with both and still loses to id 1... unless it is the lowest id: then it wins."""
    e = np.array([[0, 1], [0, 2], [3, 2], [3, 1]], np.int32)
    w = np.ones(4)
    f, st, P = dc.forward(4, e, w, 0, -1, dc.NO_NORM)
    assert st == dc.ST_OK and f.tolist() == [0.0, 1.0, 1.0, 2.0] and P[0].tolist() == [-1, 0, 0, 1] and P[1].tolist() == [-1] * 4
    e2, w2 = np.concatenate([e, [[3, 0]]]).astype(np.int32), np.array([1.0, 1.0, 1.0, 1.0, 2.0])
    assert dc.forward(4, e2, w2, 0, -1, dc.NO_NORM)[2][0].tolist() == [-1, 0, 0, 0]
    # the gradient follows the convention: all of g[3] goes down the chain 3 -> 1 -> 0
    gw, st = dc.vjp(4, e, w, 0, -1, dc.NO_NORM, P, np.array([0.0, 0.0, 0.0, 1.0]))
    assert st == dc.ST_OK and gw.tolist() == [1.0, 0.0, 0.0, 1.0]
    # rounding absorbs a weight: R[2] == R[1], no neighbour is strictly closer with an exact sum -> -1
    e3, w3 = np.array([[0, 1], [1, 2]], np.int32), np.array([1.0, 1e-30])
    assert dc.forward(3, e3, w3, 0, -1, dc.NO_NORM)[2][0].tolist() == [-1, 0, -1]


@pytest.mark.parametrize("r1", [7, -1, 3])
def test_vjp_restatement_against_central_differences(r1):
    """Distinct random weights, 12 nodes, both roots (and equal roots), every descriptor and norm.  h = 1e-6: truncation h^2 |f'''| is
    below 1e-10, rounding 2^-52 |f| / h about 1e-9: the bound 1e-7 leaves both a factor of fifty."""
    rng = np.random.default_rng(5)
    n, r0 = 12, 3
    e = dc.random_connected(rng, n, 22)
    w, g = dc.generic_weights(rng, len(e)), rng.normal(size=n)
    for desc in (0, dc.DESC_MIN, dc.DESC_MAX):
        for nf in (0, dc.NORM_EPS, dc.NO_NORM):
            fl = desc | nf
            f, st, P = dc.forward(n, e, w, r0, r1, fl)
            gw, st = dc.vjp(n, e, w, r0, r1, fl, P, g)
            num = np.zeros(len(e))
            for k in range(len(e)):
                wp, wm = w.copy(), w.copy()
                wp[k] += 1e-6
                wm[k] -= 1e-6
                num[k] = (g @ dc.forward(n, e, wp, r0, r1, fl)[0] - g @ dc.forward(n, e, wm, r0, r1, fl)[0]) / 2e-6
            assert np.abs(num - gw).max() < 1e-7, (hex(fl), np.abs(num - gw).max())


def test_work_bytes_is_monotone_and_refuses():
    from tlc_gnn_amd import _lib, engine
    L = _lib.lib()
    for sym in ("tlc_dist_filtration_work_bytes", "tlc_dist_filtration_vjp_work_bytes", "tlc_dist_filtration", "tlc_dist_filtration_vjp"):
        assert sym in _lib.SYMBOLS and getattr(L, sym).argtypes, sym
    assert (_lib.DIST_WAVE_NMAX, _lib.DIST_WG_NMAX, _lib.DIST_WG_MMAX) == (64, 2048, 4096)
    for vjp in (False, True):
        last = 0
        for B, N, M in ((1, 1, 0), (1, 64, 63), (2, 100, 200), (10, 2048, 4096), (10, 2049, 4096), (10, 2049, 4097), (11, 2049, 4097),
                        (100, 20000, 50000), (41127, 1 << 20, 1 << 20)):
            b = engine.dist_filtration_work_bytes(B, N, M, vjp=vjp)
            assert b >= last and b % 256 == 0, (B, N, M)              # (arrays round up to 256 bytes: one more graph may cost nothing)
            last = b
        assert last > engine.dist_filtration_work_bytes(100, 20000, 50000, vjp=vjp) > engine.dist_filtration_work_bytes(2, 100, 200, vjp=vjp)
    # the whole-device class's state appears exactly when the batch can hold such a graph
    small, wide = engine.dist_filtration_work_bytes(4, 2048, 4096), engine.dist_filtration_work_bytes(4, 2049, 4096)
    assert wide - small > 2049 * 56 and engine.dist_filtration_work_bytes(4, 2048, 4097) - small > 2048 * 56
    need = C.c_int64(0)
    for fn in (L.tlc_dist_filtration_work_bytes, L.tlc_dist_filtration_vjp_work_bytes):
        assert fn(C.c_int64(-1), C.c_int64(0), C.c_int64(0), C.byref(need)) == 1
        assert fn(C.c_int64(1), C.c_int64(-1), C.c_int64(0), C.byref(need)) == 1
        assert fn(C.c_int64(1), C.c_int64(1), C.c_int64(0), None) == 1
        assert fn(C.c_int64(1), C.c_int64(1 << 30), C.c_int64(0), C.byref(need)) == 4       # TLC_ERR_UNSUPPORTED
    with pytest.raises(ValueError):
        engine.dist_filtration_flags(descriptor="mean")
    with pytest.raises(ValueError):
        engine.dist_filtration_flags(norm="l2")

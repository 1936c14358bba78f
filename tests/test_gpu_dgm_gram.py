"""GPU: Gram matrices of persistence diagram kernels and their gradient (csrc/dgm_gram.hip; engine.dgm_gram / dgm_gram_vjp;
ops.diagram_gram; autograd.diagram_gram / diagram_kernel_distance; topo.gram / kernel_distance_to; Teacher_Model kernel='pss').

Values and gradients are compared with the np.longdouble restatement of tests/dgm_gram_cases.py within the bound of DESIGN.md 6.17,
(C0 + L) 2^-53 S with the argument-rounding term folded in: C0 counts the roundings of one summand (the device library's exp within
1 ulp), L is the longest chain of additions of the documented order, S the sum of the absolute values of the reference's summands.
Everything the header promises about the order -- alone / in a batch, ALL / PAIRED / SYMMETRIC, least / full workspace, run to run --
is compared with == on the raw bits."""
import ctypes as C

import numpy as np
import pytest

import dgm_gram_cases as cases
from tlc_gnn_amd import _lib

pytestmark = pytest.mark.gpu
ALL, PAIRED, SYMMETRIC, MIRROR = _lib.DG_ALL, _lib.DG_PAIRED, _lib.DG_SYMMETRIC, _lib.DG_MIRROR
INVALID = 1


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _dev(torch, a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


class Side:
    """one packed batch of diagrams (and weights) on the device"""

    def __init__(self, torch, dgms, ws=None):
        self.dgms, self.ws = [np.asarray(d, dtype=np.float64).reshape(-1, 2) for d in dgms], ws
        self.offs, self.pts = cases.pack(self.dgms)
        self.B, self.rows = len(dgms), len(self.pts)
        self.max_points = int(np.diff(self.offs).max()) if self.B else 0
        self.d_offs, self.d_pts = _dev(torch, self.offs, torch.int64), _dev(torch, self.pts, torch.float64)
        self.w = None if ws is None else cases.pack_w(ws)
        self.d_w = None if ws is None else _dev(torch, self.w, torch.float64)

    def weights(self, i):
        return None if self.ws is None else self.ws[i]

    def ptrs(self):
        return (_lib.ptr(self.d_offs), _lib.ptr(self.d_pts) if self.rows else None, _lib.ptr(self.d_w) if self.ws is not None and self.rows else None)


def work_sizes(X, Y, flags):
    """(full, least); (0, 0) for flags that the library refuses"""
    from tlc_gnn_amd import engine
    try:
        return engine.dgm_gram_work_bytes(X.B, Y.B, X.max_points, Y.max_points, flags)
    except _lib.TlcError:
        return 0, 0


def forward(torch, X, Y, gamma, scale, flags, work_bytes=None, expect=0, max_nx=None, max_ny=None):
    """the raw entry -> (out, status_x, status_y) as numpy; sentinels 7.0 / 9 wherever it does not write"""
    shape = (X.B,) if flags & PAIRED else (X.B, Y.B)
    out = torch.full(shape, 7.0, dtype=torch.float64, device="cuda")
    sx, sy = (torch.full((max(S.B, 1),), 9, dtype=torch.uint8, device="cuda") for S in (X, Y))
    if work_bytes is None:
        work_bytes = work_sizes(X, Y, flags)[0]
    work = torch.empty(work_bytes, dtype=torch.uint8, device="cuda") if work_bytes else None
    rc = _lib.lib().tlc_dgm_gram(C.c_int32(X.B), *X.ptrs(), C.c_int32(Y.B), *Y.ptrs(), C.c_double(gamma), C.c_double(scale), C.c_uint32(flags),
                                 C.c_int64(X.max_points if max_nx is None else max_nx), C.c_int64(Y.max_points if max_ny is None else max_ny),
                                 _lib.ptr(out), _lib.ptr(sx), _lib.ptr(sy), _lib.ptr(work), C.c_int64(work_bytes), _lib.stream_ptr())
    assert rc == expect, (rc, _lib.lib().tlc_last_error())
    return out.cpu().numpy(), sx.cpu().numpy()[:X.B], sy.cpu().numpy()[:Y.B]


def vjp(torch, X, Y, gamma, scale, flags, G, sx=None, sy=None, work_bytes=None, expect=0):
    """the raw VJP -> (grad_pts [rows, 2], grad_w [rows] or None) as numpy; sentinel 7.0"""
    gp = torch.full((max(X.rows, 1), 2), 7.0, dtype=torch.float64, device="cuda")
    gw = None if X.ws is None or not X.rows else torch.full((X.rows,), 7.0, dtype=torch.float64, device="cuda")
    d_sx = _dev(torch, np.zeros(max(X.B, 1)) if sx is None else sx, torch.uint8)
    d_sy = _dev(torch, np.zeros(max(Y.B, 1)) if sy is None else sy, torch.uint8)
    d_G = _dev(torch, G, torch.float64)
    if work_bytes is None:
        work_bytes = work_sizes(X, Y, flags)[0]
    work = torch.empty(work_bytes, dtype=torch.uint8, device="cuda") if work_bytes else None
    rc = _lib.lib().tlc_dgm_gram_vjp(C.c_int32(X.B), *X.ptrs(), C.c_int32(Y.B), *Y.ptrs(), C.c_double(gamma), C.c_double(scale), C.c_uint32(flags),
                                     C.c_int64(X.max_points), C.c_int64(Y.max_points), _lib.ptr(d_sx), _lib.ptr(d_sy), _lib.ptr(d_G), _lib.ptr(gp),
                                     _lib.ptr(gw), _lib.ptr(work), C.c_int64(work_bytes), _lib.stream_ptr())
    assert rc == expect, (rc, _lib.lib().tlc_last_error())
    return gp.cpu().numpy()[:X.rows], None if gw is None else gw.cpu().numpy()


def check_values(out, refs, scale, what):
    """out[i, j] against refs[i][j] (ref_pair results) within the derived bound; prints the worst ratio"""
    worst = 0.0
    for i, row in enumerate(refs):
        for j, r in enumerate(row):
            err, bound = abs(float(cases.LD(out[i][j]) - r["k"])), cases.value_bound(r, scale)
            assert err <= bound, (what, i, j, out[i][j], float(r["k"]), err, bound)
            worst = max(worst, err / bound if bound else 0.0)
    print("%s: worst error / bound = %.3f" % (what, worst))


def check_grad(gp, gw, X, i, pairs, Grow, gamma, scale, ny, what):
    rp, rw, bp, bw = cases.ref_grad(pairs, Grow, X.weights(i), gamma, scale, ny)
    s = slice(X.offs[i], X.offs[i + 1])
    ep = np.abs((gp[s].astype(cases.LD) - rp).astype(np.float64))
    assert (ep <= bp).all(), (what, i, float((ep / np.maximum(bp, 1e-300)).max()))
    if gw is not None:
        ew = np.abs((gw[s].astype(cases.LD) - rw).astype(np.float64))
        assert (ew <= bw).all(), (what, i, float((ew / np.maximum(bw, 1e-300)).max()))
    return float((ep / np.maximum(bp, 1e-300)).max()) if ep.size else 0.0


# ---- 1. values and both gradients at every cut ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mirror,weights,gamma,spread", [(1, 0, 1e-3, 30.0), (0, 1, 1e4, 0.02), (1, 1, 1.0, 1.0), (0, 0, 30.0, 0.3)])
def test_values_and_gradients_at_every_cut(torch_cuda, mirror, weights, gamma, spread):
    """Diagram sizes 0, 1, 63, 64, 65 and the slice / group constant - 1, + 0, + 1 on both sides: ALL mode meets every (n, m), PAIRED
    mode the pairs (i, 7 - i).  Values, the first argument's gradient and (roles swapped, G transposed) the second argument's."""
    torch = torch_cuda
    rs = np.random.RandomState(int(gamma * 7) % 1000 + mirror)
    scale = -0.37 if mirror else 1.9
    dX = [cases.random_diagram(rs, n, spread) for n in cases.CUT_SIZES]
    dY = [cases.random_diagram(rs, m, spread) for m in cases.CUT_SIZES]
    X = Side(torch, dX, [cases.random_weights(rs, len(d)) for d in dX] if weights else None)
    Y = Side(torch, dY, [cases.random_weights(rs, len(d)) for d in dY] if weights else None)
    assert weights == 0 or min(w.min() for w in X.ws if len(w)) < 0                      # negative weights included
    fl = MIRROR if mirror else 0
    refs = [[cases.ref_pair(dX[i], X.weights(i), dY[j], Y.weights(j), gamma, scale, mirror) for j in range(Y.B)] for i in range(X.B)]
    out, sx, sy = forward(torch, X, Y, gamma, scale, ALL | fl)
    assert not sx.any() and not sy.any()
    check_values(out, refs, scale, "ALL")
    for i in range(X.B):
        for j in range(Y.B):
            if not len(dX[i]) or not len(dY[j]):
                assert out[i, j] == 0.0 and not np.signbit(out[i, j])                   # +0.0 even under a negative scale
    Yr = Side(torch, dY[::-1], None if Y.ws is None else Y.ws[::-1])
    outp, _, _ = forward(torch, X, Yr, gamma, scale, PAIRED | fl)
    check_values(outp[:, None], [[refs[i][Y.B - 1 - i]] for i in range(X.B)], scale, "PAIRED")
    assert same_bits(outp, np.array([out[i, Y.B - 1 - i] for i in range(X.B)]))
    # the gradients
    G = rs.uniform(-1.0, 1.0, (X.B, Y.B))
    gp, gw = vjp(torch, X, Y, gamma, scale, ALL | fl, G)
    worst = max(check_grad(gp, gw, X, i, refs[i], G[i], gamma, scale, Y.B, "ALL x") for i in range(X.B))
    # roles swapped and G transposed: Y's diagrams as the first argument against a part of X (the references are made from Y's side)
    sub = [0, 1, 2, 3, 4, 7]
    Xs = Side(torch, [dX[i] for i in sub], None if X.ws is None else [X.ws[i] for i in sub])
    refs_t = [[cases.ref_pair(dY[j], Y.weights(j), dX[i], X.weights(i), gamma, scale, mirror) for i in sub] for j in range(Y.B)]
    Gt = np.ascontiguousarray(G[sub].T)
    gpy, gwy = vjp(torch, Y, Xs, gamma, scale, ALL | fl, Gt)
    worst = max([worst] + [check_grad(gpy, gwy, Y, j, refs_t[j], Gt[j], gamma, scale, Xs.B, "ALL y") for j in range(Y.B)])
    Gp = rs.uniform(-1.0, 1.0, X.B)
    gpp, gwp = vjp(torch, X, Yr, gamma, scale, PAIRED | fl, Gp)
    worst = max([worst] + [check_grad(gpp, gwp, X, i, [refs[i][Y.B - 1 - i]], [Gp[i]], gamma, scale, 1, "PAIRED x") for i in range(X.B)])
    print("gradients: worst error / bound = %.3f" % worst)
    assert (gw is None) == (not weights)


# ---- 2. closed forms ------------------------------------------------------------------------------------------------------------------------
def test_exact_closed_forms(torch_cuda):
    torch = torch_cuda
    one = np.tile([[0.25, 0.75]], (65, 1))
    X, F = Side(torch, [one]), Side(torch, [one + 40.0])
    assert forward(torch, X, X, 3.0, 1.0, ALL)[0][0, 0] == 65.0 * 65.0                   # exp(-0.0) = 1, 65 * 65 times
    assert forward(torch, X, X, 3.0, 1.0, PAIRED)[0][0] == 65.0 * 65.0
    assert forward(torch, X, F, 1.0, 1.0, ALL)[0][0, 0] == 0.0                           # exp(-3200) = 0
    assert forward(torch, X, F, 1.0, 1.0, ALL | MIRROR)[0][0, 0] == 0.0
    diag = np.stack([np.arange(5.0), np.arange(5.0)], 1)                                 # e1 and e2 are the same bits on the diagonal
    assert forward(torch, Side(torch, [diag]), X, 0.5, 1.0, ALL | MIRROR)[0][0, 0] == 0.0
    gp, _ = vjp(torch, X, F, 1.0, 1.0, ALL | MIRROR, np.ones((1, 1)))
    assert not gp.any()


# ---- 3. the bits depend on the operands alone -------------------------------------------------------------------------------------------------
def test_every_pair_alone_equals_the_batch(torch_cuda):
    """300 x 300 tiny diagrams: 90 000 units, more than the grid's wavefronts.  Alone: every pair of the 48 x 48 corner blocks (first
    and last diagrams of both sides, so units of the first pass of the grid and of its last), each as the 1 x 1 call on the same
    buffers (offsets are absolute rows, so &offs[i] is a batch of one); every entry of the batch against the restated order."""
    torch = torch_cuda
    rs = np.random.RandomState(41)
    B, K = 300, 48
    dgms = [cases.random_diagram(rs, int(k)) for k in rs.randint(0, 6, B)]
    X = Side(torch, dgms, [cases.random_weights(rs, len(d)) for d in dgms])
    gamma, scale, fl = 0.8, 0.6, ALL | MIRROR
    out, _, _ = forward(torch, X, X, gamma, scale, fl)
    again, _, _ = forward(torch, X, X, gamma, scale, fl)
    assert same_bits(out, again)                                                          # run to run
    want = cases.restate_gram(dgms[:12], X.ws[:12], dgms[:12], X.ws[:12], gamma, scale, True)
    assert np.allclose(out[:12, :12], want, rtol=0, atol=1e-12)
    alone = torch.full((B, B), 7.0, dtype=torch.float64, device="cuda")
    st = torch.zeros(2, dtype=torch.uint8, device="cuda")
    L, stream = _lib.lib(), _lib.stream_ptr()
    po, pp, pw, pa, ps = X.d_offs.data_ptr(), _lib.ptr(X.d_pts), _lib.ptr(X.d_w), alone.data_ptr(), st.data_ptr()
    cg, cs, cf, c5, c0 = C.c_double(gamma), C.c_double(scale), C.c_uint32(fl), C.c_int64(5), C.c_int64(0)
    one = C.c_int32(1)
    ends = list(range(K)) + list(range(B - K, B))
    for i in ends:
        xo = C.c_void_p(po + 8 * i)
        for j in ends:
            rc = L.tlc_dgm_gram(one, xo, pp, pw, one, C.c_void_p(po + 8 * j), pp, pw, cg, cs, cf, c5, c5, C.c_void_p(pa + 8 * (i * B + j)),
                                C.c_void_p(ps), C.c_void_p(ps + 1), None, c0, stream)
            assert rc == 0
    got = alone.cpu().numpy()
    sel = np.ix_(ends, ends)
    assert same_bits(out[sel], got[sel]) and not (got[sel] == 7.0).any()
    # PAIRED is the diagonal, SYMMETRIC the general call: upper triangle and diagonal bit for bit, the lower triangle its transpose
    assert same_bits(forward(torch, X, X, gamma, scale, PAIRED | MIRROR)[0], np.diag(out).copy())
    copy = Side(torch, dgms, X.ws)
    sym, sx, sy = forward(torch, X, X, gamma, scale, fl | SYMMETRIC)
    gen, _, _ = forward(torch, X, copy, gamma, scale, fl)
    iu = np.triu_indices(B)
    assert same_bits(sym[iu], gen[iu]) and same_bits(sym, sym.T) and not sx.any() and not sy.any()


def test_gradient_rows_alone_equal_the_batch(torch_cuda):
    torch = torch_cuda
    rs = np.random.RandomState(43)
    dX = [cases.random_diagram(rs, n) for n in (3, 0, 64, 65, 130, 1, 70)]
    dY = [cases.random_diagram(rs, m) for m in (5, 64, 0, 65, 200)]
    X = Side(torch, dX, [cases.random_weights(rs, len(d)) for d in dX])
    Y = Side(torch, dY, [cases.random_weights(rs, len(d)) for d in dY])
    G = rs.uniform(-1.0, 1.0, (X.B, Y.B))
    gamma, scale = 2.5, 0.7
    for fl in (ALL, ALL | MIRROR):
        gp, gw = vjp(torch, X, Y, gamma, scale, fl, G)
        gp2, gw2 = vjp(torch, X, Y, gamma, scale, fl, G)
        assert same_bits(gp, gp2) and same_bits(gw, gw2) and not (gp == 7.0).any()       # run to run, every row written
        for i in range(X.B):
            one = Side(torch, [dX[i]], [X.ws[i]])
            ap, aw = vjp(torch, one, Y, gamma, scale, fl, G[i:i + 1])
            s = slice(X.offs[i], X.offs[i + 1])
            assert same_bits(ap, gp[s]) and (not len(dX[i]) or same_bits(aw, gw[s])), i
        # PAIRED: row i against Y_i is the ALL call on (X_i, Y_i)
        Xp = Side(torch, dX[:5], X.ws[:5])
        Gp = rs.uniform(-1.0, 1.0, 5)
        pp, pw = vjp(torch, Xp, Y, gamma, scale, (fl & MIRROR) | PAIRED, Gp)
        for i in range(5):
            ap, aw = vjp(torch, Side(torch, [dX[i]], [X.ws[i]]), Side(torch, [dY[i]], [Y.ws[i]]), gamma, scale, fl, Gp[i:i + 1].reshape(1, 1))
            s = slice(Xp.offs[i], Xp.offs[i + 1])
            assert same_bits(ap, pp[s]) and (not len(dX[i]) or same_bits(aw, pw[s])), i
    # the order of include/tlcgnn.h, restated with numpy's exp: equal up to the two libraries' exponentials
    gp, gw = vjp(torch, X, Y, gamma, scale, ALL | MIRROR, G)
    for i in range(X.B):
        rp, rw = cases.restate_grad_rows(dX[i], X.ws[i], dY, Y.ws, G[i], gamma, scale, True)
        s = slice(X.offs[i], X.offs[i + 1])
        assert np.allclose(gp[s], rp, rtol=0, atol=1e-11) and np.allclose(gw[s], rw, rtol=0, atol=1e-11)


def test_any_workspace_gives_the_same_bits(torch_cuda):
    """Diagrams above a slice and a group: the unit partials go through d_work; the least size runs one X diagram per launch."""
    torch = torch_cuda
    rs = np.random.RandomState(47)
    S, Gr = cases.SLICE, cases.GROUP
    dX = [cases.random_diagram(rs, n) for n in (S + 5, 3, 2 * S + 1, 0, 70)]
    dY = [cases.random_diagram(rs, m) for m in (10, Gr + 1, 0, 2 * Gr + 3, 64)]
    X, Y = Side(torch, dX), Side(torch, dY)
    gamma, scale = 4.0, 1.1
    for fl in (ALL | MIRROR, PAIRED | MIRROR):
        full, least = work_sizes(X, Y, fl)
        assert 0 < least < full
        a = forward(torch, X, Y, gamma, scale, fl, work_bytes=full)[0]
        b = forward(torch, X, Y, gamma, scale, fl, work_bytes=least)[0]
        c = forward(torch, X, Y, gamma, scale, fl, work_bytes=(least + full) // 2 + 3)[0]
        assert same_bits(a, b) and same_bits(a, c) and not (a == 7.0).any()
        forward(torch, X, Y, gamma, scale, fl, work_bytes=least - 1, expect=INVALID)
    # every pair alone (its own declared sizes: most of them the one-unit case without a workspace) is the batch's entry
    out = forward(torch, X, Y, gamma, scale, ALL | MIRROR)[0]
    for i in range(X.B):
        for j in range(Y.B):
            one = forward(torch, Side(torch, [dX[i]]), Side(torch, [dY[j]]), gamma, scale, ALL | MIRROR)[0]
            assert same_bits(one[0, 0], out[i, j]), (i, j)
    r = cases.ref_pair(dX[2], None, dY[3], None, gamma, scale, True)
    assert abs(float(cases.LD(out[2, 3]) - r["k"])) <= cases.value_bound(r, scale)
    # the symmetric call through the workspace
    sym = forward(torch, X, X, gamma, scale, ALL | MIRROR | SYMMETRIC)[0]
    gen = forward(torch, X, Side(torch, dX), gamma, scale, ALL | MIRROR)[0]
    iu = np.triu_indices(X.B)
    assert same_bits(sym[iu], gen[iu]) and same_bits(sym, sym.T)
    # the VJP's chunk prefix lives in the same workspace
    Gp = rs.uniform(-1.0, 1.0, X.B)
    full, least = work_sizes(X, Y, PAIRED | MIRROR)
    ga = vjp(torch, X, Y, gamma, scale, PAIRED | MIRROR, Gp, work_bytes=full)[0]
    gb = vjp(torch, X, Y, gamma, scale, PAIRED | MIRROR, Gp, work_bytes=least)[0]
    assert same_bits(ga, gb) and not (ga == 7.0).any()
    vjp(torch, X, Y, gamma, scale, PAIRED | MIRROR, Gp, work_bytes=least - 1, expect=INVALID)


# ---- 4. one large pair ------------------------------------------------------------------------------------------------------------------------
def test_one_pair_of_5000_points(torch_cuda):
    torch = torch_cuda
    rs = np.random.RandomState(53)
    n = m = 5000
    dX, dY = cases.random_diagram(rs, n), cases.random_diagram(rs, m)
    X, Y = Side(torch, [dX]), Side(torch, [dY])
    gamma, scale = 50.0, 0.2
    r = cases.ref_pair(dX, None, dY, None, gamma, scale, True, rows=128)
    out, sx, sy = forward(torch, X, Y, gamma, scale, ALL | MIRROR)
    check_values(out, [[r]], scale, "5000 x 5000")
    assert same_bits(forward(torch, X, Y, gamma, scale, PAIRED | MIRROR)[0], out[0])
    gp, _ = vjp(torch, X, Y, gamma, scale, PAIRED | MIRROR, np.array([-1.5]))
    print("5000 x 5000 gradient: worst error / bound = %.3f" % check_grad(gp, None, X, 0, [r], [-1.5], gamma, scale, 1, "5000"))
    assert same_bits(gp, vjp(torch, X, Y, gamma, scale, ALL | MIRROR, np.array([[-1.5]]))[0])


# ---- 5. NaN / Inf ------------------------------------------------------------------------------------------------------------------------------
def test_a_bad_value_fails_its_diagram_alone(torch_cuda):
    torch = torch_cuda
    rs = np.random.RandomState(59)
    dX = [cases.random_diagram(rs, n) for n in (4, 70, 9, 1100)]
    dY = [cases.random_diagram(rs, m) for m in (6, 3, 1030)]
    wX, wY = [cases.random_weights(rs, len(d)) for d in dX], [cases.random_weights(rs, len(d)) for d in dY]
    X, Y = Side(torch, dX, wX), Side(torch, dY, wY)
    gamma, scale, fl = 1.5, 1.0, ALL | MIRROR
    G = rs.uniform(-1.0, 1.0, (4, 3))
    clean = forward(torch, X, Y, gamma, scale, fl)[0]
    gclean = vjp(torch, X, Y, gamma, scale, fl, G)
    bX = [d.copy() for d in dX]
    bX[1][69, 1] = np.nan                                                                 # a NaN coordinate in X_1
    bwY = [w.copy() for w in wY]
    bwY[2][1029] = np.inf                                                                 # an Inf weight in Y_2
    Xb, Yb = Side(torch, bX, wX), Side(torch, dY, bwY)
    out, sx, sy = forward(torch, Xb, Yb, gamma, scale, fl)
    assert sx.tolist() == [0, 3, 0, 0] and sy.tolist() == [0, 0, 3]
    assert np.isnan(out[1]).all() and np.isnan(out[:, 2]).all()
    keep = np.ones((4, 3), dtype=bool)
    keep[1], keep[:, 2] = False, False
    assert same_bits(out[keep], clean[keep])
    gp, gw = vjp(torch, Xb, Yb, gamma, scale, fl, G, sx=sx, sy=sy)
    s = slice(X.offs[1], X.offs[2])
    assert not gp[s].any() and not gw[s].any()                                            # zero rows
    # the other rows: the clean run without the failed column (an upstream of zero adds +-0.0 and changes no bit)
    G0 = G.copy()
    G0[:, 2] = 0.0
    gp0, gw0 = vjp(torch, X, Y, gamma, scale, fl, G0)
    rest = np.ones(X.rows, dtype=bool)
    rest[s] = False
    assert same_bits(gp[rest], gp0[rest]) and same_bits(gw[rest], gw0[rest])
    assert not same_bits(gp0[rest], gclean[0][rest])
    # PAIRED, and the wrappers name the diagram
    outp, sxp, syp = forward(torch, Side(torch, bX[:3], wX[:3]), Yb, gamma, scale, PAIRED | MIRROR)
    assert sxp.tolist() == [0, 3, 0] and syp.tolist() == [0, 0, 3] and np.isnan(outp[1:]).all() and same_bits(outp[0], clean[0, 0])
    from tlc_gnn_amd import autograd, ops
    with pytest.raises(RuntimeError, match="diagram 1 of x"):
        ops.diagram_gram(Xb.d_pts, Xb.d_offs, Y.d_pts, Y.d_offs)
    with pytest.raises(RuntimeError, match="diagram 2 of y"):
        autograd.diagram_gram(X.d_pts, X.d_offs, Yb.d_pts, Yb.d_offs, wy=Yb.d_w)
    r = ops.diagram_gram(Xb.d_pts, Xb.d_offs, check=False)
    assert r["status_x"].tolist() == [0, 3, 0, 0] and bool(torch.isnan(r["out"][1]).all()) and bool(torch.isnan(r["out"][:, 1]).all())


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(torch_cuda):
    torch = torch_cuda
    rs = np.random.RandomState(61)
    dX, dY = [cases.random_diagram(rs, n) for n in (4, 7, 2)], [cases.random_diagram(rs, m) for m in (3, 5, 6)]
    X, Y = Side(torch, dX), Side(torch, dY)
    Xw = Side(torch, dX, [cases.random_weights(rs, len(d)) for d in dX])

    def refused(Xs, Ys, gamma=1.0, scale=1.0, flags=ALL, **kw):
        out, sx, sy = forward(torch, Xs, Ys, gamma, scale, flags, expect=INVALID, **kw)
        assert (out == 7.0).all() and (sx == 9).all() and (sy == 9).all()
        shape = (Xs.B,) if flags & PAIRED else (Xs.B, Ys.B)
        if "max_nx" not in kw and "max_ny" not in kw:
            gp, gw = vjp(torch, Xs, Ys, gamma, scale, flags, np.ones(shape), expect=INVALID)
            assert (gp == 7.0).all() and (gw is None or (gw == 7.0).all())

    for kw in (dict(gamma=0.0), dict(gamma=-2.0), dict(gamma=float("nan")), dict(gamma=float("inf")), dict(scale=float("nan")),
               dict(scale=float("-inf")), dict(flags=0), dict(flags=ALL | PAIRED), dict(flags=ALL | 32), dict(flags=PAIRED | SYMMETRIC),
               dict(flags=ALL | SYMMETRIC)):                                              # (different X and Y buffers)
        refused(X, Y, **kw)
        refused(Xw, Y, **kw)
    refused(X, Side(torch, dY[:2]), flags=PAIRED)                                         # nx != ny
    refused(X, Y, max_nx=6)                                                               # a diagram above its max_points
    refused(X, Y, max_ny=5)
    for S in (X, Y):                                                                      # offsets that decrease
        good = S.d_offs.clone()
        S.d_offs[1] = S.d_offs[2] + 1
        refused(X, Y)
        S.d_offs.copy_(good)
    X.d_offs[0] = -1
    refused(X, Y)
    X.d_offs[0] = 0
    out, sx, sy = forward(torch, X, Y, 1.0, 1.0, ALL)                                     # and the same buffers are accepted afterwards
    assert not (out == 7.0).any() and not sx.any() and not sy.any()
    # empty batches: TLC_OK, nothing written
    E = Side(torch, [])
    assert forward(torch, E, Y, 1.0, 1.0, ALL)[0].shape == (0, 3)
    out, _, sy = forward(torch, X, E, 1.0, 1.0, ALL)
    assert out.shape == (3, 0)
    gp, _ = vjp(torch, X, E, 1.0, 1.0, ALL, np.zeros((3, 0)))
    assert not gp.any()                                                                   # every row written: zeros


# ---- 7. autograd ----------------------------------------------------------------------------------------------------------------------------------
def _leaf(torch, a):
    return _dev(torch, a, torch.float64).requires_grad_(True)


def test_gradcheck(torch_cuda):
    from tlc_gnn_amd import autograd, ops
    torch = torch_cuda
    rs = np.random.RandomState(67)
    dX, dY = [cases.random_diagram(rs, n) for n in (3, 0, 4)], [cases.random_diagram(rs, m) for m in (2, 5, 1)]
    xo, x = cases.pack(dX)
    yo, y = cases.pack(dY)
    d_xo, d_yo = _dev(torch, xo, torch.int64), _dev(torch, yo, torch.int64)
    x, y = _leaf(torch, x), _leaf(torch, y)
    wx, wy = _leaf(torch, cases.random_weights(rs, 7)), _leaf(torch, cases.random_weights(rs, 8))
    for kernel, sigma in (("pss", 0.3), ("gauss", 0.4)):
        for paired in (False, True):
            fn = lambda a, b, c, d: autograd.diagram_gram(a, d_xo, b, d_yo, wx=c, wy=d, kernel=kernel, sigma=sigma, paired=paired)
            out = fn(x, y, wx, wy)
            assert out.shape == ((3,) if paired else (3, 3)) and out.requires_grad
            assert torch.autograd.gradcheck(fn, (x, y, wx, wy))                           # the fp64 defaults: eps 1e-6, atol 1e-5, rtol 1e-3
            sym = lambda a, c: autograd.diagram_gram(a, d_xo, wx=c, kernel=kernel, sigma=sigma, paired=paired)
            assert torch.autograd.gradcheck(sym, (x, wx))
            if not paired:
                both = autograd.diagram_gram(x, d_xo, x.detach(), d_xo, wx=wx, wy=wx.detach(), kernel=kernel, sigma=sigma)
                assert torch.equal(torch.triu(sym(x, wx)), torch.triu(both))
        dist = lambda a, b: autograd.diagram_kernel_distance(a, d_xo, b, d_yo, kernel=kernel, sigma=sigma)
        assert torch.autograd.gradcheck(dist, (x, y))
        d = dist(x, y)
        assert d.shape == (3,) and bool((d >= 0).all())
        assert float(autograd.diagram_kernel_distance(x, d_xo, x.detach(), d_xo, kernel=kernel, sigma=sigma).abs().max()) == 0.0
    # no weights: no weight gradient is asked of the library; PWG weights are torch ops, so C and p get gradients
    Cp = torch.tensor([1.3, 0.8], dtype=torch.float64, device="cuda", requires_grad=True)
    pwg = lambda a, cp: autograd.diagram_gram(a, d_xo, wx=ops.pwg_weights(a, cp[0], cp[1]), kernel="gauss", sigma=0.5)
    assert torch.autograd.gradcheck(pwg, (x, Cp))
    f32 = autograd.diagram_gram(x.detach().float().requires_grad_(True), d_xo)
    assert f32.dtype == torch.float32 and f32.requires_grad
    one = autograd.diagram_gram(x[:3], y=y[:2])                                           # offsets None: one diagram each
    assert torch.equal(one[0, 0], autograd.diagram_gram(x, d_xo, y, d_yo)[0, 0])
    r = ops.diagram_gram(x, d_xo, y, d_yo, kernel="pss", sigma=0.3)
    assert torch.equal(r["out"], autograd.diagram_gram(x, d_xo, y, d_yo, sigma=0.3).detach()) and not r["out"].requires_grad


# ---- 8. topo, the teacher and a training smoke ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def graphs(torch_cuda):
    import pd_grad_cases as pg
    torch = torch_cuda
    rs = np.random.RandomState(21)
    gs = [(n, pg.small_graph(rs, n)) for n in (5, 9, 16, 12)] + [(70, pg.chord_graph(rs, 70, 120))]
    no, eo, E, f = pg.pack(gs, [pg.distinct_values(rs, n) for n, _ in gs])
    return dict(no=_dev(torch, no, torch.int64), eo=_dev(torch, eo, torch.int64), E=_dev(torch, E, torch.int32), f=_dev(torch, f, torch.float64),
                B=len(gs), span=float(f.max() - f.min()))


@pytest.mark.parametrize("which,kernel", [("ord0+ext1", "pss"), ("ext1", "gauss"), ("ord0+ext0+ext1", "pss")])
def test_topo_gram_and_kernel_distance(torch_cuda, graphs, which, kernel):
    """topo.gram / topo.kernel_distance_to against the same chain built by hand: topo's diagrams, the longdouble restatement on their
    points, and its gradient pushed through the diagrams' own backward (a selection of node values, so bounds travel the same way)."""
    from tlc_gnn_amd import topo
    torch, g = torch_cuda, graphs
    B, sigma = g["B"], 0.2 * g["span"]
    gamma, scale, mirror = cases.kernel_params(kernel, sigma)
    f = g["f"].clone().requires_grad_(True)
    K = topo.gram(f, g["no"], g["eo"], g["E"], which=which, sigma=sigma, kernel=kernel)
    assert K.shape == (B, B) and K.dtype == torch.float64 and torch.equal(K, K.t())
    Gm = np.random.RandomState(2).standard_normal((B, B))
    K.backward(_dev(torch, Gm, torch.float64))
    f2 = g["f"].clone().requires_grad_(True)
    pts, offs = topo._select(f2, g["no"], g["eo"], g["E"], which, "host")
    P, po = pts.detach().cpu().numpy(), offs.cpu().numpy()
    D = [P[po[b]:po[b + 1]] for b in range(B)]
    refs = [[cases.ref_pair(D[i], None, D[j], None, gamma, scale, mirror) for j in range(B)] for i in range(B)]
    check_values(K.detach().cpu().numpy(), refs, scale, "topo.gram")
    Gs = Gm + Gm.T                                                                        # Y is X: G + G^T
    # (2^-45 below: the reference rounded to fp64, and the selection's own sum -- a node value is the coordinate of fewer than 256 points)
    gp, bp = np.zeros_like(P), np.zeros_like(P)
    for i in range(B):
        rp, _, b, _ = cases.ref_grad(refs[i], Gs[i], None, gamma, scale, B)
        gp[po[i]:po[i + 1]], bp[po[i]:po[i + 1]] = rp.astype(np.float64), b + np.abs(rp.astype(np.float64)) * 2.0 ** -45
    pts.backward(_dev(torch, gp, torch.float64), retain_graph=True)
    want = f2.grad.clone()
    f2.grad = None
    pts.backward(_dev(torch, bp, torch.float64))
    assert bool(((f.grad - want).abs() <= f2.grad + 1e-300).all()) and float(f.grad.abs().max()) > 0
    # the distance to the diagrams of other values
    rs = np.random.RandomState(3)
    other = g["f"] + 0.2 * g["span"] * _dev(torch, rs.standard_normal(g["f"].numel()), torch.float64)
    tp, to = topo._select(other, g["no"], g["eo"], g["E"], which, "host")
    f3 = g["f"].clone().requires_grad_(True)
    d = topo.kernel_distance_to(f3, g["no"], g["eo"], g["E"], tp, to, which=which, sigma=sigma, kernel=kernel)
    assert d.shape == (B,) and bool((d > 0).all())
    T, tO = tp.cpu().numpy(), to.cpu().numpy()
    for b in range(B):
        Tb = T[tO[b]:tO[b + 1]]
        xx, yy, xy = refs[b][b], cases.ref_pair(Tb, None, Tb, None, gamma, scale, mirror), cases.ref_pair(D[b], None, Tb, None, gamma, scale, mirror)
        want_d = xx["k"] + yy["k"] - 2 * xy["k"]
        bound = cases.value_bound(xx, scale) + cases.value_bound(yy, scale) + 2 * cases.value_bound(xy, scale)
        bound += 3 * 2.0 ** -53 * float(abs(xx["k"]) + abs(yy["k"]) + 2 * abs(xy["k"]))    # the two additions and the doubling's operand
        assert abs(float(cases.LD(float(d[b])) - want_d)) <= bound, b
    d.sum().backward()
    assert float(f3.grad.abs().max()) > 0
    zero = topo.kernel_distance_to(g["f"], g["no"], g["eo"], g["E"], pts.detach(), offs, which=which, sigma=sigma, kernel=kernel)
    assert float(zero.abs().max()) <= 1e-12 * float(K.abs().max())


def test_teacher_model_with_the_pss_loss(torch_cuda):
    torch = torch_cuda
    from tlc_gnn_amd.Knowledge_Distillation.Teacher_model import Teacher_Model
    ei = torch.tensor([[0, 1, 1, 2, 0, 1, 2], [1, 0, 2, 1, 0, 1, 2]]).cuda()              # four edges, then the three self loops
    f = torch.rand(3, 1).cuda()
    PD = torch.tensor([[0.1, 0.5], [0.2, 0.3], [0.0, 0.9], [0.4, 0.6]]).cuda()
    m = Teacher_Model(type='GAT', dropout=0.0).cuda().train()
    out = m(f, ei, PD, kernel='pss', grad_PI=False)
    loss0, parts = out[2], out[3:6]
    assert loss0.shape == (1,) and loss0.requires_grad and float(loss0) >= 0 and all(float(p) == 0 and p.shape == (1,) for p in parts)
    loss0.backward()
    assert any(p.grad is not None and float(p.grad.abs().max()) > 0 for p in m.parameters())
    wide = m(f, ei, PD, kernel='pss', grad_PI=False, sigma=5.0)[2]
    assert float(wide) != float(loss0)
    # batched: two copies of the graph, offsets given
    ei2 = torch.cat([torch.cat([ei[:, :4], ei[:, :4] + 3], 1), torch.arange(6).repeat(2, 1).cuda()], 1)
    ptr = torch.tensor([0, 4, 8]).cuda()
    b = m(torch.cat([f, f]), ei2, torch.cat([PD, PD]), kernel='pss', grad_PI=False, graph_ptr=torch.tensor([0, 3, 6]).cuda(), edge_ptr=ptr)[2]
    assert abs(float(b) - 2 * float(loss0)) <= 1e-4 * (1 + abs(float(loss0)))
    with pytest.raises(NotImplementedError):
        m(f, ei, PD, kernel='sliced', grad_PI=False)


def test_training_smoke(torch_cuda):
    """64 small random graphs; f a free parameter started at a perturbation of the hidden values; 200 Adam steps on the summed squared
    PSS distance to the hidden values' diagrams.  The loss stays finite and ends below where it began (the ratio reached is in
    DESIGN.md 6.17)."""
    import pd_grad_cases as pg
    from tlc_gnn_amd import topo
    torch = torch_cuda
    rs = np.random.RandomState(31)
    gs = [(n, pg.small_graph(rs, n)) for n in rs.randint(6, 20, size=64)]
    no, eo, E, hidden = pg.pack(gs, [pg.distinct_values(rs, n) for n, _ in gs])
    no, eo, E = _dev(torch, no, torch.int64), _dev(torch, eo, torch.int64), _dev(torch, E, torch.int32)
    span = float(hidden.max() - hidden.min())
    tp, to = topo._select(_dev(torch, hidden, torch.float64), no, eo, E, "ord0+ext1", "host")
    f = _dev(torch, hidden + 0.1 * span * rs.standard_normal(len(hidden)), torch.float64).requires_grad_(True)
    opt = torch.optim.Adam([f], lr=0.01 * span)
    losses = []
    for _ in range(200):
        opt.zero_grad()
        loss = topo.kernel_distance_to(f, no, eo, E, tp, to, sigma=0.05 * span).sum()
        loss.backward()
        opt.step()
        losses.append(float(loss))
    print("kernel distance training: first %.6e last %.6e ratio %.4f" % (losses[0], losses[-1], losses[-1] / losses[0]))
    assert np.isfinite(losses).all() and losses[-1] < losses[0]

"""GPU: persistence landscapes of packed diagrams and their gradient (csrc/landscape.hip; engine.landscape / landscape_vjp;
ops.landscape; autograd.diagram_landscape; topo.landscapes).

The reference is the numpy restatement of include/tlcgnn.h's definition in tests/landscape_cases.py.  Every value is one fp64
subtraction and one min, every gradient a sum of +-g in a fixed order: values, winners and gradients are compared with
np.array_equal on the bits.  There is no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import landscape_cases as cases
from tlc_gnn_amd import _lib

pytestmark = pytest.mark.gpu
WAVE_NMAX, LDS_NMAX, KMAX = _lib.LS_WAVE_NMAX, _lib.LS_LDS_NMAX, _lib.LS_KMAX
SIZES = cases.class_sizes(WAVE_NMAX, LDS_NMAX)
TS = (1, 63, 64, 65, 256, 257)
KS = (1, 2, 5, 16)                      # K > n occurs; the instantiations 1, 2, 8 (below its K) and 16
MORE_KS = (3, 4, 7, 8, 15)              # with KS: every instantiation (1, 2, 4, 8, 16) at its own K and just below it


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
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


class Packed:
    """a batch on the device, and the raw entries on it with outputs pre-filled with sentinels"""

    def __init__(self, torch, dgms, ts):
        self.torch, self.dgms, self.ts = torch, dgms, np.asarray(ts, dtype=np.float64)
        self.offs, self.pts = cases.pack(dgms)
        self.B, self.T = len(dgms), len(self.ts)
        self.sizes = np.diff(self.offs)
        self.max_points = int(self.sizes.max()) if self.B else 0
        self.d_offs, self.d_pts = _dev(torch, self.offs, torch.int64), _dev(torch, self.pts, torch.float64)
        self.d_ts = _dev(torch, self.ts, torch.float64)

    def forward(self, K, winners=True, work_bytes=None, expect=0):
        """-> (out [B, K, T], winner [B, K, T] or None, status [B]) as numpy; sentinels 7.0 / -9 / 9 wherever the entry does not write"""
        torch = self.torch
        from tlc_gnn_amd import engine
        out = torch.full((self.B, K, self.T), 7.0, dtype=torch.float64, device="cuda")
        win = torch.full((self.B, K, self.T), -9, dtype=torch.int32, device="cuda") if winners else None
        st = torch.full((self.B,), 9, dtype=torch.uint8, device="cuda")
        if work_bytes is None:
            work_bytes = engine.landscape_work_bytes(self.B, self.max_points, K, self.T)[0]
        work = torch.empty(work_bytes, dtype=torch.uint8, device="cuda") if work_bytes else None
        rc = _lib.lib().tlc_landscape(C.c_int32(self.B), _lib.ptr(self.d_offs), _lib.ptr(self.d_pts), C.c_int32(self.T), _lib.ptr(self.d_ts),
                                      C.c_int32(K), C.c_int64(self.max_points), _lib.ptr(out), _lib.ptr(win), _lib.ptr(st), _lib.ptr(work),
                                      C.c_int64(work_bytes), _lib.stream_ptr())
        assert rc == expect, (rc, _lib.lib().tlc_last_error())
        return out.cpu().numpy(), None if win is None else win.cpu().numpy(), st.cpu().numpy()

    def vjp(self, K, winner, gout):
        """-> grad_pts [sum n, 2] as numpy; sentinel 7.0"""
        torch = self.torch
        g = torch.full((max(len(self.pts), 1), 2), 7.0, dtype=torch.float64, device="cuda")
        d_win, d_gout = _dev(torch, winner, torch.int32), _dev(torch, gout, torch.float64)      # (named: they live until the copy back)
        rc = _lib.lib().tlc_landscape_vjp(C.c_int32(self.B), _lib.ptr(self.d_offs), _lib.ptr(self.d_pts), C.c_int32(self.T), _lib.ptr(self.d_ts),
                                          C.c_int32(K), C.c_int64(self.max_points), _lib.ptr(d_win), _lib.ptr(d_gout), _lib.ptr(g),
                                          _lib.stream_ptr())
        assert rc == 0, _lib.lib().tlc_last_error()
        return g.cpu().numpy()[:len(self.pts)]

    def restate(self, K):
        """the restatement of every diagram at K -> (out, winner, status), computed once at KMAX: its first K rows are the K best"""
        if not hasattr(self, "_ref"):
            self._ref = [cases.restate(d, self.ts, KMAX) for d in self.dgms]
        return (np.stack([r[0][:K] for r in self._ref]), np.stack([r[1][:K] for r in self._ref]),
                np.array([r[2] for r in self._ref], dtype=np.uint8))

    def restate_vjp(self, winner, gout):
        return np.concatenate([cases.restate_vjp(d, self.ts, winner[b], gout[b]) for b, d in enumerate(self.dgms)] + [np.zeros((0, 2))])


def check_forward(P, K, got):
    out, win, st = got
    wo, ww, ws = P.restate(K)
    assert np.array_equal(st, ws)
    assert same_bits(out, wo), np.argwhere(bits(out) != bits(wo))[:5]
    assert np.array_equal(win, ww)
    # every cell written; absent cells are +0.0 (the sign bit too) with winner -1
    absent = win == -1
    assert not (bits(out)[absent & (ws[:, None, None] == 0)]).any() and (win >= -1).all()


def check_vjp(P, K, win, seed=0):
    gout = np.random.RandomState(seed).standard_normal(win.shape)
    g = P.vjp(K, win, gout)
    assert same_bits(g, P.restate_vjp(win, gout))
    won = np.zeros(len(P.pts), dtype=bool)
    for b in range(P.B):
        w = win[b][win[b] >= 0]
        won[P.offs[b] + w] = True
    assert not bits(g[~won]).any()                                # rows of non-winners: exactly +0.0, and written
    return g


# ---- 1. every class, both sides of the cuts, every instantiation ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def class_dgms():
    rs = np.random.RandomState(3)
    return [cases.random_diagram(rs, n) for n in SIZES]


@pytest.mark.parametrize("T", TS)
def test_classes(torch_cuda, class_dgms, T):
    P = Packed(torch_cuda, class_dgms, cases.grid(T))
    for K in KS + (MORE_KS if T == 65 else ()):
        got = P.forward(K)
        check_forward(P, K, got)
        if K in (2, 5) or T == 65:
            check_vjp(P, K, got[1], seed=K)
    # without winners the values are the same
    assert same_bits(P.forward(5, winners=False)[0], P.forward(5)[0])


def test_every_diagram_alone_equals_the_batch(torch_cuda, class_dgms):
    torch = torch_cuda
    T, K = 65, 5
    P = Packed(torch, class_dgms, cases.grid(T))
    out, win, st = P.forward(K)
    again = P.forward(K)
    assert same_bits(out, again[0]) and np.array_equal(win, again[1])          # run == run
    gout = np.random.RandomState(1).standard_normal(win.shape)
    g = P.vjp(K, win, gout)
    assert same_bits(g, P.vjp(K, win, gout))
    for b, d in enumerate(class_dgms):
        A = Packed(torch, [d], P.ts)
        ao, aw, ast = A.forward(K)
        assert same_bits(ao[0], out[b]) and np.array_equal(aw[0], win[b]) and ast[0] == st[b], b
        assert same_bits(A.vjp(K, aw, gout[b:b + 1]), g[P.offs[b]:P.offs[b + 1]]), b


def test_one_large_diagram(torch_cuda):
    rs = np.random.RandomState(4)
    P = Packed(torch_cuda, [cases.random_diagram(rs, 70000)], cases.grid(64))
    got = P.forward(4)
    check_forward(P, 4, got)
    assert (got[1] >= 0).any() and got[1].max() > 16 * LDS_NMAX              # winners from the last slices too
    check_vjp(P, 4, got[1])


# ---- 2. ties ------------------------------------------------------------------------------------------------------------------------------
def test_ties(torch_cuda):
    rs = np.random.RandomState(5)
    dgms = [cases.integer_diagram(rs, n) for n in (8, 40, 300, LDS_NMAX + 50)]
    dgms += [np.tile([[0.25, 0.75]], (n, 1)) for n in (20, 100, LDS_NMAX + 3)]               # copies of one point
    dgms += [cases.nested(12)]
    P = Packed(torch_cuda, dgms, cases.integer_grid())
    for K in (1, 4, 16):
        got = P.forward(K)
        check_forward(P, K, got)
        check_vjp(P, K, got[1], seed=K)
    out, win, _ = P.forward(16)
    j = int(np.argwhere(P.ts == 0.5)[0, 0])
    for b in (4, 5, 6):                                                          # N copies: winners 0 .. K-1 in order
        assert win[b, :, j].tolist() == list(range(16)) and (out[b, :, j] == 0.25).all()
    # the named rows of integer_diagram: (1, 3) three times and (-0.0, 2) before (0, 2); the point with death == birth, the one with
    # death < birth and (-2, -0.0) at t >= 0 are never present
    jt = int(np.argwhere(P.ts == 2.0)[0, 0])
    assert win[0, :3, jt].tolist() == [0, 1, 7] and (out[0, :3, jt] == 1.0).all()
    j1 = int(np.argwhere(P.ts == 1.0)[0, 0])
    assert win[0, :2, j1].tolist() == [2, 3]
    assert not np.isin(win[0], (5, 6)).any() and not np.isin(win[0][:, P.ts >= 0], 4).any()


# ---- 3. more diagrams than any grid -------------------------------------------------------------------------------------------------------
def test_a_batch_larger_than_the_grid(torch_cuda):
    rs = np.random.RandomState(6)
    B, T, K = 20000, 16, 3
    n = rs.randint(0, 9, size=B)
    n[[7, 9000, 19999]] = (WAVE_NMAX, WAVE_NMAX + 1, 2 * WAVE_NMAX)
    dgms = [cases.random_diagram(rs, k) for k in n]
    P = Packed(torch_cuda, dgms, cases.grid(T))
    out, win, st = P.forward(K)
    assert not st.any() and (win >= -1).all() and not (out == 7.0).any()
    gout = rs.standard_normal(win.shape)
    g = P.vjp(K, win, gout)
    assert not (g == 7.0).any()
    for b in [0, 7, 8191, 8192, 9000, 16384, 19999] + rs.randint(0, B, size=40).tolist():
        wo, ww, _ = cases.restate(dgms[b], P.ts, K)
        assert same_bits(out[b], wo) and np.array_equal(win[b], ww), b
        assert same_bits(g[P.offs[b]:P.offs[b + 1]], cases.restate_vjp(dgms[b], P.ts, ww, gout[b])), b
        ao, aw, _ = Packed(torch_cuda, [dgms[b]], P.ts).forward(K)
        assert same_bits(ao[0], out[b]) and np.array_equal(aw[0], win[b]), b


# ---- 4. the workspace -------------------------------------------------------------------------------------------------------------------
def test_any_workspace_gives_the_same_bits(torch_cuda):
    from tlc_gnn_amd import engine
    rs = np.random.RandomState(7)
    T, K = 70, 5
    dgms = [cases.random_diagram(rs, 9), cases.random_diagram(rs, 5 * LDS_NMAX + 7), cases.random_diagram(rs, LDS_NMAX + 1)]
    P = Packed(torch_cuda, dgms, cases.grid(T))
    full, least = engine.landscape_work_bytes(P.B, P.max_points, K, T)
    assert 0 < least < full
    want = P.forward(K, work_bytes=full)
    check_forward(P, K, want)
    for wb in (least, least + (full - least) // 3, full - 1, 2 * full):
        got = P.forward(K, work_bytes=wb)
        assert same_bits(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), wb
    got = P.forward(K, work_bytes=least - 1, expect=1)                           # refused, nothing written
    assert (got[0] == 7.0).all() and (got[2] == 9).all()


# ---- 5. status 3 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [10, 300, LDS_NMAX + 10])
@pytest.mark.parametrize("poison", [np.nan, np.inf, -np.inf])
def test_a_bad_coordinate_fails_its_diagram_alone(torch_cuda, n, poison):
    rs = np.random.RandomState(8)
    T, K = 65, 3
    dgms = [cases.random_diagram(rs, k) for k in (5, n, 70, LDS_NMAX + 2)]
    clean = Packed(torch_cuda, dgms, cases.grid(T)).forward(K)
    bad = [d.copy() for d in dgms]
    bad[1][n - 1, rs.randint(2)] = poison
    P = Packed(torch_cuda, bad, cases.grid(T))
    out, win, st = P.forward(K)
    assert st.tolist() == [0, 3, 0, 0]
    assert np.isnan(out[1]).all() and (win[1] == -1).all()
    for b in (0, 2, 3):
        assert same_bits(out[b], clean[0][b]) and np.array_equal(win[b], clean[1][b])
    check_forward(P, K, (out, win, st))
    g = check_vjp(P, K, win)
    assert not bits(g[P.offs[1]:P.offs[2]]).any()                                # its gradient is zero
    from tlc_gnn_amd import ops
    with pytest.raises(RuntimeError, match="diagram 1 "):
        ops.landscape(P.d_pts, P.d_offs, P.d_ts, K=K)
    assert ops.landscape(P.d_pts, P.d_offs, P.d_ts, K=K, check=False)["status"].tolist() == [0, 3, 0, 0]


# ---- 6. what only the device can refuse, and the empty batch ---------------------------------------------------------------------------------
def test_refusals_after_the_read_back(torch_cuda):
    torch = torch_cuda
    from tlc_gnn_amd import engine
    rs = np.random.RandomState(9)
    dgms = [cases.random_diagram(rs, k) for k in (5, 9, 3)]
    for bad in (np.nan, np.inf):
        ts = cases.grid(8)
        ts[3] = bad
        P = Packed(torch, dgms, ts)
        got = P.forward(2, expect=1)
        assert b"sample 3" in _lib.lib().tlc_last_error() and (got[0] == 7.0).all() and (got[2] == 9).all()
    P = Packed(torch, dgms, cases.grid(8))
    P.d_offs = _dev(torch, [0, 9, 5, 17], torch.int64)                          # decreasing
    P.forward(2, expect=1)
    assert b"decrease" in _lib.lib().tlc_last_error()
    P = Packed(torch, dgms, cases.grid(8))
    P.max_points = 8                                                            # a diagram above max_points
    P.forward(2, expect=1)
    assert b"max_points" in _lib.lib().tlc_last_error()
    with pytest.raises(_lib.TlcError):
        engine.landscape_vjp(P.d_pts, P.d_offs, _dev(torch, [0.0, np.nan], torch.float64), 1, torch.zeros((3, 1, 2), dtype=torch.int32, device="cuda"),
                             torch.zeros((3, 1, 2), dtype=torch.float64, device="cuda"))
    # no diagram
    out, win, st = engine.landscape(torch.zeros((0, 2), dtype=torch.float64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"), P.d_ts, 3)
    assert out.shape == (0, 3, 8) and win.shape == (0, 3, 8) and st.shape == (0,)
    assert engine.landscape_vjp(torch.zeros((0, 2), dtype=torch.float64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"), P.d_ts, 3,
                                win, out).shape == (0, 2)


# ---- 7. autograd --------------------------------------------------------------------------------------------------------------------------
def test_gradcheck(torch_cuda):
    from tlc_gnn_amd import autograd
    torch = torch_cuda
    dgms, ts, draws = cases.gradcheck_input()
    assert draws <= 100
    offs, pts = cases.pack(dgms)
    d_pts = _dev(torch, pts, torch.float64).requires_grad_(True)
    d_offs, d_ts = _dev(torch, offs, torch.int64), _dev(torch, ts, torch.float64)
    fn = lambda p: autograd.diagram_landscape(p, d_offs, d_ts, K=3)
    out = fn(d_pts)
    assert out.shape == (2, 3, 4) and out.requires_grad and float(out.abs().sum()) > 0
    assert torch.autograd.gradcheck(fn, (d_pts,))                               # the fp64 defaults: eps 1e-6, atol 1e-5, rtol 1e-3
    f32 = autograd.diagram_landscape(d_pts.detach().float().requires_grad_(True), d_offs, d_ts, K=3)
    assert f32.dtype == torch.float32
    one = autograd.diagram_landscape(d_pts[:4], ts=d_ts, K=3)                   # offs=None: one diagram
    assert torch.equal(one[0], out[0])


@pytest.fixture(scope="module")
def graphs(torch_cuda):
    import pd_grad_cases as pg
    torch = torch_cuda
    rs = np.random.RandomState(21)
    gs = [(n, pg.small_graph(rs, n)) for n in (5, 9, 16, 12)] + [(70, pg.chord_graph(rs, 70, 120)), (300, pg.chord_graph(rs, 300, 700))]
    no, eo, E, f = pg.pack(gs, [pg.distinct_values(rs, n) for n, _ in gs])
    return dict(no=_dev(torch, no, torch.int64), eo=_dev(torch, eo, torch.int64), E=_dev(torch, E, torch.int32), f=_dev(torch, f, torch.float64),
                B=len(gs), lo=float(f.min()), hi=float(f.max()))


@pytest.mark.parametrize("which", ["ord0+ext1", "ord0", "ext1", "ord0+ext0+ext1"])
def test_topo_landscapes(torch_cuda, graphs, which):
    from tlc_gnn_amd import topo
    torch, g = torch_cuda, graphs
    K, ts = 4, np.linspace(g["lo"], g["hi"], 33)
    d_ts = _dev(torch, ts, torch.float64)
    f = g["f"].clone().requires_grad_(True)
    out = topo.landscapes(f, g["no"], g["eo"], g["E"], d_ts, K=K, which=which)
    assert out.shape == (g["B"], K, 33) and out.dtype == torch.float64 and float(out.max()) > 0
    gout = torch.as_tensor(np.random.RandomState(2).standard_normal(out.shape)).cuda()
    out.backward(gout)
    assert float(f.grad.abs().max()) > 0
    # the restatement on the diagrams' points, and its gradient pushed through pd_grad's selection
    f2 = g["f"].clone().requires_grad_(True)
    pts, offs = topo._select(f2, g["no"], g["eo"], g["E"], which, "host")
    P, po = pts.detach().cpu().numpy(), offs.cpu().numpy()
    gp = np.zeros_like(P)
    for b in range(g["B"]):
        d = P[po[b]:po[b + 1]]
        wo, ww, ws = cases.restate(d, ts, K)
        assert ws == 0 and same_bits(out[b].detach().cpu().numpy(), wo), b
        gp[po[b]:po[b + 1]] = cases.restate_vjp(d, ts, ww, gout[b].cpu().numpy())
    pts.backward(_dev(torch, gp, torch.float64))
    assert torch.equal(f.grad, f2.grad)
    # float32 values: the float64 result of the same (float32-valued) points, rounded once
    f32 = g["f"].float()
    o32 = topo.landscapes(f32.clone().requires_grad_(True), g["no"], g["eo"], g["E"], d_ts, K=K, which=which)
    o64 = topo.landscapes(f32.double(), g["no"], g["eo"], g["E"], d_ts, K=K, which=which)
    assert o32.dtype == torch.float32 and o32.requires_grad and torch.equal(o32.detach(), o64.float())


def test_training_smoke(torch_cuda):
    """64 small random graphs; f a free parameter started at a perturbation of the hidden values; 200 Adam steps on the MSE to the
    hidden values' landscapes.  The loss stays finite and ends below where it began (the ratio reached is in DESIGN.md 6.16)."""
    import pd_grad_cases as pg
    from tlc_gnn_amd import topo
    torch = torch_cuda
    rs = np.random.RandomState(31)
    gs = [(n, pg.small_graph(rs, n)) for n in rs.randint(6, 20, size=64)]
    no, eo, E, hidden = pg.pack(gs, [pg.distinct_values(rs, n) for n, _ in gs])
    no, eo, E = _dev(torch, no, torch.int64), _dev(torch, eo, torch.int64), _dev(torch, E, torch.int32)
    ts = _dev(torch, np.linspace(hidden.min(), hidden.max(), 50), torch.float64)
    target = topo.landscapes(_dev(torch, hidden, torch.float64), no, eo, E, ts, K=5)
    f = _dev(torch, hidden + 0.1 * (hidden.max() - hidden.min()) * rs.standard_normal(len(hidden)), torch.float64).requires_grad_(True)
    opt = torch.optim.Adam([f], lr=0.01 * float(hidden.max() - hidden.min()))
    losses = []
    for _ in range(200):
        opt.zero_grad()
        loss = ((topo.landscapes(f, no, eo, E, ts, K=5) - target) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss))
    print("landscape training: first %.6e last %.6e ratio %.4f" % (losses[0], losses[-1], losses[-1] / losses[0]))
    assert np.isfinite(losses).all() and losses[-1] < losses[0]

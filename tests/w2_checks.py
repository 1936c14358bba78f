"""What the GPU tests of the matching Wasserstein loss share (tests/test_gpu_w2_large.py, tests/test_gpu_w2_classes.py): packing a batch,
one problem's outputs against scipy's assignment solver and the restated loss (oracle/w2_ref.py), and the C entries of csrc/w2_match.hip
called on a sub-range of a batch into sentinel-filled outputs.  torch is handed in: importing this module needs no GPU."""
import ctypes as C

import numpy as np

from matching_class_cases import pair as _pair                        # noqa: F401  (the clouds, shared with the CPU tests)


def _pack(torch, xs, ys):
    xoff = np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int64)
    yoff = np.concatenate([[0], np.cumsum([len(y) for y in ys])]).astype(np.int64)
    X = np.concatenate(list(xs) + [np.zeros((0, 2))]).reshape(-1, 2)
    Y = np.concatenate(list(ys) + [np.zeros((0, 2))]).reshape(-1, 2)
    return xoff, yoff, torch.as_tensor(xoff).cuda(), torch.as_tensor(X).cuda(), torch.as_tensor(yoff).cuda(), torch.as_tensor(Y).cuda()


def _host(r):
    return {k: (None if v is None else v.cpu().numpy()) for k, v in r.items() if k != "work"}


def _check_training(torch, Xb, Yb, order, a, loss, wxy, wxd, grad, ref_cost, unique=True):
    from oracle import w2_ref
    n, m = len(Xb), len(Yb)
    # a valid partial matching: every target exactly once, the rest on the diagonal
    assert sorted(a[a >= 0].tolist()) == list(range(m)) and (a >= -1).all() and (a < max(m, 1)).all()
    M = w2_ref.cost_matrix(Xb, Yb, order)
    cost = float(M[np.arange(n), np.where(a >= 0, a, m)].sum())
    print("training n=%d m=%d order=%d: cost %.17g scipy %.17g" % (n, m, order, cost, ref_cost))
    assert abs(cost - ref_cost) <= 1e-9 * max(1.0, abs(ref_cost)), (n, m, cost, ref_cost)
    if not unique:
        return
    l2, wxy2, wxd2 = w2_ref.loss_from_assignment(Xb, Yb, a, order)
    assert abs(loss - l2) <= 1e-12 * max(1.0, l2) and abs(wxy - wxy2) <= 1e-12 * max(1.0, wxy2) and abs(wxd - wxd2) <= 1e-12 * max(1.0, wxd2)
    if n:
        Xt = torch.tensor(Xb, requires_grad=True)
        w2_ref.loss_torch(Xt, torch.tensor(Yb), a, order).backward()
        assert np.abs(grad - Xt.grad.numpy()).max() <= 1e-12


def _check_inference(torch, Xb, Yb, order, ax, ay, loss, wxy, wxd, wyd, grad, ref, unique=True):
    from oracle import w2_ref
    n, m = len(Xb), len(Yb)
    if n == 0 or m == 0:
        # (:98-113) total persistence of the other diagram, the parts reported as 0, nothing matched
        assert abs(loss - ref[0]) <= 1e-12 * max(1.0, ref[0]) and wxy == 0 and wxd == 0 and wyd == 0
        assert (ax == -1).all() and (ay == -1).all()
        if n:
            d = (Xb[:, 1] - Xb[:, 0]) * 0.5
            want = np.stack([-0.5 * d / loss, 0.5 * d / loss], 1) if order == 2 else np.stack([-0.5 * np.sign(d), 0.5 * np.sign(d)], 1)
            assert np.abs(grad - want).max() <= 1e-12
        return
    on = ax >= 0
    # the two maps are each other's inverse on the matched points
    assert (ax < m).all() and (ax >= -1).all() and (ay < n).all() and (ay >= -1).all()
    assert (ay[ax[on]] == np.flatnonzero(on)).all() and (ay >= 0).sum() == on.sum()
    C = w2_ref.inference_cost_matrix(Xb, Yb, order)
    cost = float(C[np.flatnonzero(on), ax[on]].sum() + C[np.flatnonzero(~on), m].sum() + C[n, np.flatnonzero(ay < 0)].sum())
    print("evaluation n=%d m=%d order=%d: cost %.17g scipy %.17g" % (n, m, order, cost, ref[6]))
    assert abs(cost - ref[6]) <= 1e-9 * max(1.0, abs(ref[6])), (n, m, cost, ref[6])
    if not unique:
        return
    for got, want in zip((loss, wxy, wxd, wyd), w2_ref.inference_loss_from_assignment(Xb, Yb, ax, ay, order)):
        assert abs(got - want) <= 1e-12 * max(1.0, want)
    Xt = torch.tensor(Xb, requires_grad=True)
    Yt = torch.tensor(Yb)
    parts = []
    if on.any():
        parts.append((Yt[torch.as_tensor(ax[on]).long()] - Xt[torch.as_tensor(on)]).abs().amax(dim=1))
    if (~on).any():
        q = Xt[torch.as_tensor(~on)]
        parts.append(((q[:, 1] - q[:, 0]) * 0.5).abs())
    if (ay < 0).any():
        q = Yt[torch.as_tensor(ay < 0)]
        parts.append(((q[:, 1] - q[:, 0]) * 0.5).abs())
    ((torch.cat(parts) ** order).sum() ** (1.0 / order)).backward()
    assert np.abs(grad - Xt.grad.numpy()).max() <= 1e-12


# ---- one form's call and check, for the tests that run both -----------------------------------------------------------------------------
def solve(torch, problems, infer, order, max_points):
    """ops.w2_partial_matching / ops.w2_inference_matching on a list of (X, Y) with an explicit max_points -> (xoff, yoff, host outputs;
    the training form's `assign` under the key assign_x)"""
    from tlc_gnn_amd import ops
    xoff, yoff, dxo, dX, dyo, dY = _pack(torch, [p[0] for p in problems], [p[1] for p in problems])
    fn = ops.w2_inference_matching if infer else ops.w2_partial_matching
    h = _host(fn(dxo, dX, dyo, dY, order=order, want_grad=True, max_points=max_points))
    if not infer:
        h["assign_x"] = h.pop("assign")
    for v in h.values():
        v.setflags(write=False)
    return xoff, yoff, h


def check_problem(torch, problem, infer, order, h, xoff, yoff, b, unique=True):
    """problem b of a solved batch through _check_training / _check_inference, scipy's optimum computed here"""
    from oracle import w2_ref
    Xb, Yb = problem
    sx, sy = slice(xoff[b], xoff[b + 1]), slice(yoff[b], yoff[b + 1])
    assert h["status"][b] == 0, (b, len(Xb), len(Yb), h["status"][b])
    if infer:
        _check_inference(torch, Xb, Yb, order, h["assign_x"][sx], h["assign_y"][sy], h["loss"][b], h["wxy"][b], h["wxd"][b], h["wyd"][b],
                         h["grad"][sx], w2_ref.inference_matching(Xb, Yb, order), unique=unique)
    else:
        _check_training(torch, Xb, Yb, order, h["assign_x"][sx], h["loss"][b], h["wxy"][b], h["wxd"][b], h["grad"][sx],
                        w2_ref.partial_matching(Xb, Yb, order)[4], unique=unique)


def check_refused(h, infer, xoff, yoff, b, code):
    """what w2_fail is documented to write: the status, loss 0 (NaN for status 3), zero parts, no matching, a zero gradient"""
    sx, sy = slice(xoff[b], xoff[b + 1]), slice(yoff[b], yoff[b + 1])
    assert h["status"][b] == code, (b, h["status"][b], code)
    assert np.isnan(h["loss"][b]) if code == 3 else h["loss"][b] == 0.0, (b, h["loss"][b])
    assert h["wxy"][b] == 0.0 and h["wxd"][b] == 0.0 and (not infer or h["wyd"][b] == 0.0), b
    assert (h["assign_x"][sx] == -1).all() and (h["grad"][sx] == 0.0).all(), b
    if infer:
        assert (h["assign_y"][sy] == -1).all(), b


# ---- the C entries on a sub-range of a batch, into outputs nobody pre-filled with the answer -----------------------------------------------
DOUBLE_SENTINEL, INT_SENTINEL, STATUS_SENTINEL = -7.0, -7, 77


def _raw_outputs(torch, infer, B, nx, ny):
    f64 = lambda *shape: torch.full(shape, DOUBLE_SENTINEL, dtype=torch.float64, device="cuda")
    i32 = lambda *shape: torch.full(shape, INT_SENTINEL, dtype=torch.int32, device="cuda")
    o = dict(loss=f64(B), wxy=f64(B), wxd=f64(B), assign_x=i32(max(nx, 1)), grad=f64(max(nx, 1), 2),
             status=torch.full((B,), STATUS_SENTINEL, dtype=torch.uint8, device="cuda"))
    if infer:
        o.update(wyd=f64(B), assign_y=i32(max(ny, 1)))
    return o


def _raw_call(o, infer, dxo, dX, dyo, dY, first, count, order, max_points):
    """tlc_w2_partial_matching / tlc_w2_inference_matching on problems first .. first + count of the packed batch, writing into the
    batch's own output rows"""
    from tlc_gnn_amd import _lib
    at = lambda t, k: C.c_void_p(t.data_ptr() + k * t.element_size())
    head = (C.c_int32(count), at(dxo, first), _lib.ptr(dX), at(dyo, first), _lib.ptr(dY), C.c_int(order), C.c_int32(max_points),
            at(o["loss"], first), at(o["wxy"], first), at(o["wxd"], first))
    if infer:
        rc = _lib.lib().tlc_w2_inference_matching(*head, at(o["wyd"], first), _lib.ptr(o["assign_x"]), _lib.ptr(o["assign_y"]), _lib.ptr(o["grad"]),
                                                  at(o["status"], first), _lib.stream_ptr())
    else:
        rc = _lib.lib().tlc_w2_partial_matching(*head, _lib.ptr(o["assign_x"]), _lib.ptr(o["grad"]), at(o["status"], first), _lib.stream_ptr())
    assert rc == 0, _lib.lib().tlc_last_error()


def same_bits(torch, a, b):
    """torch.equal on the bit patterns: a NaN loss (status 3) equals itself"""
    if a.dtype == torch.float64:
        a, b = a.view(torch.int64), b.view(torch.int64)
    return torch.equal(a, b)

"""Shared by tests/test_gpu_dgm_gram.py and tests/test_cpu_dgm_gram_host.py: numpy restatements of the diagram kernels of
include/tlcgnn.h ("Gram matrices of persistence diagram kernels") -- the function and its gradient in np.longdouble, with the sums of
absolute values that the error bound of DESIGN.md 6.17 is made of, and the documented summation order in fp64 -- and the generators of
the test inputs."""
import math

import numpy as np

LD = np.longdouble
SLICE, GROUP, CHUNK = 1024, 1024, 64            # TLC_DG_SLICE, TLC_DG_GROUP and the 64 lanes (the host test checks them against the header)
ALL, PAIRED, SYMMETRIC, MIRROR = 1, 2, 4, 8     # TLC_DG_*
U = 2.0 ** -53
# roundings per summand that are relative to the summand (the library's exp is within 1 ulp = 2 u) ...
C0_VALUE, C0_GRAD_PTS, C0_GRAD_W = 6, 10, 6
# ... and the rounding of the exponential's argument (five roundings, rounded up to six for the second-order terms): its effect
# |a| e^a <= 1 / e per unit of weight is not relative to the summand
C_ARG = 6
TINY = 2.0 ** -1000                             # per summand: results in the subnormal range are absolute errors, not relative ones


def kernel_params(kernel, sigma):
    """ops.dgm_kernel_params, restated"""
    if kernel == "pss":
        return 1.0 / (8.0 * sigma), 1.0 / (8.0 * math.pi * sigma), True
    assert kernel == "gauss"
    return 1.0 / (2.0 * sigma * sigma), 1.0, False


def pack(dgms):
    offs = np.zeros(len(dgms) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(d) for d in dgms])
    pts = np.concatenate([np.asarray(d, dtype=np.float64).reshape(-1, 2) for d in dgms] + [np.zeros((0, 2))])
    return offs, np.ascontiguousarray(pts)


def pack_w(ws):
    return np.ascontiguousarray(np.concatenate([np.asarray(w, dtype=np.float64).reshape(-1) for w in ws] + [np.zeros(0)]))


def random_diagram(rs, n, spread=1.0):
    b = rs.uniform(0.0, spread, n)
    return np.stack([b, b + rs.uniform(0.0, spread, n)], 1)


def random_weights(rs, n):
    """weights of both signs"""
    return rs.uniform(-1.0, 2.0, n)


def slices_of(n):
    return max(1, -(-n // SLICE))


def groups_of(m):
    return max(1, -(-m // GROUP))


def chain(n, m):
    """the longest chain of additions behind one summand of out[i, j] in the documented order"""
    return min(n, SLICE) + 6 + min(-(-m // CHUNK), GROUP // CHUNK) + slices_of(n) * groups_of(m)


def gamma_k(k):
    """(1 + u)^k - 1 <= k u / (1 - k u)"""
    return k * U / (1.0 - k * U)


# ---- the function in longdouble ---------------------------------------------------------------------------------------------------------
def ref_pair(X, wx, Y, wy, gamma, scale, mirror, rows=256):
    """One diagram pair in np.longdouble.  -> dict: k; sig = the sum of the absolute values of k's summands; alp = the same with every
    exponential e^a replaced by |a| e^a; and per point p of X, for an upstream of 1 and before the factors in front of the sums: gb, gd
    = sum_q w_q (-(p - q) e1 + mirror (p - q~) e2), gw = sum_q w_q (e1 - mirror e2), with their sig_* and alp_* likewise."""
    X, Y = np.asarray(X, dtype=LD).reshape(-1, 2), np.asarray(Y, dtype=LD).reshape(-1, 2)
    n, m = len(X), len(Y)
    wx = np.ones(n, dtype=LD) if wx is None else np.asarray(wx, dtype=LD)
    wy = np.ones(m, dtype=LD) if wy is None else np.asarray(wy, dtype=LD)
    g = LD(gamma)
    names = ("gb", "gd", "gw", "sig_b", "sig_d", "sig_w", "alp_b", "alp_d", "alp_w")
    per = {k: np.zeros(n, dtype=LD) for k in names}
    tot = dict(k=[], sig=[], alp=[])
    awy = np.abs(wy)[None, :]
    for r0 in range(0, n, rows):
        xb, xd = X[r0:r0 + rows, 0][:, None], X[r0:r0 + rows, 1][:, None]
        db, dd = xb - Y[None, :, 0], xd - Y[None, :, 1]
        a1 = -g * (db * db + dd * dd)
        e1 = np.exp(a1)
        f1 = np.abs(a1) * e1
        if mirror:
            mb, md = xb - Y[None, :, 1], xd - Y[None, :, 0]
            a2 = -g * (mb * mb + md * md)
            e2 = np.exp(a2)
            f2 = np.abs(a2) * e2
        else:
            mb = md = e2 = f2 = np.zeros((1, 1), dtype=LD)
        s = slice(r0, r0 + rows)
        w = wy[None, :]
        per["gw"][s] = (w * (e1 - e2)).sum(1)
        per["sig_w"][s] = (awy * (e1 + e2)).sum(1)
        per["alp_w"][s] = (awy * (f1 + f2)).sum(1)
        per["gb"][s] = (w * (mb * e2 - db * e1)).sum(1)
        per["gd"][s] = (w * (md * e2 - dd * e1)).sum(1)
        per["sig_b"][s] = (awy * (np.abs(mb) * e2 + np.abs(db) * e1)).sum(1)
        per["sig_d"][s] = (awy * (np.abs(md) * e2 + np.abs(dd) * e1)).sum(1)
        per["alp_b"][s] = (awy * (np.abs(mb) * f2 + np.abs(db) * f1)).sum(1)
        per["alp_d"][s] = (awy * (np.abs(md) * f2 + np.abs(dd) * f1)).sum(1)
        tot["k"].append((wx[s] * per["gw"][s]).sum())
        tot["sig"].append((np.abs(wx[s]) * per["sig_w"][s]).sum())
        tot["alp"].append((np.abs(wx[s]) * per["alp_w"][s]).sum())
    sc = LD(scale)
    out = dict(per)
    out["k"] = sc * (np.sum(np.array(tot["k"], dtype=LD)) if n else LD(0))
    out["sig"] = abs(sc) * (np.sum(np.array(tot["sig"], dtype=LD)) if n else LD(0))
    out["alp"] = abs(sc) * (np.sum(np.array(tot["alp"], dtype=LD)) if n else LD(0))
    out["n"], out["m"] = n, m
    out["wmax"] = float(max(np.abs(wx).max() if n else 0, 1) * max(np.abs(wy).max() if m else 0, 1))
    return out


def value_bound(r, scale):
    """|kernel - r['k']| is at most this: (C0 + L) 2^-53 S with the argument term folded in"""
    n, m = r["n"], r["m"]
    return float(gamma_k(C0_VALUE + chain(n, m)) * r["sig"] + gamma_k(C_ARG) * r["alp"]) + n * m * TINY * r["wmax"] * (abs(scale) + 1)


def ref_grad(pairs, Grow, wx, gamma, scale, ny_chain):
    """The gradient rows of one X diagram from its pairs (ref_pair results, Y's diagrams ascending) and their upstream values Grow ->
    (grad_pts [n, 2], grad_w [n], bound_pts [n, 2], bound_w [n]) in longdouble / float."""
    n = pairs[0]["n"]
    wx = np.ones(n, dtype=LD) if wx is None else np.asarray(wx, dtype=LD)
    acc = {k: np.zeros(n, dtype=LD) for k in ("gb", "gd", "gw", "sig_b", "sig_d", "sig_w", "alp_b", "alp_d", "alp_w")}
    L, cnt = ny_chain, 0
    for r, G in zip(pairs, Grow):
        G = LD(G)
        for k in ("gb", "gd", "gw"):
            acc[k] += G * r[k]
        for k in ("sig_b", "sig_d", "sig_w", "alp_b", "alp_d", "alp_w"):
            acc[k] += abs(G) * r[k]
        L = max(L, ny_chain + r["m"])
        cnt += r["m"]
    wmax = max(p["wmax"] for p in pairs) * (float(np.abs(np.asarray(Grow, dtype=np.float64)).max()) + 1)
    c2 = LD(scale) * wx * LD(2.0 * gamma)
    floor = cnt * TINY * wmax * (abs(scale) + 1) * (2 * gamma + 1)
    gp = np.stack([c2 * acc["gb"], c2 * acc["gd"]], 1)
    bp = np.stack([np.abs(c2) * (gamma_k(C0_GRAD_PTS + L) * acc["sig_" + k] + gamma_k(C_ARG) * acc["alp_" + k]) for k in "bd"], 1)
    gw = LD(scale) * acc["gw"]
    bw = abs(LD(scale)) * (gamma_k(C0_GRAD_W + L) * acc["sig_w"] + gamma_k(C_ARG) * acc["alp_w"])
    return gp, gw, bp.astype(np.float64) + floor, bw.astype(np.float64) + floor


# ---- the documented order in fp64 -----------------------------------------------------------------------------------------------------
def _seq_sum(t):
    """+0.0, then the rows of t in turn (np.add.accumulate is sequential)"""
    return np.add.accumulate(np.concatenate([np.zeros((1,) + t.shape[1:]), t]), axis=0)[-1]


def _summands(X, wx, Y, wy, gamma, mirror):
    """t(p, q) of include/tlcgnn.h in fp64, [n, m]"""
    ng = -gamma
    db, dd = X[:, None, 0] - Y[None, :, 0], X[:, None, 1] - Y[None, :, 1]
    e = np.exp(ng * (db * db + dd * dd))
    if mirror:
        mb, md = X[:, None, 0] - Y[None, :, 1], X[:, None, 1] - Y[None, :, 0]
        e = e - np.exp(ng * (mb * mb + md * md))
    if wx is None and wy is None:
        return e
    wx = np.ones(len(X)) if wx is None else wx
    wy = np.ones(len(Y)) if wy is None else wy
    return (wx[:, None] * wy[None, :]) * e


def restate_pair(X, wx, Y, wy, gamma, scale, mirror):
    """out[i, j] of one pair in the documented order, in fp64 with numpy's exp (so: the order, not the device's bits)"""
    X, Y = np.asarray(X, dtype=np.float64).reshape(-1, 2), np.asarray(Y, dtype=np.float64).reshape(-1, 2)
    n, m = len(X), len(Y)
    if n == 0 or m == 0:
        return 0.0
    if not (np.isfinite(X).all() and np.isfinite(Y).all() and (wx is None or np.isfinite(wx).all()) and (wy is None or np.isfinite(wy).all())):
        return np.nan
    t = _summands(X, wx, Y, wy, gamma, mirror)
    R = 0.0
    for s in range(slices_of(n)):
        for g in range(groups_of(m)):
            P = 0.0
            for c0 in range(g * GROUP, min(m, (g + 1) * GROUP), CHUNK):
                a = np.zeros(CHUNK)
                blk = t[s * SLICE:(s + 1) * SLICE, c0:min(c0 + CHUNK, (g + 1) * GROUP)]
                a[:blk.shape[1]] = _seq_sum(blk)
                d = 32
                while d >= 1:
                    a[:d] = a[:d] + a[d:2 * d]
                    d //= 2
                P = P + a[0]
            R = R + P
    return scale * R


def restate_gram(dX, wX, dY, wY, gamma, scale, mirror, paired=False):
    if paired:
        return np.array([restate_pair(dX[i], None if wX is None else wX[i], dY[i], None if wY is None else wY[i], gamma, scale, mirror)
                         for i in range(len(dX))])
    return np.array([[restate_pair(dX[i], None if wX is None else wX[i], dY[j], None if wY is None else wY[j], gamma, scale, mirror)
                      for j in range(len(dY))] for i in range(len(dX))]).reshape(len(dX), len(dY))


def brute_pair(X, wx, Y, wy, gamma, scale, mirror):
    """the same value by plain Python loops over the documented order (diagrams of a few points: one slice, one group, one chunk)"""
    n, m = len(X), len(Y)
    assert n <= SLICE and m <= CHUNK
    if n == 0 or m == 0:
        return 0.0
    ng = -gamma
    a = [0.0] * CHUNK
    for l in range(m):
        for p in range(n):
            db, dd = X[p][0] - Y[l][0], X[p][1] - Y[l][1]
            e = np.exp(ng * (db * db + dd * dd))
            if mirror:
                mb, md = X[p][0] - Y[l][1], X[p][1] - Y[l][0]
                e = e - np.exp(ng * (mb * mb + md * md))
            t = e if wx is None and wy is None else ((1.0 if wx is None else wx[p]) * (1.0 if wy is None else wy[l])) * e
            a[l] = a[l] + t
    d = 32
    while d >= 1:
        for l in range(d):
            a[l] = a[l] + a[l + d]
        d //= 2
    return scale * (0.0 + (0.0 + a[0]))


def restate_grad_rows(X, wx, dY, wY, Grow, gamma, scale, mirror):
    """the gradient rows of one X diagram (weights wx or None) against the diagrams dY (weights wY: a list, or None) in the documented
    order, fp64 with numpy's exp -> (grad_pts [n, 2], grad_w [n])"""
    X = np.asarray(X, dtype=np.float64).reshape(-1, 2)
    n, ng = len(X), -gamma
    gb, gd, gw = np.zeros(n), np.zeros(n), np.zeros(n)
    for j, Y in enumerate(dY):
        Y = np.asarray(Y, dtype=np.float64).reshape(-1, 2)
        db, dd = X[:, None, 0] - Y[None, :, 0], X[:, None, 1] - Y[None, :, 1]
        t1 = np.exp(ng * (db * db + dd * dd))
        if wx is not None or wY is not None:
            wq = np.ones(len(Y)) if wY is None else wY[j]
            t1 = wq[None, :] * t1
        if mirror:
            mb, md = X[:, None, 0] - Y[None, :, 1], X[:, None, 1] - Y[None, :, 0]
            t2 = np.exp(ng * (mb * mb + md * md))
            if wx is not None or wY is not None:
                t2 = wq[None, :] * t2
            ib, idd, iw = _seq_sum((mb * t2 - db * t1).T), _seq_sum((md * t2 - dd * t1).T), _seq_sum((t1 - t2).T)
        else:
            ib, idd, iw = _seq_sum((-(db * t1)).T), _seq_sum((-(dd * t1)).T), _seq_sum(t1.T)
        gb, gd, gw = gb + Grow[j] * ib, gd + Grow[j] * idd, gw + Grow[j] * iw
    c = scale if wx is None and wY is None else scale * (np.ones(n) if wx is None else wx)
    c2 = c * (2.0 * gamma)
    return np.stack([c2 * gb, c2 * gd], 1), scale * gw


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
CUT_SIZES = (0, 1, 63, 64, 65, SLICE - 1, SLICE, SLICE + 1)


def pd_batch(rs, count=48, most=69):
    return [random_diagram(rs, int(rs.randint(0, most + 1))) for _ in range(count)]


def molecules(rs, count, lo=4, hi=40):
    """diagrams the size of a molecule graph's (a few dozen points)"""
    return [random_diagram(rs, int(k)) for k in rs.randint(lo, hi + 1, count)]

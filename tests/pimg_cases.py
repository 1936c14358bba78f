"""Shared by tests/test_cpu_pimg_host.py, tests/test_gpu_pimg.py and tests/golden/make_golden_pimg.py: a numpy / scipy restatement of the
general persistence imager written from its mathematics (include/tlcgnn.h, "The general persistence imager"), the tolerance of the
issue, and the builders of the golden cases.  Nothing here touches a device.

The image is [birth_bin, pers_bin].  Separable sigma: sum_i w_i outer(dPhi_b(i), dPhi_p(i)) with Phi = erfc(-z / sqrt 2) / 2.
Correlated sigma: the bivariate normal CDF at the grid corners as  Phi Phi + asin(r) / (4 pi) * Gauss-Legendre sum over the
correlation (Drezner-Wesolowsky), differenced over the four corners of a pixel per point, then summed over the points."""
import numpy as np
from scipy.special import erfc

EPS = np.finfo(np.float64).eps
MAX_RES, SLICE, CHUNK, GROUP = 128, 1024, 32, 32          # TLC_PI_MAX_RES; _lib.PI_SLICE / PI_CHUNK / PI_GROUP (the CPU test compares them)


def phi(z):
    return erfc(-np.asarray(z, dtype=np.float64) / np.sqrt(2.0)) / 2.0


def ramp(pers, low=0.0, high=1.0, start=0.0, end=1.0):
    pers = np.asarray(pers, dtype=np.float64)
    return np.where(pers < start, low, np.where(pers > end, high, (pers - start) * (high - low) / (end - start) + low))


def n_nodes(r):
    return 6 if abs(r) < 0.3 else (12 if abs(r) < 0.75 else 20)


def bvn(zb, zp, r):
    """P(X <= zb, Y <= zp) of the standard bivariate normal with correlation r, |r| < 0.925"""
    zb, zp = np.asarray(zb, dtype=np.float64), np.asarray(zp, dtype=np.float64)
    x, w = np.polynomial.legendre.leggauss(n_nodes(r))
    asr = np.arcsin(r)
    hk, hs = zb * zp, (zb * zb + zp * zp) / 2.0
    acc = np.zeros(np.broadcast(zb, zp).shape)
    for xj, wj in zip(x, w):
        sn = np.sin(asr * (1.0 + xj) / 2.0)
        acc = acc + wj * np.exp((sn * hk - hs) / (1.0 - sn * sn))
    return phi(zb) * phi(zp) + asr * acc / (4.0 * np.pi)


def coords(pts, skew):
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 2)
    return pts[:, 0], (pts[:, 1] - pts[:, 0]) if skew else pts[:, 1]


def image(pts, bpnts, ppnts, ramp_params=(0.0, 1.0, 0.0, 1.0), sigma=(1.0, 1.0, 0.0), skew=True, weights=None):
    """-> (image [Rb, Rp], sum_i |w_i|)"""
    b, x = coords(pts, skew)
    w = ramp(x, *ramp_params) if weights is None else np.asarray(weights, dtype=np.float64)
    vb, vp, cov = sigma
    zb = (np.asarray(bpnts)[None, :] - b[:, None]) / np.sqrt(vb)          # [n, Rb + 1]
    zp = (np.asarray(ppnts)[None, :] - x[:, None]) / np.sqrt(vp)          # [n, Rp + 1]
    img = np.zeros((len(bpnts) - 1, len(ppnts) - 1))
    if cov == 0.0:
        db, dp = np.diff(phi(zb), axis=1), np.diff(phi(zp), axis=1)
        for i in range(len(b)):
            img += w[i] * np.outer(db[i], dp[i])
    else:
        r = cov / np.sqrt(vb * vp)
        for i in range(len(b)):
            F = bvn(zb[i][:, None], zp[i][None, :], r)
            img += w[i] * (F[1:, 1:] - F[:-1, 1:] - F[1:, :-1] + F[:-1, :-1])
    return img, float(np.sum(np.abs(w)))


def bound(n, wsum, correlated=False):
    """the issue's per-pixel bound: (64 + n) eps sum |w| (+ 1e-300) for the separable path, (256 + n) eps sum |w| for the correlated"""
    return ((256 if correlated else 64) + n) * EPS * wsum + 1e-300


def worst_ratio(dev, ref, n, wsum, correlated=False):
    return float(np.max(np.abs(np.asarray(dev) - ref)) / bound(n, wsum, correlated)) if np.size(ref) else 0.0


def default_lines(res):
    return np.linspace(0.0, 1.0 + 1.0 / res, res + 1, endpoint=False, dtype=np.float64)


def lines(lo, hi, res):
    """res pixels over [lo, hi] as the imager's mesh makes them"""
    pix = (hi - lo) / res
    return np.linspace(lo, hi + pix, res + 1, endpoint=False, dtype=np.float64)


def diagram(n, seed, lo=0.0, hi=1.0):
    """n (birth, death) points with birth in [lo, hi) and persistence in [0, hi - lo) -- inside the unit-like window of the grids"""
    rs = np.random.RandomState(seed)
    b = lo + (hi - lo) * 0.6 * rs.rand(n)
    p = (hi - lo) * 0.9 * rs.rand(n)
    return np.stack([b, b + p], 1)


def pack(dgms):
    offs = np.concatenate([[0], np.cumsum([len(d) for d in dgms])]).astype(np.int64)
    pts = np.concatenate([np.asarray(d, dtype=np.float64).reshape(-1, 2) for d in dgms]) if len(dgms) else np.zeros((0, 2))
    return offs, np.ascontiguousarray(pts)


# ---- the refusals of the C ABI: (what the message must say, bpnts, ppnts, ramp, sigma) -------------------------------------------------
def refusal_specs():
    ok, r95 = default_lines(5), 0.95 * np.sqrt(0.02 * 0.03)
    flat, back = ok.copy(), ok.copy()
    flat[3] = flat[2]
    back[4] = back[2] - 0.01
    nanl = ok.copy()
    nanl[1] = np.nan
    good_ramp, good_sig = (0.0, 1.0, 0.0, 1.0), (1.0, 1.0, 0.0)
    return [
        ("strictly increasing", flat, ok, good_ramp, good_sig),
        ("strictly increasing", ok, back, good_ramp, good_sig),
        ("not finite", nanl, ok, good_ramp, good_sig),
        ("TLC_PI_MAX_RES", np.arange(MAX_RES + 2, dtype=np.float64), ok, good_ramp, good_sig),
        ("TLC_PI_MAX_RES", ok, np.zeros(1), good_ramp, good_sig),
        ("end > start", ok, ok, (0.0, 1.0, 0.5, 0.5), good_sig),
        ("end > start", ok, ok, (0.0, 1.0, 0.5, 0.25), good_sig),
        ("ramp", ok, ok, (0.0, np.inf, 0.0, 1.0), good_sig),
        ("ramp", ok, ok, (np.nan, 1.0, 0.0, 1.0), good_sig),
        ("sigma is not finite", ok, ok, good_ramp, (np.nan, 1.0, 0.0)),
        ("positive definite", ok, ok, good_ramp, (0.0, 1.0, 0.0)),
        ("positive definite", ok, ok, good_ramp, (1.0, -1.0, 0.0)),
        ("positive definite", ok, ok, good_ramp, (1.0, 1.0, 1.0)),
        ("positive definite", ok, ok, good_ramp, (1.0, 1.0, 2.0)),
        ("0.925", ok, ok, good_ramp, (0.02, 0.03, r95)),
        ("0.925", ok, ok, good_ramp, (0.02, 0.03, -r95)),
    ]


# ---- the golden cases (tests/golden/make_golden_pimg.py runs the reference on them; the tests run the drop-in) -------------------------
# grid state machines: a constructor and a sequence of (attribute, value) / ("fit", seed) steps
GRID_CASES = {
    "default5": (dict(resolution=5), []),
    "setters_rect": (dict(resolution=5), [("pixel_size", 0.1), ("birth_range", (0.0, 2.0))]),
    "setters_pad": (dict(resolution=4), [("pixel_size", 0.3), ("pers_range", (0.1, 1.45)), ("birth_range", (-0.2, 0.9))]),
    "setters_order": (dict(resolution=6), [("birth_range", (0.0, 3.0)), ("pixel_size", 0.25), ("pers_range", (0.0, 0.7))]),
    "unequal_ctor": (dict(birth_range=(0.0, 2.0), pers_range=(0.0, 1.0), resolution=5), []),
    "unequal_ctor_pix": (dict(birth_range=(-1.0, 0.5), pers_range=(0.0, 3.0), pixel_size=0.2, resolution=7), []),
    "fit_default_pixel": (dict(resolution=5), [("fit", 11)]),
    "fit_small_pixel": (dict(resolution=5), [("pixel_size", 0.05), ("fit", 12)]),
    "fit_noskew": (dict(resolution=5), [("pixel_size", 0.07), ("fit_noskew", 13)]),
}


def fit_diagrams(seed):
    rs = np.random.RandomState(seed)
    return [diagram(int(rs.randint(3, 30)), int(rs.randint(1 << 30)), lo=0.1, hi=0.9) for _ in range(4)]


def apply_grid_steps(imager, steps):
    for name, val in steps:
        if name == "fit":
            imager.fit(fit_diagrams(val))
        elif name == "fit_noskew":
            imager.fit(fit_diagrams(val), skew=False)
        else:
            setattr(imager, name, val)
    return imager


# images: constructor kwargs, setter steps, diagram, skew, and whether the reference's output is the transpose of [birth_bin, pers_bin]
def _sig(vb, vp, cov=0.0):
    return np.array([[vb, cov], [cov, vp]])


IMAGE_CASES = {
    "iso_20": dict(ctor=dict(resolution=20, kernel_params={"sigma": 0.01}), steps=[], n=40, seed=1, skew=True, transposed=False),
    "iso_rect_20x10": dict(ctor=dict(resolution=5, kernel_params={"sigma": 0.01}), steps=[("pixel_size", 0.1), ("birth_range", (0.0, 2.0))],
                           n=40, seed=2, skew=True, transposed=False),
    "iso_noskew": dict(ctor=dict(resolution=12, kernel_params={"sigma": 0.02}), steps=[], n=30, seed=3, skew=False, transposed=False),
    "iso_ramp": dict(ctor=dict(resolution=10, kernel_params={"sigma": 0.01}, weight_params=dict(low=0.25, high=2.0, start=0.2, end=0.6)),
                     steps=[], n=40, seed=4, skew=True, transposed=False),
    "diag_8": dict(ctor=dict(resolution=8, kernel_params={"sigma": _sig(0.01, 0.04)}), steps=[], n=40, seed=5, skew=True, transposed=True),
    "corr_p02": dict(ctor=dict(resolution=8, kernel_params={"sigma": _sig(0.02, 0.03, 0.2 * np.sqrt(0.02 * 0.03))}), steps=[], n=24, seed=6,
                     skew=True, transposed=True),
    "corr_p05": dict(ctor=dict(resolution=8, kernel_params={"sigma": _sig(0.02, 0.03, 0.5 * np.sqrt(0.02 * 0.03))}), steps=[], n=24, seed=7,
                     skew=True, transposed=True),
    "corr_p08": dict(ctor=dict(resolution=8, kernel_params={"sigma": _sig(0.02, 0.03, 0.8 * np.sqrt(0.02 * 0.03))}), steps=[], n=24, seed=8,
                     skew=True, transposed=True),
    "corr_m05": dict(ctor=dict(resolution=8, kernel_params={"sigma": _sig(0.02, 0.03, -0.5 * np.sqrt(0.02 * 0.03))}), steps=[], n=24, seed=9,
                     skew=True, transposed=True),
}


def case_inputs(name):
    c = IMAGE_CASES[name]
    d = diagram(c["n"], c["seed"])
    if not c["skew"]:
        d = np.stack([d[:, 0], d[:, 1] - d[:, 0]], 1)                   # rows are (birth, persistence)
    return c, d


def case_ctor(c):
    """fresh constructor arguments (the reference writes 'mu' into kernel_params)"""
    k = dict(c["ctor"])
    if "kernel_params" in k:
        k["kernel_params"] = dict(k["kernel_params"])
    if "weight_params" in k:
        k["weight_params"] = dict(k["weight_params"])
    return k


def case_spec(imager, c):
    """(bpnts, ppnts, ramp, sigma, skew) of an imager (reference or drop-in) for `image`"""
    wp = dict(low=0.0, high=1.0, start=0.0, end=1.0)
    wp.update(imager.weight_params)
    s = np.asarray(imager.kernel_params["sigma"], dtype=np.float64)
    sig = (float(s), float(s), 0.0) if s.ndim == 0 else (float(s[0, 0]), float(s[1, 1]), float(s[0, 1]))
    return (np.asarray(imager._bpnts, dtype=np.float64), np.asarray(imager._ppnts, dtype=np.float64),
            (wp["low"], wp["high"], wp["start"], wp["end"]), sig, c["skew"])

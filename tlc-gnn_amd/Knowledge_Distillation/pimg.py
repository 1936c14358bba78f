"""Drop-in for the reference's Knowledge_Distillation/pimg.py (the torch fork of the CSU-TDA PersistenceImages class behind
`Teacher_Model.forward(grad_PI=True)`), on the general HIP imager (`tlc_pi_image` / `tlc_pi_image_vjp`, csrc/pi_general.hip).

  linear_ramp :11-32, bvncdf :34-53, PersistenceImager.__init__ :209-244, the setters :262-290, __repr__ :292-302,
  _create_mesh :304-316, fit :318-352, transform :354-414, fit_transform :416-436.

Unlike `sg2dgm/PersistenceImager.py`, which accepts only the configuration the TLC-GNN pipeline uses, every argument of the class is
honoured here: any ranges and pixel size (through the constructor, the setters or `fit`), `skew=False`, `weight_params`, a custom
weight function, and `kernel_params['sigma']` as a scalar, a diagonal or a full 2 x 2 matrix.

LAYOUT.  An image is `[birth_bin, pers_bin]` ALWAYS.  The reference keeps that layout only for an isotropic sigma; its general branch
(`sigma_b != sigma_p` or a correlated sigma) builds `np.meshgrid(bpnts, ppnts)` with 'xy' indexing and reshapes to
`(res0 + 1, res1 + 1)`, so for a square grid it returns the TRANSPOSE `[pers_bin, birth_bin]`, and for a rectangular grid the
reshape scrambles the image: the reference's rectangular non-isotropic output is not meaningful and is not reproduced.

CORRELATION.  |r| >= 0.925 (r = cov / sqrt(var_b var_p)) is refused: the reference's branch for it differs from the exact bivariate
CDF by 0.15 at r = +-0.95, so there is nothing to agree with.  Below 0.925 the reference (transposed) and this module agree with
the exact CDF to a few 1e-16.
"""
import numpy as np

from .. import engine

_RAMP_KEYS = ("low", "high", "start", "end")
_RAMP_DEFAULT = dict(low=0.0, high=1.0, start=0.0, end=1.0)
R_MAX = 0.925


def linear_ramp(birth, pers, low=0.0, high=1.0, start=0.0, end=1.0):
    """Weight of (birth, persistence) pairs (:11-32): `low` below `start`, `high` above `end`, the straight line between.  Tensors give a
    tensor, arrays an array (`birth` only fixes the length).  The HIP imager evaluates the same ramp on the device."""
    try:
        import torch
        if isinstance(pers, torch.Tensor):
            line = (pers - start) * (high - low) / (end - start) + low
            return torch.where(pers < start, torch.full_like(line, low), torch.where(pers > end, torch.full_like(line, high), line))
    except ImportError:  # pragma: no cover
        pass
    pers = np.asarray(pers, dtype=np.float64)
    line = (pers - start) * (high - low) / (end - start) + low
    return np.where(pers < start, low, np.where(pers > end, high, line))


def _phi(z):
    import torch
    z = np.asarray(z, dtype=np.float64)
    return (torch.special.erfc(torch.from_numpy(np.ascontiguousarray(-z / np.sqrt(2.0)))) / 2.0).numpy().reshape(z.shape)


def parse_sigma(sigma):
    """kernel_params['sigma'] -> (var_b, var_p, cov): a scalar is an isotropic variance, a 2 x 2 matrix must be symmetric, positive
    definite and have |r| < 0.925 (ValueError otherwise, saying why)."""
    if sigma is None:
        return 1.0, 1.0, 0.0
    s = np.asarray(sigma, dtype=np.float64)
    if s.ndim == 0:
        vb = vp = float(s)
        cov = 0.0
    elif s.shape == (2, 2):
        if s[0, 1] != s[1, 0]:
            raise ValueError("sigma %s is not symmetric" % s.tolist())
        vb, vp, cov = float(s[0, 0]), float(s[1, 1]), float(s[0, 1])
    else:
        raise ValueError("sigma must be a scalar variance or a 2 x 2 covariance matrix, not shape %s" % (s.shape,))
    if not (np.isfinite(vb) and np.isfinite(vp) and np.isfinite(cov)):
        raise ValueError("sigma is not finite")
    if not (vb > 0.0 and vp > 0.0 and vb * vp - cov * cov > 0.0):
        raise ValueError("sigma [[%g, %g], [%g, %g]] is singular or not positive definite" % (vb, cov, cov, vp))
    r = cov / np.sqrt(vb * vp)
    if cov != 0.0 and abs(r) >= R_MAX:
        raise ValueError("correlation r = %g: |r| >= %g is refused (the reference's branch for it is wrong by 0.15 at |r| = 0.95)" % (r, R_MAX))
    return vb, vp, cov


def bvncdf(birth, pers, mu=None, sigma=None):
    """P(X <= birth, Y <= pers) of the normal distribution with mean `mu` and covariance `sigma` (:34-53), on the host: the product of
    two univariate CDFs for a diagonal sigma, else the Drezner-Wesolowsky form -- Phi Phi + asin(r) / (4 pi) * the Gauss-Legendre sum
    over the correlation (6, 12 or 20 nodes) -- that the HIP imager evaluates at the grid corners.  It is the class's only kernel."""
    mu = np.zeros(2) if mu is None else np.asarray(mu, dtype=np.float64)
    vb, vp, cov = parse_sigma(sigma)
    zb = (np.asarray(birth, dtype=np.float64) - mu[0]) / np.sqrt(vb)
    zp = (np.asarray(pers, dtype=np.float64) - mu[1]) / np.sqrt(vp)
    out = _phi(zb) * _phi(zp)
    if cov == 0.0:
        return out
    r = cov / np.sqrt(vb * vp)
    x, w = np.polynomial.legendre.leggauss(6 if abs(r) < 0.3 else (12 if abs(r) < 0.75 else 20))
    asr = np.arcsin(r)
    sn = np.sin(asr * (1.0 + x) / 2.0)
    hk, hs = zb * zp, (zb * zb + zp * zp) / 2.0
    quad = sum(wj * np.exp((sj * hk - hs) / (1.0 - sj * sj)) for wj, sj in zip(w, sn))
    return out + asr * quad / (4.0 * np.pi)


def _dict_text(d):
    return "None" if d is None else "{" + ", ".join("%s: %s" % (k, str(v)) for k, v in d.items()) + "}"


class PersistenceImager:
    """The reference's class (:208-436): same constructor signature and defaults, same grid state machine -- `_bpnts` / `_ppnts`
    equal the reference's arrays after the same calls, the padding of incommensurable ranges and the (res, res) resolution that
    unequal construction ranges keep included --, images on the GPU."""

    def __init__(self, birth_range=None, pers_range=None, pixel_size=None, resolution=5,
                 weight=linear_ramp, weight_params=None, kernel=bvncdf, kernel_params=None):
        if kernel is not bvncdf:
            raise NotImplementedError("PersistenceImager: bvncdf is the only kernel the HIP imager evaluates")
        birth_range = (0.0, 1.0) if birth_range is None else birth_range
        pers_range = (0.0, 1.0) if pers_range is None else pers_range
        self._resolution = (resolution, resolution)
        if pixel_size is None:
            pixel_size = np.min([pers_range[1] - pers_range[0], birth_range[1] - birth_range[0]]) / resolution
        self.weight = weight
        self.weight_params = {} if weight_params is None else weight_params
        self.kernel = kernel
        self.kernel_params = {'sigma': np.array([[1.0, 0.0], [0.0, 1.0]])} if kernel_params is None else kernel_params
        self._pixel_size = pixel_size
        self._birth_range, self._pers_range = birth_range, pers_range
        self._width = birth_range[1] - birth_range[0]
        self._height = pers_range[1] - pers_range[0]
        self._create_mesh()

    # ---- the grid ----------------------------------------------------------------------------------------------------------------
    width = property(lambda self: self._width)
    height = property(lambda self: self._height)
    resolution = property(lambda self: self._resolution)

    def _cover(self, rng):
        # whole pixels that cover a range (:265-266)
        return int(np.ceil((rng[1] - rng[0]) / self._pixel_size)) * self._pixel_size

    def _regrid(self):
        self._resolution = (int(self._width / self._pixel_size), int(self._height / self._pixel_size))
        self._create_mesh()

    @property
    def pixel_size(self):
        return self._pixel_size

    @pixel_size.setter
    def pixel_size(self, val):
        self._pixel_size = val
        self._width, self._height = self._cover(self._birth_range), self._cover(self._pers_range)
        self._regrid()

    @property
    def birth_range(self):
        return self._birth_range

    @birth_range.setter
    def birth_range(self, val):
        self._birth_range = val
        self._width = self._cover(val)
        self._regrid()

    @property
    def pers_range(self):
        return self._pers_range

    @pers_range.setter
    def pers_range(self, val):
        self._pers_range = val
        self._height = self._cover(val)
        self._regrid()

    def _create_mesh(self):
        """:304-316.  The ranges grow by half the padding on each side so that they span whole pixels; the grid lines are the
        `linspace` of res + 1 points over [lo, hi + pixel).  With unequal construction ranges the resolution stays (res, res) and
        the spacing is (width + pixel) / (res + 1), not the pixel size: the grid is whatever this linspace gives."""
        (b0, b1), (p0, p1) = self._birth_range, self._pers_range
        db, dp = self._width - (b1 - b0), self._height - (p1 - p0)
        self._birth_range = (b0 - db / 2, b1 + db / 2)
        self._pers_range = (p0 - dp / 2, p1 + dp / 2)
        self._bpnts = np.linspace(self._birth_range[0], self._birth_range[1] + self._pixel_size, self._resolution[0] + 1,
                                  endpoint=False, dtype=np.float64)
        self._ppnts = np.linspace(self._pers_range[0], self._pers_range[1] + self._pixel_size, self._resolution[1] + 1,
                                  endpoint=False, dtype=np.float64)

    def __repr__(self):
        return ("PersistenceImager object: \n"
                "  pixel size: %g \n" % self.pixel_size
                + "  resolution: (%d, %d) \n" % self.resolution
                + "  birth range: (%g, %g) \n" % self.birth_range
                + "  persistence range: (%g, %g) \n" % self.pers_range
                + "  weight: %s \n" % self.weight.__name__
                + "  kernel: %s \n" % self.kernel.__name__
                + "  weight parameters: %s \n" % _dict_text(self.weight_params)
                + "  kernel parameters: %s" % _dict_text(self.kernel_params))

    @staticmethod
    def _host(dgm):
        try:
            import torch
            if isinstance(dgm, torch.Tensor):
                dgm = dgm.detach().cpu().numpy()
        except ImportError:  # pragma: no cover
            pass
        return np.array(dgm, dtype=np.float64).reshape(-1, 2)

    def fit(self, pers_dgms, skew=True):
        """:318-352.  The ranges become the extent of the diagrams in the birth-persistence plane (first the birth range, then the
        persistence range, through the setters: the pixel size is kept)."""
        lo_b, hi_b, lo_p, hi_p = np.inf, -np.inf, np.inf, -np.inf
        for dgm in pers_dgms:
            d = self._host(dgm)
            if skew:
                d[:, 1] = d[:, 1] - d[:, 0]
            (mn_b, mn_p), (mx_b, mx_p) = d.min(axis=0), d.max(axis=0)
            if mn_b < lo_b:
                lo_b = mn_b
            if mn_p < lo_p:
                lo_p = mn_p
            if mx_b > hi_b:
                hi_b = mx_b
            if mx_p > hi_p:
                hi_p = mx_p
        self.birth_range = (lo_b, hi_b)
        self.pers_range = (lo_p, hi_p)

    # ---- the specification the kernels take ------------------------------------------------------------------------------------------
    def weight_is_ramp(self):
        return self.weight is linear_ramp

    def spec(self, skew=True):
        """The `engine.PiSpec` of this imager's present state (ValueError for a sigma or ramp the kernels refuse)."""
        if self.kernel is not bvncdf:
            raise NotImplementedError("PersistenceImager: bvncdf is the only kernel the HIP imager evaluates")
        ramp = dict(_RAMP_DEFAULT)
        if self.weight_is_ramp():
            unknown = set(self.weight_params) - set(_RAMP_KEYS)
            if unknown:
                raise ValueError("linear_ramp has no parameter(s) %s" % sorted(unknown))
            ramp.update(self.weight_params)
            if not ramp["end"] > ramp["start"]:
                raise ValueError("linear_ramp needs end > start (start %g, end %g)" % (ramp["start"], ramp["end"]))
        rb, rp = self._resolution
        if not (1 <= rb <= engine._lib.PI_MAX_RES and 1 <= rp <= engine._lib.PI_MAX_RES):
            raise ValueError("resolution (%d, %d) outside 1 .. %d" % (rb, rp, engine._lib.PI_MAX_RES))
        return engine.PiSpec(self._bpnts, self._ppnts, [ramp[k] for k in _RAMP_KEYS], parse_sigma(self.kernel_params.get('sigma')), skew)

    def _host_weights(self, pts64, skew):
        """A custom weight function runs on the host, on (birth, persistence) arrays, and its values go to the kernel as they are."""
        d = pts64.detach().cpu().numpy().copy()
        if skew:
            d[:, 1] = d[:, 1] - d[:, 0]
        w = self.weight(d[:, 0], d[:, 1], **self.weight_params)
        return np.ascontiguousarray(np.asarray(w, dtype=np.float64).reshape(-1))

    def transform_batch(self, pts, offs, skew=True):
        """Images of a packed batch: pts [K, 2] and offs int64[B + 1] (tensors or arrays) -> device tensor [B, Rb, Rp] in pts' dtype
        (float64 for arrays), differentiable in pts like `transform`."""
        import torch
        from .. import autograd
        pts = pts if isinstance(pts, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(pts, dtype=np.float64).reshape(-1, 2)))
        offs = offs if isinstance(offs, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(offs, dtype=np.int64)))
        pts, offs = pts.cuda(), offs.cuda().to(torch.int64)
        spec = self.spec(skew)
        rb, rp = spec.resolution
        if self.weight_is_ramp():
            img = autograd.GeneralDiagramImage.apply(pts, offs, spec, "weight")
        else:
            if pts.requires_grad and torch.is_grad_enabled():
                raise ValueError("PersistenceImager: a custom weight function is evaluated on the host; its images are forward only "
                                 "(detach the diagram)")
            p64 = pts.detach().to(torch.float64).contiguous()
            w = torch.from_numpy(self._host_weights(p64, skew)).to(p64.device)
            img = engine.pi_image(offs, p64, spec, weights=w).to(pts.dtype)
        return img.reshape(offs.numel() - 1, rb, rp)

    def transform(self, pers_dgm, skew=True, use_cuda=True):
        """:354-414.  pers_dgm: (N, 2) tensor or array of (birth, death) pairs -- (birth, persistence) with skew=False -> tensor
        [Rb, Rp], `[birth_bin, pers_bin]`, in the input's dtype, on the GPU (use_cuda=False: computed there, returned on the host).
        Differentiable like the reference's: the CDF factors are detached (:392,395), the gradient reaches a point through its
        weight alone (`autograd.diagram_image(..., imager=self, grad='full')` has the true derivative)."""
        n = int(pers_dgm.shape[0]) if hasattr(pers_dgm, "shape") else len(pers_dgm)
        img = self.transform_batch(pers_dgm, np.array([0, n], dtype=np.int64), skew=skew)[0]
        return img if use_cuda else img.cpu()

    def fit_transform(self, pers_dgms, skew=True):
        """:416-436.  `fit`, then the image of every diagram (a list, one launch)."""
        dgms = [self._host(d) for d in pers_dgms]
        self.fit(dgms, skew=skew)
        offs = np.concatenate([[0], np.cumsum([len(d) for d in dgms])]).astype(np.int64)
        pts = np.concatenate(dgms) if len(dgms) else np.zeros((0, 2))
        return list(self.transform_batch(pts, offs, skew=skew)) if len(dgms) else []

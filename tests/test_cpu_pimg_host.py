"""CPU: the host side of the general persistence imager (Knowledge_Distillation/pimg.py, engine.PiSpec, include/tlcgnn.h) -- no GPU call.

The restatement of tests/pimg_cases.py is checked against the reference's recorded images (tests/golden/pimg_general.npz, made by
tests/golden/make_golden_pimg.py) and against scipy's exact bivariate CDF; the drop-in's grid state machine, `fit` and `__repr__`
against the reference's recorded state; the header's constants against their mirrors; and the refusals Python makes itself."""
import os
import re

import numpy as np
import pytest

import pimg_cases as cases
from tlc_gnn_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "pimg_general.npz"))


@pytest.fixture(scope="module")
def pimg():
    from tlc_gnn_amd.Knowledge_Distillation import pimg
    return pimg


def dropin(pimg, ctor, steps):
    return cases.apply_grid_steps(pimg.PersistenceImager(**ctor), steps)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cases.IMAGE_CASES))
def test_restatement_matches_reference_images(golden, pimg, name):
    """Within the issue's bound (largest ratio seen: 1.5e-3).  The diagonal and correlated goldens are the reference's transposed
    output, so they are compared through .T."""
    c, d = cases.case_inputs(name)
    assert np.array_equal(d, golden["img_%s_pts" % name])
    im = dropin(pimg, cases.case_ctor(c), c["steps"])
    bp, pp, rp, sg, sk = cases.case_spec(im, c)
    assert np.array_equal(bp, golden["img_%s_bpnts" % name]) and np.array_equal(pp, golden["img_%s_ppnts" % name])
    img, wsum = cases.image(d, bp, pp, rp, sg, sk)
    ref = golden["img_%s_out" % name]
    ref = ref.T if c["transposed"] else ref
    assert img.shape == ref.shape
    ratio = cases.worst_ratio(img, ref, len(d), wsum, correlated=sg[2] != 0.0)
    print("%s: ratio %.3g" % (name, ratio))
    assert ratio <= 1.0


def test_reference_nonisotropic_output_is_the_transpose(golden):
    """fact 1 of the layout: untransposed, the diagonal-sigma golden is far from [birth_bin, pers_bin]"""
    c, d = cases.case_inputs("diag_8")
    img, _ = cases.image(d, golden["img_diag_8_bpnts"], golden["img_diag_8_ppnts"], sigma=(0.01, 0.04, 0.0))
    assert np.abs(img - golden["img_diag_8_out"]).max() > 0.05
    assert np.abs(img - golden["img_diag_8_out"].T).max() < 1e-14


@pytest.mark.parametrize("r", [0.2, 0.5, 0.8, -0.5, 0.29, 0.74, 0.92, -0.92])
def test_restatement_bvn_matches_scipy(r):
    """the Gauss-Legendre form against scipy.stats.multivariate_normal.cdf on a grid of arguments, every node count"""
    from scipy.stats import multivariate_normal
    z = np.array([-4.0, -1.5, -0.3, 0.0, 0.7, 2.2, 5.0])
    zb, zp = np.meshgrid(z, z, indexing="ij")
    got = cases.bvn(zb, zp, r)
    want = multivariate_normal.cdf(np.stack([zb, zp], -1), mean=[0.0, 0.0], cov=[[1.0, r], [r, 1.0]], abseps=1e-14, releps=1e-14)
    assert np.abs(got - want).max() < 5e-13          # scipy's own quadrature error dominates; the formula's is ~1e-16


def test_dropin_bvncdf_matches_restatement(pimg):
    rs = np.random.RandomState(0)
    x, y = rs.randn(50), rs.randn(50)
    for vb, vp, r in ((0.5, 2.0, 0.0), (0.5, 2.0, 0.2), (1.0, 1.0, 0.6), (0.1, 0.3, -0.9)):
        cov = r * np.sqrt(vb * vp)
        got = pimg.bvncdf(x, y, mu=np.array([0.1, -0.2]), sigma=np.array([[vb, cov], [cov, vp]]))
        zb, zp = (x - 0.1) / np.sqrt(vb), (y + 0.2) / np.sqrt(vp)
        want = cases.phi(zb) * cases.phi(zp) if r == 0.0 else cases.bvn(zb, zp, r)
        assert np.abs(got - want).max() < 1e-15


def test_device_quadrature_tables_are_leggauss():
    """the constants in csrc/pi_general.hip are the positive halves of numpy's 6-, 12- and 20-point rules, 17 significant digits"""
    src = open(os.path.join(ROOT, "tlc-gnn_amd", "csrc", "pi_general.hip")).read()
    for n in (6, 12, 20):
        x, w = np.polynomial.legendre.leggauss(n)
        for tag, want in (("X", x[x > 0][::-1]), ("W", w[x > 0][::-1])):
            m = re.search(r"PIG_GL%d_%s\[\d+\] = \{([^}]*)\}" % (n, tag), src)
            got = np.array([float(t) for t in m.group(1).replace("\n", " ").split(",")])
            assert np.array_equal(got, want), (n, tag)


# ---- the drop-in's grid ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cases.GRID_CASES))
def test_grid_state_machine_matches_reference(golden, pimg, name):
    ctor, steps = cases.GRID_CASES[name]
    im = dropin(pimg, ctor, steps)
    assert np.array_equal(im._bpnts, golden["grid_%s_bpnts" % name])
    assert np.array_equal(im._ppnts, golden["grid_%s_ppnts" % name])
    state = np.array([im.pixel_size, im.resolution[0], im.resolution[1], im.birth_range[0], im.birth_range[1], im.pers_range[0],
                      im.pers_range[1], im.width, im.height], dtype=np.float64)
    assert np.array_equal(state, golden["grid_%s_state" % name])
    assert repr(im) == str(golden["grid_%s_repr" % name])


def test_rectangular_and_unequal_range_grids(pimg):
    """fact 3: the setters make (20, 10); unequal construction ranges keep (res, res) with a spacing that is not the pixel"""
    im = dropin(pimg, *cases.GRID_CASES["setters_rect"])
    assert im.resolution == (20, 10) and im._bpnts.size == 21 and im._ppnts.size == 11
    im = dropin(pimg, *cases.GRID_CASES["unequal_ctor"])
    assert im.resolution == (5, 5) and im.pixel_size == 0.2
    assert abs((im._bpnts[1] - im._bpnts[0]) - 2.2 / 6) < 1e-15
    spec = im.spec()
    assert spec.resolution == (5, 5) and np.array_equal(spec.bpnts, im._bpnts) and spec.skew


def test_default_spec_is_the_default_imager(pimg):
    from tlc_gnn_amd import engine
    for res in (1, 5, 8):
        im = pimg.PersistenceImager(resolution=res)
        s, d = im.spec(), engine.PiSpec.default(res)
        assert np.array_equal(s.bpnts, d.bpnts) and np.array_equal(s.ppnts, d.ppnts)
        assert np.array_equal(s.ramp, d.ramp) and np.array_equal(s.sigma, d.sigma) and s.skew == d.skew
        assert np.array_equal(d.bpnts, cases.default_lines(res))


def test_sigma_forms(pimg):
    assert pimg.parse_sigma(0.01) == (0.01, 0.01, 0.0)
    assert pimg.parse_sigma(np.diag([0.01, 0.04])) == (0.01, 0.04, 0.0)
    assert pimg.parse_sigma([[2.0, 0.5], [0.5, 1.0]]) == (2.0, 1.0, 0.5)
    assert pimg.parse_sigma(None) == (1.0, 1.0, 0.0)
    im = pimg.PersistenceImager(resolution=4, kernel_params={"sigma": 0.25}, weight_params=dict(high=3.0, end=0.5))
    s = im.spec(skew=False)
    assert s.sigma.tolist() == [0.25, 0.25, 0.0] and s.ramp.tolist() == [0.0, 3.0, 0.0, 0.5] and not s.skew


def test_linear_ramp_host(pimg):
    import torch
    p = np.array([-1.0, 0.2, 0.4, 0.6, 0.9])
    want = np.array([0.25, 0.25, 1.125, 2.0, 2.0])
    assert np.allclose(pimg.linear_ramp(p, p, low=0.25, high=2.0, start=0.2, end=0.6), want, rtol=0, atol=1e-15)
    assert np.allclose(pimg.linear_ramp(torch.from_numpy(p), torch.from_numpy(p), low=0.25, high=2.0, start=0.2, end=0.6).numpy(), want,
                       rtol=0, atol=1e-15)
    assert np.array_equal(pimg.linear_ramp(p, p), cases.ramp(p))


# ---- constants and refusals ----------------------------------------------------------------------------------------------------------
def test_header_constants_match_mirrors():
    header = open(os.path.join(ROOT, "include", "tlcgnn.h")).read()
    val = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, header).group(1))  # noqa: E731
    assert val("TLC_PI_MAX_RES") == _lib.PI_MAX_RES == cases.MAX_RES == 128
    assert val("TLC_PI_GRAD_WEIGHT") == _lib.PI_GRAD_WEIGHT == 0
    assert val("TLC_PI_GRAD_FULL") == _lib.PI_GRAD_FULL == 1
    layouts = open(os.path.join(ROOT, "tlc-gnn_amd", "csrc", "scratch_layouts.h")).read()
    m = re.search(r"struct TlcPiImageScratch \{\s*static constexpr int64_t SLICE = (\d+), MAX_GROUP = (\d+);", layouts)
    assert (int(m.group(1)), int(m.group(2))) == (_lib.PI_SLICE, _lib.PI_GROUP) == (cases.SLICE, cases.GROUP)
    src = open(os.path.join(ROOT, "tlc-gnn_amd", "csrc", "pi_general.hip")).read()
    assert int(re.search(r"#define PIG_C (\d+)", src).group(1)) == _lib.PI_CHUNK == cases.CHUNK
    for sym in ("tlc_pi_image", "tlc_pi_image_vjp", "tlc_pi_image_work_bytes"):
        assert sym in _lib.SYMBOLS and getattr(_lib.lib(), sym).argtypes, sym


def test_work_bytes_is_host_arithmetic():
    """one definition (TlcPiImageScratch): 0 up to a slice; above it slices x pixels x 8 (+ 256 of alignment), 32 diagrams at most"""
    import ctypes as C
    L = _lib.lib()
    least = C.c_int64(-5)
    assert L.tlc_pi_image_work_bytes(7, cases.SLICE, 50, 50, C.byref(least)) == 0 and least.value == 0
    assert L.tlc_pi_image_work_bytes(1, cases.SLICE + 1, 50, 40, C.byref(least)) == 2 * 2000 * 8 + 256 and least.value == 2 * 2000 * 8 + 256
    assert L.tlc_pi_image_work_bytes(100, 70000, 100, 100, C.byref(least)) == 32 * 69 * 10000 * 8 + 256
    assert least.value == 69 * 10000 * 8 + 256
    assert L.tlc_pi_image_work_bytes(3, 5000, 128, 1, None) == 3 * 5 * 128 * 8 + 256
    for bad in ((-1, 10, 5, 5), (1, -1, 5, 5), (1, 10, 0, 5), (1, 10, 5, 129)):
        assert L.tlc_pi_image_work_bytes(*bad, None) == -1
        assert b"tlc_pi_image_work_bytes" in L.tlc_last_error()


def test_specification_is_refused_before_any_device_call():
    """the C ABI checks the specification on the host, first: with no diagrams the refusals need no GPU"""
    from tlc_gnn_amd import engine
    L = _lib.lib()
    good = engine.PiSpec.default(5)
    assert L.tlc_pi_image(0, 0, None, None, None, None, *good._c_args(), None, None, 0, None) == 0
    assert L.tlc_pi_image_vjp(0, 0, None, None, *good._c_args(), _lib.PI_GRAD_FULL, None, None, None) == 0
    for say, bp, pp, rp, sg in cases.refusal_specs():
        s = engine.PiSpec(bp, pp, rp, sg)
        assert L.tlc_pi_image(0, 0, None, None, None, None, *s._c_args(), None, None, 0, None) == 1, say
        msg = L.tlc_last_error().decode()
        assert "tlc_pi_image" in msg and say in msg, (say, msg)
        assert L.tlc_pi_image_vjp(0, 0, None, None, *s._c_args(), _lib.PI_GRAD_WEIGHT, None, None, None) == 1, say
        assert say in L.tlc_last_error().decode()
    r5 = 0.5 * np.sqrt(0.02 * 0.03)
    corr = engine.PiSpec(good.bpnts, good.ppnts, sigma=(0.02, 0.03, r5))
    assert L.tlc_pi_image_vjp(0, 0, None, None, *corr._c_args(), _lib.PI_GRAD_WEIGHT, None, None, None) == 0
    assert L.tlc_pi_image_vjp(0, 0, None, None, *corr._c_args(), _lib.PI_GRAD_FULL, None, None, None) == 1
    assert "separable" in L.tlc_last_error().decode()
    assert L.tlc_pi_image_vjp(0, 0, None, None, *good._c_args(), 2, None, None, None) == 1
    assert "mode" in L.tlc_last_error().decode()


def test_python_side_refusals(pimg):
    with pytest.raises(NotImplementedError, match="bvncdf"):
        pimg.PersistenceImager(kernel=lambda *a, **k: 0.0)
    r95 = 0.95 * np.sqrt(0.02 * 0.03)
    with pytest.raises(ValueError, match="0.925"):
        pimg.PersistenceImager(kernel_params={"sigma": np.array([[0.02, r95], [r95, 0.03]])}).spec()
    with pytest.raises(ValueError, match="positive definite"):
        pimg.PersistenceImager(kernel_params={"sigma": np.array([[1.0, 2.0], [2.0, 1.0]])}).spec()
    with pytest.raises(ValueError, match="positive definite"):
        pimg.PersistenceImager(kernel_params={"sigma": -0.1}).spec()
    with pytest.raises(ValueError, match="symmetric"):
        pimg.PersistenceImager(kernel_params={"sigma": np.array([[1.0, 0.1], [0.2, 1.0]])}).spec()
    with pytest.raises(ValueError, match="end > start"):
        pimg.PersistenceImager(weight_params=dict(start=0.5, end=0.5)).spec()
    with pytest.raises(ValueError, match="no parameter"):
        pimg.PersistenceImager(weight_params=dict(slope=2.0)).spec()
    im = pimg.PersistenceImager(resolution=5)
    im.pixel_size = 1.0 / 200
    with pytest.raises(ValueError, match="outside 1 .. 128"):
        im.spec()
    from tlc_gnn_amd import autograd, engine
    import torch
    with pytest.raises(ValueError, match="'weight' or 'full'"):
        autograd.diagram_image(torch.zeros(2, 2), res=5, grad="position")
    with pytest.raises(ValueError, match="forward only"):
        autograd.diagram_image(torch.zeros(2, 2), imager=pimg.PersistenceImager(weight=lambda b, p: p * p))
    with pytest.raises(ValueError, match="'weight' or 'full'"):
        engine.pi_image_vjp.__wrapped__(torch.zeros(2, dtype=torch.int64), torch.zeros(1, 2), torch.zeros(1, 25), engine.PiSpec.default(5),
                                        mode="both")

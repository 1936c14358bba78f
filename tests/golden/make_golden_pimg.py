#!/usr/bin/env python
"""Regenerates tests/golden/pimg_general.npz by RUNNING THE UNMODIFIED REFERENCE imager on the cases of tests/pimg_cases.py.

Run from the repo root:  python tests/golden/make_golden_pimg.py

Like make_golden.py it exposes the reference's `sg2dgm/PersistenceImager.pyx` as a `.py` module in a throw-away directory (a
symlink; the file is plain Python) and stores INPUTS + EXPECTED OUTPUTS as data.  `numpy.Inf` is gone from numpy 2, and the reference's
`fit` uses it: the generator sets `numpy.Inf = numpy.inf` for its own process so that `fit` runs.

Stored:
  grid_<case>_{bpnts,ppnts,state}   the grid lines and (pixel, res0, res1, b0, b1, p0, p1, width, height) after the case's steps
  grid_<case>_repr                  repr(imager)
  img_<case>_{pts,out}              the diagram and the image AS THE REFERENCE RETURNS IT: [birth_bin, pers_bin] for an isotropic
                                    sigma, the transpose [pers_bin, birth_bin] for the diagonal and correlated cases (its general
                                    branch meshes with 'xy' indexing) -- pimg_cases.IMAGE_CASES[case]['transposed'] says which
  img_<case>_{bpnts,ppnts}          the grid of the image
"""
import importlib
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.dirname(HERE))

import pimg_cases as cases  # noqa: E402


def load_reference():
    np.Inf = np.inf
    tmp = tempfile.mkdtemp(prefix="pimg_ref_")
    os.symlink(os.path.join(REF, "sg2dgm", "PersistenceImager.pyx"), os.path.join(tmp, "ref_persistence_imager.py"))
    sys.path.insert(0, tmp)
    return importlib.import_module("ref_persistence_imager")


def main():
    ref = load_reference()
    out = {}
    for name, (ctor, steps) in cases.GRID_CASES.items():
        im = cases.apply_grid_steps(ref.PersistenceImager(**ctor), steps)
        out["grid_%s_bpnts" % name] = np.asarray(im._bpnts)
        out["grid_%s_ppnts" % name] = np.asarray(im._ppnts)
        out["grid_%s_state" % name] = np.array([im.pixel_size, im.resolution[0], im.resolution[1], im.birth_range[0], im.birth_range[1],
                                                im.pers_range[0], im.pers_range[1], im.width, im.height], dtype=np.float64)
        out["grid_%s_repr" % name] = np.array(repr(im))
    for name in cases.IMAGE_CASES:
        c, d = cases.case_inputs(name)
        im = cases.apply_grid_steps(ref.PersistenceImager(**cases.case_ctor(c)), c["steps"])
        out["img_%s_pts" % name] = d
        out["img_%s_bpnts" % name] = np.asarray(im._bpnts)
        out["img_%s_ppnts" % name] = np.asarray(im._ppnts)
        out["img_%s_out" % name] = np.asarray(im.transform(d, skew=c["skew"]))
        print(name, out["img_%s_out" % name].shape, float(out["img_%s_out" % name].sum()))
    path = os.path.join(HERE, "pimg_general.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

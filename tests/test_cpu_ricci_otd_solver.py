"""CPU: the transportation solver of the exact Ollivier-Ricci kernels, csrc/ricci_otd_solve.h -- the very source the kernels compile,
built here for the host (tests/aids/otd_solve_host.cpp) and run by one thread and by eight threads behind a barrier -- against the LP
reference and the closed forms of tests/ricci_otd_cases.py, with == on the integers.  It also holds the rounds a solve takes against
the solver's cap, 4 (na + nb) + 64, which is a watchdog and not a proven bound: a solve may use a quarter of it at the most here, so a
change that brings real edges near the cap fails a test before it turns an edge into NaN on the device."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import ricci_otd_cases as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def solver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler (g++, c++ or clang++) is needed to build csrc/ricci_otd_solve.h for the host"
    exe = str(tmp_path_factory.mktemp("otd") / "otd_solve_host")
    subprocess.run([cxx, "-O2", "-std=c++20", "-pthread", "-I", os.path.join(ROOT, "tlc-gnn_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "aids", "otd_solve_host.cpp")], check=True)

    def run(problems):
        lines = [str(len(problems))]
        for a, b, c in problems:
            lines += ["%d %d" % (len(a), len(b)), " ".join(map(str, a.tolist())), " ".join(map(str, b.tolist())), " ".join(map(str, c.ravel().tolist()))]
        out = subprocess.run([exe], input="\n".join(lines), stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")
        return [tuple(int(v) for v in l.split()) for l in out if l.strip()]
    return run


def _check(solver, jobs):
    """jobs: (graph, s, t, num, den, expected W or None for the LP's)"""
    res = solver([oc.reduced_problem(g[0], g[1], s, t, num, den) for g, s, t, num, den, _ in jobs])
    assert len(res) == len(jobs)
    for (g, s, t, num, den, want), (w1, w8, rounds, cap) in zip(jobs, res):
        if want is None:
            want = oc.exact_wd(g[0], g[1], s, t, num, den)[0]
        deg = np.bincount(g[1].ravel(), minlength=g[0])
        na, nb = int(deg[s]) + 1, int(deg[t]) + 1
        assert w1 == want and w8 == want, (s, t, num, den, w1, w8, want)
        assert cap == 4 * (na + nb) + 64 and 0 <= rounds <= cap // 4, (na, nb, rounds, cap)


def test_random_graphs_every_edge_and_orientation(solver):
    jobs = []
    for g in (oc.gnp(24, 0.4, 5), oc.random_tree(60, 3)):
        for s, t in g[1].tolist():
            jobs += [(g, s, t, 1, 2, None), (g, t, s, 1, 2, None)]
    g = oc.gnp(24, 0.4, 5)
    for s, t in g[1][:40].tolist():
        jobs += [(g, s, t, 0, 1, None), (g, s, t, 1, 1, None), (g, s, t, 1, 4, None), (g, s, t, 1023, 1024, None)]
    _check(solver, jobs)


def test_closed_forms(solver):
    jobs = []
    for n in (3, 4, 5, 8):
        g = oc.complete(n)
        jobs.append((g, 0, 1, 1, 2, int((1 - oc.kappa_complete(n)) * 2 * (n - 1) ** 2)))
    for n in (3, 4, 5, 6, 7):
        jobs.append((oc.cycle(n), 0, 1, 1, 2, int((1 - oc.kappa_cycle(n)) * 8)))
    for d in (1, 2, 5, 9):
        jobs.append((oc.star(d), 0, 1, 1, 2, int((1 - oc.kappa_star(d)) * 2 * d)))
    for d, c, m in ((6, 2, 1), (12, 0, 5), (10, 4, 0), (799, 100, 300)):
        jobs.append((oc.two_hubs(d, d, c, m), 0, 1, 1, 2, int((1 - oc.kappa_two_hubs(d, c, m)) * 2 * d * d)))
    _check(solver, jobs)


def test_tier_shapes_with_all_four_codes(solver):
    """the lop-sided supports need the most rounds (a round pushes to at most min(na, nb) sinks): 250 x 6 takes about a hundred"""
    jobs = []
    for na, nb in ((64, 128), (91, 91), (250, 6), (6, 250), (2, 300), (300, 2), (201, 201)):
        ds, dt = na - 1, nb - 1
        c = (min(ds, dt) - 1) // 3
        lo = min(ds, dt) - 1 - c
        jobs.append((oc.two_hubs(ds, dt, c, m=lo // 3, cross=lo // 2, outside=5, seed=na + nb), 0, 1, 1, 2, None))
    _check(solver, jobs)

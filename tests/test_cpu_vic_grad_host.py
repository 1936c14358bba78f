"""CPU: the restatements of tests/vic_grad_cases.py against independent formulations, the header's constants and work sizes, and the
refusals that the entries of csrc/vic_grad.hip make before they launch anything -- no GPU call."""
import ctypes as C
import math
import os
import re

import numpy as np

import vic_grad_cases as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (0, 1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 2047, 2048, 2049, 2303, 2304, 2305, 5000, 70000)


def test_constants_mirror_the_header():
    from tlc_gnn_amd import _lib
    header = open(os.path.join(ROOT, "include", "tlcgnn.h")).read()
    got = {k: int(v) for k, v in re.findall(r"#define (TLC_SEG_[A-Z_]+)\s+(\d+)", header)}
    assert got == {"TLC_SEG_LANE_MAX": 16, "TLC_SEG_WAVE_MAX": 2048}
    assert (_lib.SEG_LANE_MAX, _lib.SEG_WAVE_MAX, _lib.SEG_WG_THREADS) == (vc.LANE_MAX, vc.WAVE_MAX, vc.WG_THREADS) == (16, 2048, 256)


def test_segment_sum_restatement_against_fsum():
    """|restated - fsum| <= L * 2^-53 * sum |v| for every class and cut: each of the at most L - 1 additions behind an output rounds a
    partial sum that is at most sum |v| in magnitude (to first order; the factor L instead of L - 1 covers the second-order terms)."""
    rng = np.random.default_rng(1)
    for L in LENGTHS:
        v = rng.normal(size=L) * 10.0 ** rng.integers(-3, 4, size=L)
        got = vc.segment_sum_one(v)
        assert abs(got - math.fsum(v)) <= L * 2.0 ** -53 * float(np.abs(v).sum()), L
        assert not np.signbit(got)  or got != 0.0, L


def test_segment_sum_restatement_is_exact_on_integers():
    rng = np.random.default_rng(2)
    for L in LENGTHS:
        v = rng.integers(-1000, 1000, size=L).astype(np.float64)
        assert vc.segment_sum_one(v) == float(v.astype(np.int64).sum()), L
    # every sum starts from +0.0: all -0.0 terms, and a cancelling pair, give +0.0
    for L in (1, 16, 17, 2049):
        z = vc.segment_sum_one(np.full(L, -0.0))
        assert z == 0.0 and not np.signbit(z), L
    z = vc.segment_sum_one(np.array([1.5, -1.5]))
    assert z == 0.0 and not np.signbit(z)


def test_segment_index_restatement():
    key = np.array([3, -1, 0, 3, 7, 2, 3, -5, 0, 9], np.int32)
    ptr, pos = vc.segment_index(key, 8)                                        # (9 is past the last key: skipped like a negative one)
    assert ptr.tolist() == [0, 2, 2, 3, 6, 6, 6, 6, 7] and pos.tolist() == [2, 8, 5, 0, 3, 6, 4, 1, 7, 9]
    val = np.arange(10, dtype=np.float64)
    assert vc.segment_sum(val, ptr, pos).tolist() == [10.0, 0.0, 5.0, 9.0, 0.0, 0.0, 0.0, 4.0]


def _host_batch(seed=4, n=60, m=150, B=40, hop=2):
    """A random graph and the packed vicinities ball(u) & ball(v) of B of its edges, built with Python sets."""
    rng = np.random.default_rng(seed)
    es = set()
    while len(es) < m:
        a, b = (int(x) for x in rng.integers(0, n, 2))
        if a != b:
            es.add((min(a, b), max(a, b)))
    ge = np.array(sorted(es), np.int32)
    adj = [set() for _ in range(n)]
    for a, b in ge:
        adj[a].add(int(b))
        adj[b].add(int(a))

    def ball(u):
        seen = {u}
        front = {u}
        for _ in range(hop):
            front = set().union(*(adj[x] for x in front)) - seen
            seen |= front
        return seen
    pairs = ge[rng.choice(len(ge), B, replace=False)]
    node_ptr, edge_ptr, ids, edges = [0], [0], [], []
    for u, v in pairs:
        S = sorted(ball(int(u)) & ball(int(v)))
        loc = {x: k for k, x in enumerate(S)}
        ids += S
        edges += [(loc[a], loc[b]) for a, b in ge if a in loc and b in loc]
        node_ptr.append(len(ids))
        edge_ptr.append(len(edges))
    return n, ge, pairs, np.array(node_ptr, np.int64), np.array(edge_ptr, np.int64), np.array(ids, np.int64), np.array(edges, np.int32).reshape(-1, 2)


def test_lookup_restatement_against_searchsorted():
    n, ge, pairs, node_ptr, edge_ptr, ids, edges = _host_batch()
    for one_root in (False, True):
        eid, roots, st = vc.lookup(ge, node_ptr, edge_ptr, ids, edges, pairs, one_root=one_root)
        eid2, roots2 = vc.lookup_searchsorted(n, ge, node_ptr, edge_ptr, ids, edges, pairs, one_root=one_root)
        assert not st.any() and np.array_equal(eid, eid2) and np.array_equal(roots, roots2)
        assert np.array_equal(np.sort(ge[eid], 1), np.sort(np.stack([ids[np.repeat(node_ptr[:-1], np.diff(edge_ptr)) + edges[:, 0]],
                                                                     ids[np.repeat(node_ptr[:-1], np.diff(edge_ptr)) + edges[:, 1]]], 1), 1))
    # an edge that is not in the list refuses its vicinity alone
    eid0, roots0, _ = vc.lookup(ge, node_ptr, edge_ptr, ids, edges, pairs)
    gone = int(eid0[edge_ptr[3]])
    eid, roots, st = vc.lookup(np.delete(ge, gone, 0), node_ptr, edge_ptr, ids, edges, pairs)
    hit = np.array([bool((eid0[edge_ptr[g]:edge_ptr[g + 1]] == gone).any()) for g in range(len(pairs))])
    assert hit[3] and not hit.all() and np.array_equal(st, np.where(hit, vc.ST_BAD_INPUT, vc.ST_OK))
    per_edge = np.repeat(hit, np.diff(edge_ptr))
    assert (eid[per_edge] == -1).all() and (roots[hit] == -1).all()
    assert np.array_equal(eid[~per_edge], eid0[~per_edge] - (eid0[~per_edge] > gone)) and np.array_equal(roots[~hit], roots0[~hit])


def test_work_sizes_against_their_definitions():
    from tlc_gnn_amd import _lib, engine
    for sym in ("tlc_packed_edge_lookup", "tlc_segment_index_work_bytes", "tlc_segment_index", "tlc_segment_sum_work_bytes",
                "tlc_segment_sum_f64", "tlc_lp_decode_bwd_pi_f32"):
        assert sym in _lib.SYMBOLS and getattr(_lib.lib(), sym).argtypes, sym
    for n_items, n_keys in ((0, 0), (1, 1), (63, 5), (4096, 70000), (4097, 65535), (10 ** 7, 44324)):
        assert engine.segment_index_work_bytes(n_items, n_keys) == vc.index_work_bytes(n_items, n_keys), (n_items, n_keys)
        assert engine.segment_sum_work_bytes(n_keys) == vc.sum_work_bytes(n_keys), n_keys


def test_refusals_launch_nothing():
    """Every refusal is decided before the first launch, so it can be asked for without a device."""
    from tlc_gnn_amd import _lib
    L = _lib.lib()
    F = C.c_void_p(0x1000)                                                    # non-null, 256-byte aligned, never read by a refused call
    need = C.c_int64(0)
    assert L.tlc_segment_index_work_bytes(-1, 1, C.byref(need)) == 1 and L.tlc_segment_index_work_bytes(1, 1 << 31, C.byref(need)) == 1
    assert L.tlc_segment_index_work_bytes(1, 1, None) == 1 and L.tlc_segment_sum_work_bytes(-1, C.byref(need)) == 1
    assert L.tlc_segment_sum_work_bytes(1, None) == 1
    # lookup: negative sizes, flags, null pointers, pairs without roots
    lk = lambda M=5, ge=F, B=2, np_=F, ep=F, ids=F, i64=1, e=F, tn=4, tm=4, pr=F, one=0, eid=F, ro=F, st=F: L.tlc_packed_edge_lookup(
        M, ge, B, np_, ep, ids, i64, e, tn, tm, pr, one, eid, ro, st, None)
    assert lk(B=0) == 0
    for kw in (dict(M=-1), dict(B=-1), dict(tn=-1), dict(tm=-1), dict(i64=2), dict(one=2), dict(ge=None), dict(np_=None), dict(ep=None),
               dict(ids=None), dict(e=None), dict(eid=None), dict(st=None), dict(pr=None), dict(ro=None), dict(M=1 << 31)):
        assert lk(**kw) == 1, kw
    # index and sum: sizes, null pointers, a small or misaligned workspace
    ix = lambda n=10, key=F, M=4, ptr=F, pos=F, w=F, wb=1 << 30: L.tlc_segment_index(n, key, M, ptr, pos, w, wb, None)
    for kw in (dict(n=-1), dict(M=-1), dict(n=1 << 31), dict(key=None), dict(ptr=None), dict(pos=None), dict(w=None),
               dict(wb=vc.index_work_bytes(10, 4) - 1), dict(w=C.c_void_p(0x1010))):
        assert ix(**kw) == 1, kw
    sm = lambda M=4, ptr=F, pos=F, n=10, val=F, out=F, w=F, wb=1 << 30: L.tlc_segment_sum_f64(M, ptr, pos, n, val, out, w, wb, None)
    assert sm(M=0) == 0
    for kw in (dict(M=-1), dict(n=-1), dict(ptr=None), dict(pos=None), dict(val=None), dict(out=None), dict(w=None),
               dict(wb=vc.sum_work_bytes(4) - 1), dict(w=C.c_void_p(0x1010))):
        assert sm(**kw) == 1, kw
    # decoder: other widths are unsupported, null pointers and negative sizes invalid
    dp = lambda E=3, n=5, ed=16, pd=25, pairs=F, gpi=F: L.tlc_lp_decode_bwd_pi_f32(E, pairs, F, F, n, ed, F, pd, F, F, F, F, F, gpi, None)
    assert dp(E=0) == 0 and dp(ed=8) == 4 and dp(pd=9) == 4
    assert dp(E=-1) == 1 and dp(n=0) == 1 and dp(pairs=None) == 1 and dp(gpi=None) == 1

"""Link-prediction scoring on the device (csrc/lp_metrics.hip, ops.binary_rank_metrics, metrics.py, pipelines.test(metrics="device")):
against sklearn 1.7, against exact integer / Fraction values, run-to-run and alone-versus-batch determinism, the LDS tier against the
radix tier, error reporting, and the pipelines against their sklearn default."""
import ctypes as C
import warnings
from fractions import Fraction

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CAP = 16384                      # include/tlcgnn.h TLC_RANK_LDS_CAP
PATTERNS = ["random", "q3", "q17", "q1000", "equal", "zeros", "denormal", "saturated"]


def _scores(pattern, n, rs, dtype):
    if pattern == "random":
        s = rs.rand(n)
    elif pattern.startswith("q"):                       # heavy ties: values quantised to a few levels
        s = rs.randint(0, int(pattern[1:]), n) / float(pattern[1:])
    elif pattern == "equal":
        s = np.full(n, 0.37)
    elif pattern == "zeros":                            # only -0.0 / +0.0: one threshold
        s = np.where(rs.rand(n) < 0.5, -0.0, 0.0)
    elif pattern == "denormal":
        tiny = np.finfo(dtype).smallest_subnormal
        s = rs.randint(-5, 6, n) * tiny
    elif pattern == "saturated":                        # sigmoid outputs next to 0 and 1 in f32
        lv = np.array([0.0, np.float32(1e-45), np.float32(1e-38), np.nextafter(np.float32(1), np.float32(0)), 1.0,
                       np.nextafter(np.float32(0.5), np.float32(1)), 0.5])
        s = lv[rs.randint(0, len(lv), n)]
    else:
        raise ValueError(pattern)
    return np.asarray(s, dtype=dtype)


def _labels(n, rs, frac=0.5):
    y = (rs.rand(n) < frac).astype(np.int64)
    if n >= 2 and y.min() == y.max():
        y[0], y[-1] = 1, 0
    return y


def _to_label_tensor(torch, y, kind):
    t = torch.from_numpy(y)
    t = {"uint8": t.to(torch.uint8), "bool": t.to(torch.bool), "int64": t, "float32": t.float()}[kind]
    return t.cuda()


def _exact(s, y):
    """(U2, P, N, (p_g, tp_g, fp_g)): the tie groups of the scores in descending order, exact integers."""
    s64 = np.asarray(s, dtype=np.float64) + 0.0          # -0.0 -> +0.0
    _, inv = np.unique(-s64, return_inverse=True)
    G = inv.max() + 1 if len(inv) else 0
    p = np.bincount(inv[y == 1], minlength=G).astype(np.int64)
    q = np.bincount(inv[y == 0], minlength=G).astype(np.int64)
    tp, fp = np.cumsum(p), np.cumsum(q)
    P, N = int(tp[-1]), int(fp[-1])
    U2 = int(np.sum(p * (2 * (N - fp) + q)))
    return U2, P, N, (p, tp, fp)


def _exact_ap(groups, P):
    p, tp, fp = groups
    acc = Fraction(0)
    for pg, t, f in zip(p.tolist(), tp.tolist(), fp.tolist()):
        if pg:
            acc += Fraction(pg * t, t + f)
    return acc / P


def _same_bits(torch, a, b):
    """torch.equal on the bits: NaN outputs (one class, empty) compare equal to themselves."""
    if a.dtype == torch.float64:
        a, b = a.view(torch.int64), b.view(torch.int64)
    return a.shape == b.shape and torch.equal(a, b)


def _run(torch, s, y, label_kind="int64", force_radix=False):
    from tlc_gnn_amd import ops
    st = torch.from_numpy(s).cuda()
    yt = _to_label_tensor(torch, y, label_kind)
    outs = [ops.binary_rank_metrics(st, yt, force_radix=force_radix) for _ in range(3)]
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert _same_bits(torch, a, b), "not bit-identical run to run"
    auc, ap, npos, nneg, status = (t.cpu() for t in outs[0])
    return float(auc[0]), float(ap[0]), int(npos[0]), int(nneg[0]), int(status[0])


def _check_case(torch, s, y, label_kind, force_radix=False, fraction=None):
    from sklearn.metrics import roc_auc_score, average_precision_score
    n = len(s)
    auc, ap, npos, nneg, status = _run(torch, s, y, label_kind, force_radix)
    assert status == 0
    U2, P, N, groups = _exact(s, y)
    assert (npos, nneg) == (P, N)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sk_auc, sk_ap = roc_auc_score(y, s), average_precision_score(y, s)
    tol = 1e-12 if n <= 10 ** 5 else 1e-10
    if P == 0 or N == 0:
        assert np.isnan(auc) and np.isnan(sk_auc)
        assert ap == (0.0 if P == 0 else 1.0) == sk_ap
        return auc, ap
    assert auc == U2 / (2 * P * N), (auc, U2, P, N)          # bit-equal: one correctly rounded division
    assert abs(auc - sk_auc) <= tol, (auc, sk_auc)
    assert abs(ap - sk_ap) <= tol, (ap, sk_ap)
    if fraction is None:
        fraction = n <= 2000
    if fraction:
        want = _exact_ap(groups, P)
        assert abs(Fraction(ap) - want) <= Fraction(1, 10 ** 15) * want, (ap, float(want))
    return auc, ap


SIZES = [1, 2, 63, 64, 65, CAP - 1, CAP, CAP + 1, 10 ** 5]


@pytest.mark.parametrize("n", SIZES)
def test_against_sklearn_and_exact_values(n):
    """Every pattern at n, f32 and f64 scores, the label dtypes in rotation; AUC bit-equal to U2 / (2 P N) with Python integers,
    AP within 1e-15 relative of Fractions (n <= 2 000 always; two cases of 20 000 in the next test)."""
    import torch
    rs = np.random.RandomState(n)
    kinds = ["uint8", "bool", "int64", "float32"]
    for k, pattern in enumerate(PATTERNS):
        for j, dtype in enumerate([np.float32, np.float64]):
            s = _scores(pattern, n, rs, dtype)
            y = _labels(n, rs, frac=0.3 if k % 2 else 0.5)
            _check_case(torch, s, y, kinds[(k + j) % 4])


def test_fraction_ap_at_20000():
    import torch
    rs = np.random.RandomState(20000)
    for pattern, dtype in [("random", np.float32), ("q1000", np.float64)]:
        _check_case(torch, _scores(pattern, 20000, rs, dtype), _labels(20000, rs), "float32", fraction=True)


@pytest.mark.parametrize("n", [10 ** 6, 1 << 24])
def test_against_sklearn_large(n):
    import torch
    rs = np.random.RandomState(7)
    cases = [("random", np.float32, "float32"), ("q1000", np.float64, "uint8")]
    if n == 10 ** 6:
        cases += [("q3", np.float32, "int64"), ("saturated", np.float32, "bool"), ("random", np.float64, "int64")]
    for pattern, dtype, kind in cases:
        _check_case(torch, _scores(pattern, n, rs, dtype), _labels(n, rs), kind)


@pytest.mark.parametrize("n", [1, 2, 100, CAP, CAP + 1, 10 ** 5])
def test_single_class(n):
    """Only negatives: AUC NaN, AP 0.0; only positives: AUC NaN, AP 1.0 (sklearn 1.7), both tiers."""
    import torch
    rs = np.random.RandomState(3)
    s = _scores("q17", n, rs, np.float32)
    for val, want_ap in [(0, 0.0), (1, 1.0)]:
        y = np.full(n, val, dtype=np.int64)
        for fr in (False, True):
            auc, ap, npos, nneg, status = _run(torch, s, y, "int64", force_radix=fr)
            assert status == 0 and np.isnan(auc) and ap == want_ap and (npos, nneg) == ((0, n) if val == 0 else (n, 0))


def test_tiers_agree():
    """TLC_RANK_FORCE_RADIX: AUC and counts bit-equal to the LDS tier, AP within 1e-15 relative."""
    import torch
    rs = np.random.RandomState(11)
    for n in [1, 2, 65, 777, 4432, CAP]:
        for pattern in PATTERNS:
            for dtype in (np.float32, np.float64):
                s, y = _scores(pattern, n, rs, dtype), _labels(n, rs)
                a = _run(torch, s, y)
                b = _run(torch, s, y, force_radix=True)
                assert a[0] == b[0] or (np.isnan(a[0]) and np.isnan(b[0]))
                assert a[2:] == b[2:]
                assert abs(a[1] - b[1]) <= 1e-15 * abs(a[1])


def test_segment_alone_equals_segment_in_a_batch():
    """Both tiers in one call: each segment's five outputs bit-equal to the segment scored alone."""
    import torch
    from tlc_gnn_amd import ops
    rs = np.random.RandomState(5)
    sizes = [3, 70000, 4432, 1, CAP, CAP + 1, 20000, 64]
    for dtype in (np.float32, np.float64):
        segs = [(_scores(PATTERNS[i % len(PATTERNS)], n, rs, dtype), _labels(n, rs)) for i, n in enumerate(sizes)]
        s = torch.from_numpy(np.concatenate([a for a, _ in segs])).cuda()
        y = torch.from_numpy(np.concatenate([b for _, b in segs]).astype(np.float32)).cuda()
        ptr = np.concatenate([[0], np.cumsum(sizes)])
        batch = ops.binary_rank_metrics(s, y, ptr)
        again = ops.binary_rank_metrics(s, y, torch.from_numpy(ptr))
        for a, b in zip(batch, again):
            assert _same_bits(torch, a, b)
        for i in range(len(sizes)):
            alone = ops.binary_rank_metrics(s[ptr[i]:ptr[i + 1]], y[ptr[i]:ptr[i + 1]])
            for a, b in zip(batch, alone):
                assert _same_bits(torch, a[i:i + 1], b), (i, sizes[i])


def test_metrics_module_matches_sklearn_and_raises_like_it():
    import torch
    from sklearn.metrics import roc_auc_score, average_precision_score
    from tlc_gnn_amd import metrics
    rs = np.random.RandomState(9)
    s, y = _scores("q17", 5000, rs, np.float32), _labels(5000, rs)
    st, yt = torch.from_numpy(s).cuda(), torch.from_numpy(y).cuda()
    auc, ap = metrics.roc_auc_ap(yt, st)
    assert auc == metrics.roc_auc_score(yt, st) and ap == metrics.average_precision_score(yt, st)
    assert abs(auc - roc_auc_score(y, s)) <= 1e-12 and abs(ap - average_precision_score(y, s)) <= 1e-12
    assert isinstance(auc, float) and isinstance(ap, float)
    with pytest.warns(UserWarning, match="Only one class"):
        assert np.isnan(metrics.roc_auc_score(torch.zeros(4, device="cuda"), st[:4]))
    with pytest.warns(UserWarning, match="No positive class"):
        assert metrics.average_precision_score(torch.zeros(4, device="cuda"), st[:4]) == 0.0
    for n in (10, 10 ** 5):                             # LDS and radix tiers
        for bad in (float("nan"), float("inf"), float("-inf")):
            sb = torch.rand(n, device="cuda")
            sb[n // 2] = bad
            with pytest.raises(ValueError, match="NaN or infinity"):
                metrics.roc_auc_score(torch.ones(n, device="cuda").bernoulli_(0.5), sb)
        yb = torch.zeros(n, dtype=torch.int64, device="cuda")
        yb[n // 3] = 2
        with pytest.raises(ValueError, match="only 0 and 1"):
            metrics.average_precision_score(yb, torch.rand(n, device="cuda"))
        with pytest.raises(ValueError, match="only 0 and 1"):
            metrics.roc_auc_ap(torch.full((n,), 0.5, device="cuda"), torch.rand(n, device="cuda"))
    with pytest.raises(ValueError, match="empty"):
        metrics.roc_auc_score(torch.zeros(0, device="cuda"), torch.zeros(0, device="cuda"))


def test_abi_rejects_malformed_seg_ptr():
    import torch
    from tlc_gnn_amd import _lib, ops
    L = _lib.lib()
    s = torch.rand(10, device="cuda")
    y = torch.zeros(10, dtype=torch.uint8, device="cuda")
    out = torch.empty(8, dtype=torch.float64, device="cuda")
    st = torch.empty(2, dtype=torch.int32, device="cuda")
    for bad in ([0, 6, 4], [-1, 5], [3, 2]):
        sp = np.asarray(bad, dtype=np.int64)
        hp = sp.ctypes.data_as(C.c_void_p)
        assert L.tlc_binary_rank_metrics_work_bytes(hp, len(sp) - 1, 0, 0) == -1
        rc = L.tlc_binary_rank_metrics(_lib.ptr(s), 0, _lib.ptr(y), 0, hp, C.c_int32(len(sp) - 1), 0, _lib.ptr(out), _lib.ptr(out[2:]),
                                       _lib.ptr(out[4:]), _lib.ptr(out[6:]), _lib.ptr(st), None, 0, _lib.stream_ptr())
        assert rc == 1                                   # TLC_ERR_INVALID_ARG
        with pytest.raises(ValueError, match="seg_ptr"):
            ops.binary_rank_metrics(s, y, bad)
    sp = np.asarray([0, 10], dtype=np.int64)
    rc = L.tlc_binary_rank_metrics(_lib.ptr(s), 5, _lib.ptr(y), 0, sp.ctypes.data_as(C.c_void_p), 1, 0, _lib.ptr(out), _lib.ptr(out[2:]),
                                   _lib.ptr(out[4:]), _lib.ptr(out[6:]), _lib.ptr(st), None, 0, _lib.stream_ptr())
    assert rc == 4                                       # TLC_ERR_UNSUPPORTED: an unknown score dtype
    torch.cuda.synchronize()


def _pipeline_setup():
    """The 300-node graph of test_gpu_dropins.py::test_pipelines_test_and_train_forward."""
    import torch
    from tlc_gnn_amd import synth, pipelines
    from tlc_gnn_amd.baselines import TLCGNN
    from tlc_gnn_amd.data import Data
    n, m, F_ = 300, 900, 48
    edges = synth.holme_kim_edges(n, m, triad_p=0.5, seed=5)
    ei = torch.from_numpy(np.concatenate([edges, edges[:, ::-1]]).T.copy()).long()
    x = torch.from_numpy(synth.synthetic_features(n, F_, seed=5))
    rs = np.random.RandomState(2)
    E = 1200
    pairs = rs.randint(0, n, size=(E, 2))
    PI = rs.uniform(0, 0.3, size=(E, 25))
    y = torch.from_numpy((rs.rand(E) < 0.5).astype(np.int64))
    data = Data(x=x.clone(), edge_index=ei.clone(), y=torch.zeros(n), total_edges=pairs, total_edges_y=y,
                train_pos=300, train_neg=400, val_pos=100, val_neg=100, test_pos=150, test_neg=150)
    pipelines.setup_seed(3)
    model = TLCGNN.Net(data, F_, 2, PI=PI)
    model.apply(pipelines.weights_init)
    return model.cuda(), data.to("cuda")


def _same_numbers(a, b):
    assert len(a) == len(b)
    assert abs(float(a[0]) - float(b[0])) <= 1e-6
    for u, v in zip(a[1:], b[1:]):
        assert type(u) is type(v)
        assert abs(u - v) <= 1e-12, (u, v)


def test_pipelines_test_device_equals_default():
    import torch
    from tlc_gnn_amd import pipelines
    model, data = _pipeline_setup()
    want = pipelines.test(model, data)
    got = pipelines.test(model, data, metrics="device")
    assert isinstance(got[0], torch.Tensor) and got[0].dtype == want[0].dtype and got[0].device == want[0].device
    assert got[0].shape == want[0].shape
    _same_numbers(got, want)
    assert pipelines.test(model, data, metrics="device") == got
    with pytest.raises(ValueError):
        pipelines.test(model, data, metrics="cpu")


def test_pipelines_fit_device_equals_default():
    """Seeded fit runs with each metrics path: the same early-stopping decisions, the same tuple within the bounds."""
    import torch
    from tlc_gnn_amd import pipelines
    res = {}
    for metrics in ("sklearn", "device"):
        model, data = _pipeline_setup()
        opt = torch.optim.Adam(model.parameters(), lr=0.01)
        pipelines.setup_seed(7)
        res[metrics] = pipelines.fit(model, data, opt, total_epochs=40, wait_total=5, metrics=metrics)
    a, b = res["device"], res["sklearn"]
    for u, v in zip(a[:4], b[:4]):
        assert type(u) is type(v) and abs(u - v) <= 1e-12, (a, b)
    assert abs(float(a[4]) - float(b[4])) <= 1e-6

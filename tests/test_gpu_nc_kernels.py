"""GPU: the kernels of nc_curv.hip one by one (tlc_nc_group, tlc_nc_linear_f32 / _bwd_f32, tlc_nc_curv_fwd_f32 / _bwd_f32), called through
ops.nc_* and the C ABI, against plain f64 restatements on the CPU (torch float64 with autograd, PyG's softmax as
oracle/lp_forward_ref.segment_softmax) -- at the edges of their parameter space: the 1024-node chunks of the scan, the 16-blocks of
the MFMA, the 64-edge tiles of the edge MLP, C and D at 1 and at their limits, logits beyond expf's range, PReLU at z == 0, E = 0.
test_gpu_nc_curv.py tests the module built on these kernels; this file is the net under the kernels themselves."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch


# ---- 1. grouping ------------------------------------------------------------------------------------------------------------------
GROUP_PARTS = ("src_ptr", "tgt_ptr", "src_eid", "tgt_eid", "src", "dst")


def _split_groups(g, n, E):
    cuts = np.cumsum([0, n + 1, n + 1, E, E, E, E])
    assert len(g) == cuts[-1]
    return {k: g[cuts[i]:cuts[i + 1]] for i, k in enumerate(GROUP_PARTS)}


def _want_groups(ei, n):
    """The stable sort the header promises: rows by node id, ascending edge id inside a row."""
    src, dst = ei[0], ei[1]
    ptr = lambda v: np.concatenate([[0], np.cumsum(np.bincount(v, minlength=n))])          # noqa: E731
    return {"src_ptr": ptr(src), "tgt_ptr": ptr(dst), "src_eid": np.argsort(src, kind="stable"), "tgt_eid": np.argsort(dst, kind="stable"),
            "src": src, "dst": dst}


def _chunk_border_nodes(n):
    """The nodes on both sides of every 1024-node chunk edge of the scan, and the last node."""
    nodes = {n - 1}
    for edge in range(1024, n + 2, 1024):
        nodes.update(v for v in (edge - 2, edge - 1, edge, edge + 1) if 0 <= v < n)
    return sorted(nodes)


def _group_graph(n, seed):
    """Random edges + a node of out-degree 3000 and one of in-degree 3000 (the last two ids: beyond every chunk edge) + a few edges
    out of and into every node beside a chunk edge and the last node + duplicates + self loops, in shuffled order."""
    rs = np.random.RandomState(seed)
    border = np.array(_chunk_border_nodes(n))
    parts = [np.stack([rs.randint(0, n, 2000), rs.randint(0, n, 2000)]),
             np.stack([np.full(3000, max(n - 2, 0)), rs.randint(0, n, 3000)]),
             np.stack([rs.randint(0, n, 3000), np.full(3000, n - 1)]),
             np.stack([np.repeat(border, 3), rs.randint(0, n, 3 * len(border))]),
             np.stack([rs.randint(0, n, 2 * len(border)), np.repeat(border, 2)])]
    parts.append(parts[0][:, :50])                                                           # duplicates
    loops = np.arange(0, n, max(1, n // 40))
    parts.append(np.stack([loops, loops]))
    ei = np.concatenate(parts, axis=1)
    return ei[:, rs.permutation(ei.shape[1])].astype(np.int64)


def _check_groups(torch, ei, n):
    from tlc_gnn_amd import ops
    E = ei.shape[1]
    d_ei = torch.from_numpy(ei).cuda()
    g = ops.nc_group(d_ei, n)
    assert g.dtype == torch.int32
    got, want = _split_groups(g.cpu().numpy(), n, E), _want_groups(ei, n)
    for k in GROUP_PARTS:
        assert np.array_equal(got[k], want[k]), (n, E, k)
    assert torch.equal(g, ops.nc_group(d_ei, n)), (n, E)        # the counting atomics' order does not reach the result


@pytest.mark.parametrize("n", [1, 2, 1023, 1024, 1025, 2049, 5000])
def test_group_is_a_stable_sort_across_scan_chunks(n):
    torch = _torch()
    ei = _group_graph(n, seed=n)
    out_deg, in_deg = np.bincount(ei[0], minlength=n), np.bincount(ei[1], minlength=n)
    assert out_deg.max() >= 3000 and in_deg.max() >= 3000
    for v in _chunk_border_nodes(n):
        assert out_deg[v] >= 3 and in_deg[v] >= 2, v
    assert int((ei[0] == ei[1]).sum()) > 0 and (n == 1 or not np.array_equal(np.sort(ei[0], kind="stable"), ei[0]))
    _check_groups(torch, ei, n)


@pytest.mark.parametrize("n", [1, 7, 1025])
@pytest.mark.parametrize("E", [0, 1])
def test_group_of_no_edge_and_of_one_edge(E, n):
    torch = _torch()
    _check_groups(torch, np.zeros((2, 0), dtype=np.int64) if E == 0 else np.array([[n - 1], [0]], dtype=np.int64), n)
    if E == 1:
        _check_groups(torch, np.array([[0], [n - 1]], dtype=np.int64), n)


# ---- 2. projection ----------------------------------------------------------------------------------------------------------------
def _close(got, want, rtol, atol_frac):
    """test_gpu_lp_train._close: allclose with an atol of atol_frac of the largest wanted entry."""
    import torch
    atol = atol_frac * float(want.abs().max()) if want.numel() else 0.0
    ok = torch.allclose(got.to(want.dtype), want, rtol=rtol, atol=atol)
    return ok, float((got.to(want.dtype) - want).abs().max()) if want.numel() else 0.0


@pytest.mark.parametrize("K", [1, 3, 4, 15, 16, 17, 500, 745])
@pytest.mark.parametrize("N", [1, 3, 16, 63, 64, 65, 256])
@pytest.mark.parametrize("M", [0, 1, 63, 64, 65, 300])
def test_linear_odd_shapes_and_deterministic(M, N, K):
    """y = x W^T (+ b), gx = gy W, gw = gy^T x, gb = 1^T gy against the f64 products: the criterion and the numbers of
    test_gemm_tn_odd_shapes_and_deterministic (rtol 1e-4, atol 1e-5 of the largest entry); every call twice, the same bits."""
    torch = _torch()
    from tlc_gnn_amd import ops
    rs = np.random.RandomState(100000 * M + 1000 * N + K)
    x, w, b, gy = (torch.from_numpy(rs.randn(*s).astype(np.float32)) for s in ((M, K), (N, K), (N,), (M, N)))
    dx, dw, db, dgy = x.cuda(), w.cuda(), b.cuda(), gy.cuda()
    for bias in (None, db):
        y = ops.nc_linear(dx, dw, bias)
        want = x.double() @ w.double().t() + (b.double() if bias is not None else 0.0)
        ok, err = _close(y.cpu().double(), want, 1e-4, 1e-5)
        assert tuple(y.shape) == (M, N) and ok, (M, N, K, bias is not None, err)
        assert torch.equal(y, ops.nc_linear(dx, dw, bias)), (M, N, K)
    want = {"gx": gy.double() @ w.double(), "gw": gy.double().t() @ x.double(), "gb": gy.double().sum(0)}
    for need_gx in (True, False):
        got = dict(zip(("gx", "gw", "gb"), ops.nc_linear_bwd(dx, dw, dgy, need_gx=need_gx)))
        again = dict(zip(("gx", "gw", "gb"), ops.nc_linear_bwd(dx, dw, dgy, need_gx=need_gx)))
        assert (got["gx"] is not None) == need_gx
        for k, v in got.items():
            if v is None:
                continue
            ok, err = _close(v.cpu().double(), want[k], 1e-4, 1e-5)
            assert tuple(v.shape) == tuple(want[k].shape) and ok, (M, N, K, k, need_gx, err)
            assert torch.equal(v, again[k]), (M, N, K, k)
        if M == 0:                                                 # sums over no row: exact zeros, not whatever the buffers held
            assert bool((got["gw"] == 0).all()) and bool((got["gb"] == 0).all())


@pytest.mark.parametrize("K", [1, 3, 4, 15, 16, 17, 31, 32, 33, 500, 745])
def test_linear_small_integers_are_exact(K):
    """Integers in [-4, 4]: every product and every partial sum is an integer below 2^24, exact in f32 in any order.  The results
    are bit-equal to the f64 products; a k dropped or counted twice at the edge of a 16-block is off by a whole number."""
    torch = _torch()
    from tlc_gnn_amd import ops
    M, N = 300, 65
    rs = np.random.RandomState(K)
    x, w, b, gy = (torch.from_numpy(rs.randint(-4, 5, s).astype(np.float32)) for s in ((M, K), (N, K), (N,), (M, N)))
    assert 16 * max(K, M, N) + 4 < 2 ** 24
    y = ops.nc_linear(x.cuda(), w.cuda(), b.cuda())
    assert torch.equal(y.cpu().double(), x.double() @ w.double().t() + b.double())
    gx, gw, gb = ops.nc_linear_bwd(x.cuda(), w.cuda(), gy.cuda())
    assert torch.equal(gx.cpu().double(), gy.double() @ w.double())
    assert torch.equal(gw.cpu().double(), gy.double().t() @ x.double())
    assert torch.equal(gb.cpu().double(), gy.double().sum(0))


# ---- 3. / 4. the edge MLP, the softmax and the gather: inputs and the restatement ----------------------------------------------------
# Out-degrees of nodes 0, 1, 2, ...: the by-source order of the edges is this list laid end to end.  Positions (NC_T = 64):
#   63 [0, 63) | 65 [63, 128): crosses 64, ends on 128 | 64 [128, 192): one whole aligned tile | 128 [192, 320): aligned, no row starts
#   in [256, 320) | 10 [320, 330) | 200 [330, 530): in four aligned tiles, its last one shared with the rows that follow |
#   runs of rows of 1 and 0 edges, a 17, a 3, a 30 | the last row, which ends at E.
HEAD = [63, 65, 64, 128, 10, 200]
MID = [1, 1, 1, 0, 0, 1, 0, 1, 17, 3, 1, 0, 0, 0, 1, 1, 30]
LAST = {0: 52, 1: 53, 63: 51}                                     # E % 64 -> length of the last row
ROW_64, ROW_17 = 2, len(HEAD) + 8                                 # the nodes of the aligned row of 64 and of the row of 17
TAILS = (0, 1, 63)


def _tile_graph(tail, seed=0):
    """-> (edge_index int64 [2,E] in shuffled edge order, n, out-degree per node).  Targets are random; nodes 1, 7 and n - 2 have no
    in-edge; the last six nodes have no out-edge (n - 2: no edge at all)."""
    degs = np.array(HEAD + MID + [LAST[tail]] + [0] * 6)
    n, start = len(degs), np.concatenate([[0], np.cumsum(degs)])
    E = int(start[-1])
    assert start[:7].tolist() == [0, 63, 128, 192, 320, 330, 530] and E % 64 == tail and degs[ROW_17] == 17 and degs[ROW_64] == 64
    assert start[n - 6] == E and degs[n - 7] == LAST[tail]           # the last row ends at E
    rs = np.random.RandomState(seed)
    src = np.repeat(np.arange(n), degs)
    allowed = np.setdiff1d(np.arange(n), [1, 7, n - 2])
    dst = allowed[rs.randint(0, len(allowed), E)]
    ei = np.stack([src, dst])[:, rs.permutation(E)].astype(np.int64)
    assert not np.array_equal(np.argsort(ei[0], kind="stable"), np.arange(E))               # src_eid is not the identity
    return ei, n, degs


def _random_graph(E, n=12, seed=0):
    rs = np.random.RandomState(seed)
    return np.stack([rs.randint(0, n - 2, E), rs.randint(0, n - 2, E)]).astype(np.int64)


def _inputs(torch, E, n, Cc, D, seed, slopes=(0.05, 0.4)):
    """The parameter scale of test_gpu_nc_curv.py: Linear's default init (uniform, 1 / sqrt(fan_in)), b2 in (-0.3, 0.3), w_mul in
    (0, 0.5), xl ~ N(0, 1).  f32 CPU tensors."""
    rs = np.random.RandomState(seed)
    p = {"xl": rs.randn(n, Cc), "w_mul": rs.uniform(0, 0.5, (E, D)), "w1": rs.uniform(-1, 1, (Cc, D)) / np.sqrt(D),
         "a": rs.uniform(slopes[0], slopes[1], Cc), "w2": rs.uniform(-1, 1, (Cc, Cc)) / np.sqrt(Cc), "b2": rs.uniform(-0.3, 0.3, Cc),
         "gout": rs.randn(n, Cc)}
    return {k: torch.from_numpy(v.astype(np.float32)) for k, v in p.items()}


def _ref(torch, p, ei, n, dtype, grad=False):
    """curvGN after the projection (ConvCurv_GIN.py:163-170) in `dtype` on the CPU -> (out, alpha, wt, the leaves it was computed from)."""
    import torch.nn.functional as F
    from oracle import lp_forward_ref as ref
    q = {k: v.to(dtype).clone().requires_grad_(grad and k not in ("w_mul", "gout")) for k, v in p.items()}
    ei = torch.as_tensor(ei)
    wt = F.linear(F.prelu(F.linear(q["w_mul"], q["w1"]), q["a"]), q["w2"], q["b2"])
    alpha = ref.segment_softmax(wt, ei[0], n)
    out = torch.zeros((n, q["xl"].shape[1]), dtype=dtype).index_add(0, ei[1], alpha * q["xl"][ei[0]])
    return out, alpha, wt, q


GRADS = ("xl", "w1", "a", "w2", "b2")


def _ref_grads(torch, p, ei, n, dtype):
    """autograd of the restatement -> ({name: gradient}, d wt)."""
    out, _, wt, q = _ref(torch, p, ei, n, dtype, grad=True)
    wt.retain_grad()
    out.backward(q["gout"])
    return {k: q[k].grad for k in GRADS}, wt.grad


def _gpu_fwd(torch, p, ei, n):
    from tlc_gnn_amd import ops
    d = {k: v.cuda() for k, v in p.items()}
    groups = ops.nc_group(torch.as_tensor(ei).cuda(), n)
    out, alpha = ops.nc_curv_fwd(groups, d["xl"], d["w_mul"], d["w1"], d["a"], d["w2"], d["b2"])
    return groups, d, out, alpha


def _gpu_bwd(torch, groups, d, alpha):
    from tlc_gnn_amd import ops
    return dict(zip(GRADS, ops.nc_curv_bwd(groups, d["xl"], d["w_mul"], d["w1"], d["a"], d["w2"], alpha, d["gout"])))


def _frac(got, want):
    """The largest error as a fraction of the largest wanted entry."""
    return float((got.cpu().double() - want.double()).abs().max()) / max(float(want.double().abs().max()), 1e-300)


def _check_fwd(torch, p, ei, n, degs=None):
    """out and alpha within 1e-5 of the largest wanted entry (the bound of test_gpu_nc_curv.py); rows of one edge: alpha == 1 exactly;
    nodes without in-edge: zero rows; a second call: the same bits."""
    from tlc_gnn_amd import ops
    groups, d, out, alpha = _gpu_fwd(torch, p, ei, n)
    with torch.no_grad():
        want_out, want_alpha, _, _ = _ref(torch, p, ei, n, torch.float64)
    E, Cc = ei.shape[1], p["xl"].shape[1]
    assert tuple(out.shape) == (n, Cc) and tuple(alpha.shape) == (E, Cc)
    e_out, e_alpha = _frac(out, want_out), _frac(alpha, want_alpha)
    assert e_out <= 1e-5 and e_alpha <= 1e-5, (Cc, p["w_mul"].shape[1], E, e_out, e_alpha)
    out_deg, in_deg = np.bincount(ei[0], minlength=n), np.bincount(ei[1], minlength=n)
    single = torch.from_numpy(out_deg[ei[0]] == 1)
    assert bool((alpha.cpu()[single] == 1.0).all())
    assert bool((out.cpu()[torch.from_numpy(in_deg == 0)] == 0).all())
    out2, alpha2 = ops.nc_curv_fwd(groups, d["xl"], d["w_mul"], d["w1"], d["a"], d["w2"], d["b2"])
    assert torch.equal(out, out2) and torch.equal(alpha, alpha2)
    return groups, d, out, alpha


@pytest.mark.parametrize("tail", TAILS)
@pytest.mark.parametrize("C", [1, 3, 4, 15, 16, 17, 63, 64, 65, 252, 255, 256])
def test_fwd_channels_at_tile_edges(C, tail):
    torch = _torch()
    ei, n, _ = _tile_graph(tail, seed=C)
    _check_fwd(torch, _inputs(torch, ei.shape[1], n, C, 50, seed=1000 + C), ei, n)


@pytest.mark.parametrize("tail", TAILS)
@pytest.mark.parametrize("C", [7, 64])
@pytest.mark.parametrize("D", [1, 15, 16, 17, 33, 63, 64])
def test_fwd_mul_width_at_tile_edges(D, C, tail):
    torch = _torch()
    ei, n, _ = _tile_graph(tail, seed=D)
    _check_fwd(torch, _inputs(torch, ei.shape[1], n, C, D, seed=2000 + 100 * D + C), ei, n)


def _large_logit_inputs(torch, Cc, seed):
    """The inputs of test_fwd_channels_at_tile_edges with W1 and W2 scaled (PReLU is positively homogeneous: wt - b2 scales with the
    product) so that the largest |wt| is about 170: between 100 and 250, and beyond expf's f32 range (88.7) with either sign, on the
    rows that span chunks as well as on the rows inside one."""
    ei, n, degs = _tile_graph(1, seed=seed)
    p = _inputs(torch, ei.shape[1], n, Cc, 50, seed=3000 + Cc)
    with torch.no_grad():
        _, _, wt, _ = _ref(torch, p, ei, n, torch.float64)
        s = float(np.sqrt(170.0 / float((wt - p["b2"].double()).abs().max())))
        p["w1"], p["w2"] = p["w1"] * s, p["w2"] * s
        _, _, wt, _ = _ref(torch, p, ei, n, torch.float64)
    spans = torch.from_numpy(degs[ei[0]] > 64)
    for part in (wt[spans], wt[~spans]):
        assert 100.0 <= float(part.abs().max()) <= 250.0 and float(part.max()) > 89.0 and float(part.min()) < -89.0
    return p, ei, n, degs


@pytest.mark.parametrize("C", [7, 64, 252, 256])
def test_fwd_large_logits_need_the_row_maximum(C):
    """max|wt| between 100 and 250: without the row maximum expf overflows (or every term underflows).  The bound is measured, not
    fixed: the f32 CPU restatement's own error against f64 on these inputs, times four (the kernel is f32 like the restatement but
    forms z and wt on the MFMA in another order of k); an error of the kind this case is after is infinite, NaN or of order one.
    The restatement's own error is at most 2e-5, else the inputs no longer tell a right kernel from a wrong one."""
    torch = _torch()
    p, ei, n, degs = _large_logit_inputs(torch, C, seed=C)
    _, _, out, alpha = _gpu_fwd(torch, p, ei, n)
    with torch.no_grad():
        want_out, want_alpha, _, _ = _ref(torch, p, ei, n, torch.float64)
        f32_out, f32_alpha, _, _ = _ref(torch, p, ei, n, torch.float32)
    ref_out, ref_alpha = _frac(f32_out, want_out), _frac(f32_alpha, want_alpha)
    got_out, got_alpha = _frac(out, want_out), _frac(alpha, want_alpha)
    print("large logits C=%d: out f32 restatement %.3g kernel %.3g | alpha f32 restatement %.3g kernel %.3g"
          % (C, ref_out, got_out, ref_alpha, got_alpha))
    assert ref_out <= 2e-5, ref_out
    a = alpha.cpu().double()
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(out).all())
    assert float(a.min()) >= 0.0 and float(a.max()) <= 1.0
    sums = torch.zeros((n, C), dtype=torch.float64).index_add_(0, torch.from_numpy(ei[0]), a)
    has = torch.from_numpy(degs > 0)
    tol = 64 * EPS32 * torch.from_numpy(degs[degs > 0]).double().view(-1, 1)
    assert bool(((sums[has] - 1.0).abs() <= tol).all()), float((sums[has] - 1.0).abs().max())
    # four times the restatement's error.  Observed, out: restatement 8.7e-7 to 3.1e-6, kernel 8.9e-7 to 4.8e-6 of the largest entry (at
    # most 1.7 times the restatement's); alpha: restatement 6.2e-6 to 1.2e-5, kernel 9.5e-6 to 1.9e-5 (at most 1.7 times)
    assert got_out <= 4 * ref_out, (C, got_out, ref_out)
    assert got_alpha <= 4 * ref_alpha, (C, got_alpha, ref_alpha)


def _prelu_inputs(torch, ei, n, Cc, D, seed):
    """Slopes of either sign, every fifth exactly 0; w_mul rows exactly zero: every edge of the aligned row of 64, every edge of the row
    of 17, and one edge in ten elsewhere."""
    p = _inputs(torch, ei.shape[1], n, Cc, D, seed, slopes=(-0.4, 0.4))
    p["a"][::5] = 0.0
    rs = np.random.RandomState(seed + 1)
    zero = (ei[0] == ROW_64) | (ei[0] == ROW_17) | (rs.rand(ei.shape[1]) < 0.1)
    p["w_mul"][torch.from_numpy(zero)] = 0.0
    assert bool((p["a"] < 0).any()) and bool((p["a"] > 0).any())
    return p


@pytest.mark.parametrize("C", [7, 64, 255])
def test_fwd_prelu_slopes_of_either_sign_and_zero_rows(C):
    torch = _torch()
    ei, n, degs = _tile_graph(63, seed=C)
    p = _prelu_inputs(torch, ei, n, C, 50, seed=4000 + C)
    _, _, _, alpha = _check_fwd(torch, p, ei, n)
    # a zero w_mul row: z == 0, h == 0, wt == b2.  A source row made of such edges only: exp(0) = 1 on every edge, the sum is the
    # degree (exact), alpha = 1 / degree up to the division's one rounding
    for node in (ROW_64, ROW_17):
        a = alpha.cpu().double()[torch.from_numpy(ei[0] == node)]
        assert a.shape[0] == degs[node]
        assert float((a - 1.0 / degs[node]).abs().max()) <= EPS32 / degs[node], (node, float((a - 1.0 / degs[node]).abs().max()))


@pytest.mark.parametrize("C", [5, 64])
def test_fwd_without_edges_is_zero(C):
    torch = _torch()
    n = 9
    ei = np.zeros((2, 0), dtype=np.int64)
    p = _inputs(torch, 0, n, C, 50, seed=C)
    assert tuple(p["w_mul"].shape) == (0, 50)
    _, _, out, alpha = _gpu_fwd(torch, p, ei, n)
    assert tuple(out.shape) == (n, C) and bool((out == 0).all()) and tuple(alpha.shape) == (0, C)


@pytest.mark.parametrize("C", [17, 64])
def test_fwd_same_alpha_whatever_the_edge_order(C):
    """The same graph with its edge list permuted: another order inside every source row (rows hold ascending edge ids), other tile
    rows for every edge.  wt does not depend on the tile row and the row maximum not on the order; the sum of exp does: two orders
    of a sum of `len` non-negative f32 terms differ by at most (len - 1) eps of it, the two divisions add one rounding each -- 2 len
    eps covers that to second order."""
    torch = _torch()
    ei, n, degs = _tile_graph(63, seed=C)
    p = _inputs(torch, ei.shape[1], n, C, 50, seed=5000 + C)
    _, _, out, alpha = _check_fwd(torch, p, ei, n)
    perm = np.random.RandomState(C).permutation(ei.shape[1])
    ei2, p2 = ei[:, perm], dict(p, w_mul=p["w_mul"][torch.from_numpy(perm)].contiguous())
    _, _, out2, alpha2 = _check_fwd(torch, p2, ei2, n)
    a, a2 = alpha.cpu().double()[torch.from_numpy(perm)], alpha2.cpu().double()
    tol = 2 * EPS32 * torch.from_numpy(degs[ei2[0]]).double().view(-1, 1) * a
    assert bool(((a - a2).abs() <= tol).all()), float(((a - a2).abs() / a).max())
    assert not torch.equal(a, a2)                                  # (the order did change something: the case is not vacuous)


# ---- 4. backward ------------------------------------------------------------------------------------------------------------------
def _excess(got, want, scale):
    """The worst excess of |got - want| over 1e-4 |want|, as a fraction of `scale`."""
    d = (got.cpu().double() - want.double()).abs() - 1e-4 * want.double().abs()
    return max(float(d.max()), 0.0) / scale if scale > 0 else float((got.cpu().double() != want.double()).any())


def _scales(want, dwt):
    """The criterion of test_layer_backward_matches_autograd: the gradient's largest entry; d b2 = sum_e d wt[e] vanishes per source
    row (softmax), its scale is the size of the terms it sums."""
    return {k: float(dwt.abs().sum(0).max()) if k == "b2" else float(want[k].abs().max()) for k in GRADS}


BWD_ATOL = 2e-6                    # of the gradient's scale, beside rtol 1e-4 (observed: at most 5.9e-7 of it)
BWD_INPUT_ATOL = BWD_ATOL          # what the f32 CPU restatement has to keep on the same inputs: the criterion itself


def _check_bwd(torch, p, ei, n):
    """Element-wise rtol 1e-4 plus BWD_ATOL of the gradient's scale; a second call: the same bits.  A condition on the inputs comes
    first: the f32 CPU restatement itself keeps the criterion, i.e. a right f32 computation can pass (every
    gradient here is a sum of terms that cancel within a source row; where the largest entry of one is itself such a remainder, no
    f32 computation keeps 2e-6 of it, and the case would tell nothing)."""
    want, dwt = _ref_grads(torch, p, ei, n, torch.float64)
    f32, _ = _ref_grads(torch, p, ei, n, torch.float32)
    scales = _scales(want, dwt)
    for k in GRADS:
        ref_ex = _excess(f32[k], want[k], scales[k])
        assert ref_ex <= BWD_INPUT_ATOL, ("ill-conditioned inputs", k, tuple(p["w1"].shape), ei.shape[1], ref_ex)
    groups, d, _, alpha = _gpu_fwd(torch, p, ei, n)
    got = _gpu_bwd(torch, groups, d, alpha)
    again = _gpu_bwd(torch, groups, d, alpha)
    worst = {}
    for k in GRADS:
        assert tuple(got[k].shape) == tuple(want[k].shape), k
        worst[k] = _excess(got[k], want[k], scales[k])
        assert torch.equal(got[k], again[k]), k
    print("bwd C=%d D=%d E=%d: excess over rtol 1e-4 | %s" % (tuple(p["w1"].shape) + (ei.shape[1], " ".join("%s %.2g" % kv for kv in worst.items()))))
    for k in GRADS:
        assert worst[k] <= BWD_ATOL, (k, tuple(p["w1"].shape), ei.shape[1], worst[k], scales[k])
    return got, want


BWD_SHAPES = [(1, 1), (1, 50), (3, 17), (3, 64), (17, 1), (17, 50), (64, 17), (64, 64), (255, 50), (255, 64), (256, 1), (256, 17), (256, 50)]


# C = 1: d W2 and d prelu have ONE entry each, a sum over the edges whose terms cancel within every source row.  At some draws that
# entry is a small remainder of its terms and the f32 CPU restatement itself misses the criterion by a factor of 100; these draws
# are ones at which it keeps it (the condition _check_bwd asserts), found with the restatement alone.
BWD_DRAW = {(1, 1): 1, (1, 50): 2}


@pytest.mark.parametrize("C,D", BWD_SHAPES)
def test_bwd_shapes_at_tile_edges(C, D):
    torch = _torch()
    ei, n, _ = _tile_graph(TAILS[BWD_SHAPES.index((C, D)) % 3], seed=C + D)
    _check_bwd(torch, _inputs(torch, ei.shape[1], n, C, D, seed=6000 + 100 * D + C + 7919 * BWD_DRAW.get((C, D), 0)), ei, n)


@pytest.mark.parametrize("C,D", [(64, 50), (3, 17)])
@pytest.mark.parametrize("E", [1, 63, 64, 65, 128])
def test_bwd_edge_counts_around_a_tile(E, C, D):
    """The backward's edge tiles are in edge order: 64 edges each, whatever the rows."""
    torch = _torch()
    n = 12
    ei = _random_graph(E, n, seed=E)
    p = _inputs(torch, E, n, C, D, seed=7000 + E)
    _check_fwd(torch, p, ei, n)
    _check_bwd(torch, p, ei, n)


@pytest.mark.parametrize("C", [17, 64])
def test_bwd_prelu_at_zero_takes_the_slope(C):
    """Negative and zero slopes, zero w_mul rows, and three channels whose row of W1 is exactly zero: z == 0 on every edge of such a
    channel.  torch's PReLU sends the gradient through the slope there (z > 0 ? g : a g) and gives the slope itself none (z g = 0):
    d W1 of such a row is the slope times sum_e dh m, d prelu of it is zero.  (A zero w_mul row alone multiplies its own dz by zero.)"""
    torch = _torch()
    ei, n, _ = _tile_graph(0, seed=C)
    p = _prelu_inputs(torch, ei, n, C, 50, seed=8000 + C)
    zc = [1, 6, C - 1]
    p["w1"][zc] = 0.0
    p["a"][zc] = torch.tensor([0.3, -0.25, 0.15])
    got, want = _check_bwd(torch, p, ei, n)
    for c in zc:
        assert float(want["w1"][c].abs().max()) > 1e-3 * float(want["w1"].abs().max()), c      # the rows under test carry a gradient
        assert float(want["a"][c]) == 0.0 and float(got["a"][c]) == 0.0, c
    assert float(want["a"].abs().max()) > 0.0


@pytest.mark.parametrize("C,D", [(5, 50), (64, 17)])
def test_bwd_without_edges_is_zero(C, D):
    torch = _torch()
    n = 9
    p = _inputs(torch, 0, n, C, D, seed=C)
    groups, d, _, alpha = _gpu_fwd(torch, p, np.zeros((2, 0), dtype=np.int64), n)
    got = _gpu_bwd(torch, groups, d, alpha)
    assert tuple(got["xl"].shape) == (n, C) and tuple(got["w1"].shape) == (C, D) and tuple(got["w2"].shape) == (C, C)
    for k in GRADS:
        assert bool((got[k] == 0).all()), k


# the kernel may exceed rtol 1e-4 by four times what the f32 CPU restatement exceeds it by on the same inputs.  Observed (worst of the
# five gradients, as a fraction of the gradient's scale), restatement / kernel: C = 7: 2.8e-6 / 8.0e-6; C = 64: 3.9e-6 / 4.9e-6;
# C = 252: 7.7e-6 / 7.1e-6; C = 256: 4.3e-6 / 1.3e-5 -- the kernel at most 3.0 times the restatement
LARGE_LOGIT_FACTOR = 4.0


@pytest.mark.parametrize("C", [7, 64, 252, 256])
def test_bwd_large_logits(C):
    """The inputs of test_fwd_large_logits_need_the_row_maximum.  BWD_ATOL does not carry over: at max|wt| of 100 to 250 an f32
    computation that is right already exceeds rtol 1e-4 by more than 2e-6 of the largest entry.  So the atol of this one case is
    measured: the f32 CPU restatement's worst excess over 1e-4 |want| (f64), each gradient's as a fraction of that gradient's scale,
    the worst of the five -- one figure in the place of the one BWD_ATOL -- times LARGE_LOGIT_FACTOR: the kernel is f32 like that
    restatement but sums the edges of a row and the split-K partials in another order.  The yardstick is the restatement, never
    the kernel's own output.  (Not gradient by gradient: an excess is what is left of an error after 1e-4 |want| is taken off, and
    where the restatement's error happens to stay just above that line its excess says little about the size of a right error; on
    the first run d W2 at C = 64 came out at 4.9e-6 of its scale against a restatement at 1.2e-6 of it, while d W1 of the same call
    stood at 4.3e-6 against 3.9e-6.)"""
    torch = _torch()
    p, ei, n, _ = _large_logit_inputs(torch, C, seed=C)
    groups, d, _, alpha = _gpu_fwd(torch, p, ei, n)
    got = _gpu_bwd(torch, groups, d, alpha)
    again = _gpu_bwd(torch, groups, d, alpha)
    want, dwt = _ref_grads(torch, p, ei, n, torch.float64)
    f32, _ = _ref_grads(torch, p, ei, n, torch.float32)
    scales = _scales(want, dwt)
    ref_ex = {k: _excess(f32[k], want[k], scales[k]) for k in GRADS}
    ex = {k: _excess(got[k], want[k], scales[k]) for k in GRADS}
    print("large logits C=%d: excess over rtol 1e-4 | %s" % (C, " | ".join("%s f32 restatement %.3g kernel %.3g" % (k, ref_ex[k], ex[k]) for k in GRADS)))
    atol = LARGE_LOGIT_FACTOR * max(ref_ex.values())
    for k in GRADS:
        assert bool(torch.isfinite(got[k]).all()), k
        assert ex[k] <= atol, (C, k, ex[k], atol)
        assert torch.equal(got[k], again[k]), k


# ---- 5. misuse is a return code ---------------------------------------------------------------------------------------------------
INVALID_ARG, UNSUPPORTED = 1, 4


def test_misuse_returns_a_code_before_any_launch():
    """Every call below is refused by the host checks of the entry point: nothing is launched, the outputs keep what they held.  Every
    pointer is a live buffer large enough for the sizes named in the call."""
    torch = _torch()
    from tlc_gnn_amd import _lib
    L = _lib.lib()
    n, E, CM, DM = 4, 3, 257, 65
    f = lambda *s: torch.full(s, 7.0, dtype=torch.float32, device="cuda")                   # noqa: E731
    groups = torch.zeros(2 * (n + 1) + 4 * E, dtype=torch.int32, device="cuda")
    xl, wmul, w1, a, w2, b2, alpha, out, gout = f(n, CM), f(E, DM), f(CM, DM), f(CM), f(CM, CM), f(CM), f(E, CM), f(n, CM), f(n, CM)
    gxl, gw1, ga, gw2, gb2 = f(n, CM), f(CM, DM), f(CM), f(CM, CM), f(CM)
    nbytes = 4 * (3 * E * CM + CM + 32 * CM * CM)
    work = torch.full((nbytes,), 7, dtype=torch.uint8, device="cuda")
    ptr, st = _lib.ptr, _lib.stream_ptr()
    outputs = (alpha, out, gxl, gw1, ga, gw2, gb2)

    def fwd(n_, E_, C_, D_):
        return L.tlc_nc_curv_fwd_f32(n_, E_, C_, D_, ptr(groups), ptr(xl), ptr(wmul), ptr(w1), ptr(a), ptr(w2), ptr(b2), ptr(alpha), ptr(out), st)

    def bwd(n_, E_, C_, D_, nb=nbytes):
        return L.tlc_nc_curv_bwd_f32(n_, E_, C_, D_, ptr(groups), ptr(xl), ptr(wmul), ptr(w1), ptr(a), ptr(w2), ptr(alpha), ptr(gout), ptr(gxl),
                                     ptr(gw1), ptr(ga), ptr(gw2), ptr(gb2), ptr(work), nb, st)

    for call, name in ((fwd, b"tlc_nc_curv_fwd_f32"), (bwd, b"tlc_nc_curv_bwd_f32")):
        for sizes in ((0, E, 8, 5), (n, E, 0, 5), (n, E, 8, 0), (n, -1, 8, 5)):
            assert call(*sizes) == INVALID_ARG, (name, sizes)
            assert name in L.tlc_last_error()
        for sizes in ((n, E, 257, 5), (n, E, 8, 65)):
            assert call(*sizes) == UNSUPPORTED, (name, sizes)
            assert name in L.tlc_last_error()
    need = int(L.tlc_nc_curv_work_bytes(n, E, 8, 5))
    assert 0 < need <= nbytes
    assert bwd(n, E, 8, 5, need - 1) == INVALID_ARG
    assert b"tlc_nc_curv_bwd_f32" in L.tlc_last_error() and b"tlc_nc_curv_work_bytes" in L.tlc_last_error()
    x, w, y, gw = f(n, 6), f(5, 6), f(n, 5), f(5, 6)
    lin_work = f(32 * 5 * 6)
    for N_, K_ in ((0, 6), (5, 0)):
        assert L.tlc_nc_linear_f32(n, N_, K_, ptr(x), ptr(w), None, ptr(y), st) == INVALID_ARG
        assert b"tlc_nc_linear_f32" in L.tlc_last_error()
        assert L.tlc_nc_linear_bwd_f32(n, N_, K_, ptr(x), ptr(w), ptr(y), None, ptr(gw), None, ptr(lin_work), st) == INVALID_ARG
        assert b"tlc_nc_linear_bwd_f32" in L.tlc_last_error()
    ei = torch.zeros((2, E), dtype=torch.int64, device="cuda")
    gwork = torch.full((2 * n + 4 * E,), 7, dtype=torch.int32, device="cuda")
    bad = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    for n_, E_ in ((0, E), (n, -1)):
        assert L.tlc_nc_group(n_, E_, ptr(ei), ptr(groups), ptr(gwork), ptr(bad), st) == INVALID_ARG
        assert b"tlc_nc_group" in L.tlc_last_error()
    torch.cuda.synchronize()
    for t in outputs + (y, gw):
        assert bool((t == 7.0).all())
    assert bool((groups == 0).all()) and int(bad.item()) == 7


def test_wrapper_passes_on_the_refusal_of_257_channels():
    """ops.nc_curv_fwd does not check C itself: the library refuses, and the error that comes out names the limit."""
    torch = _torch()
    from tlc_gnn_amd import _lib, ops
    n, Cc, D = 6, 257, 50
    ei = _random_graph(5, n, seed=1)
    p = _inputs(torch, 5, n, Cc, D, seed=1)
    groups = ops.nc_group(torch.from_numpy(ei).cuda(), n)
    with pytest.raises(_lib.TlcError, match=r"tlc_nc_curv_fwd_f32: TLC_ERR_UNSUPPORTED .*C = 257 \(max 256\)"):
        ops.nc_curv_fwd(groups, p["xl"].cuda(), p["w_mul"].cuda(), p["w1"].cuda(), p["a"].cuda(), p["w2"].cuda(), p["b2"].cuda())
    with pytest.raises(ValueError, match="1..256"):
        ops.nc_curv_bwd(groups, p["xl"].cuda(), p["w_mul"].cuda(), p["w1"].cuda(), p["a"].cuda(), p["w2"].cuda(),
                        torch.zeros((5, Cc), device="cuda"), p["gout"].cuda())

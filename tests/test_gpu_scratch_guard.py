"""GPU: the entries that take a bare d_work pointer write nowhere behind the count their size function returns
(tlc_*_work_floats / tlc_*_work_ints over csrc/scratch_layouts.h).  Each entry runs through the raw C ABI with d_work carved out of a
larger tensor at exactly that count, followed by 256 guard elements of a fixed bit pattern inside the same allocation; afterwards the
guard holds the pattern and the outputs have the bits of the same call through the ops wrapper.  The shapes are the smallest that
reach every path of the carving (the rank-1 / two-product / fused-weights / narrow / per-node forms of the layer, both row strides
of its backward, the splits of gemm_tn, the pad4 gaps of the encoder, ...).

tlc_gat_layer_bwd and tlc_edge_head_bwd add with float atomics, so two calls agree in every bit only where no sum depends on the order
of its terms; their inputs are built for that (see _bwd_graph and _dyadic)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 256
PATTERN = 0x5A5AA5A5            # as float32 1.5e16: scratch read before it is written would show in the outputs


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch


class Guarded:
    """`count` elements of scratch (float32, or int32 with ints=True) with GUARD elements of PATTERN behind them, in one tensor."""

    def __init__(self, size_fn, sizes, ints=False):
        torch = _torch()
        from tlc_gnn_amd import _lib
        self.count = getattr(_lib.lib(), size_fn)(*sizes)
        assert self.count >= 0, (size_fn, sizes)
        self.buf = torch.full((self.count + GUARD,), PATTERN, dtype=torch.int32, device="cuda")
        self.work = self.buf[:self.count] if ints else self.buf[:self.count].view(torch.float32)
        self.ptr = C.c_void_p(self.buf.data_ptr())

    def guard_intact(self):
        return bool((self.buf[self.count:] == PATTERN).all())

    def untouched(self):
        return bool((self.buf == PATTERN).all())


def _same_bits(got, want):
    torch = _torch()
    assert got.shape == want.shape and got.dtype == want.dtype
    return torch.equal(got.contiguous().view(torch.int32), want.contiguous().view(torch.int32))


def _randn(shape, seed, scale=0.5):
    torch = _torch()
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).cuda()


def _dyadic(shape, seed, denom=4, span=8):
    """Multiples of 1 / denom in [-span / denom, span / denom]: products and sums of a few hundred of them are exact in float32, so
    a sum of such terms has the same bits in every order."""
    torch = _torch()
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-span, span + 1, shape, generator=g).float() / denom).cuda()


def _ring_csr(n):
    """CSR by target of a ring with self loops: row i = sorted {i - 1, i, i + 1} mod n."""
    torch = _torch()
    rows = [sorted({(i - 1) % n, i, (i + 1) % n}) for i in range(n)]
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    return torch.from_numpy(rowptr).cuda(), torch.from_numpy(np.concatenate(rows).astype(np.int32)).cuda()


def _block_batch(sizes):
    """edge_index int64 [2, E] of a block-diagonal batch of path graphs, both directions, no self loops."""
    torch = _torch()
    parts, off = [], 0
    for nn in sizes:
        a = np.arange(nn - 1) + off
        parts += [np.stack([a, a + 1]), np.stack([a + 1, a])]
        off += nn
    return off, torch.from_numpy(np.concatenate(parts, axis=1).astype(np.int64)).cuda()


BATCHES = {"193 nodes in 5-node graphs": [5] * 38 + [3], "one 31-node graph": [31]}


# ---- the PDGNN layer ---------------------------------------------------------------------------------------------------------------
def _layer_params(c_in, c_out, n, seed):
    return (_randn((n, c_in), seed), _randn((c_out, c_in), seed + 1), _randn((c_out,), seed + 2), _randn((c_out, 2 * c_out), seed + 3, 0.3),
            _randn((2 * c_out,), seed + 4, 0.1))


@pytest.mark.parametrize("c_in,c_out,n", [(1, 32, 135),       # the rank-1 vector
                                          (64, 32, 135),      # two products: n C < c_in (2 C + 4)
                                          (64, 32, 136),      # fused weights, Wf in the x_l region: n C >= c_in (2 C + 4)
                                          (3, 16, 135),       # the narrow x_l kernel
                                          (64, 64, 135)])     # no MFMA layout: node rows of 3 C + 1 floats
def test_gat_layer_fwd(c_in, c_out, n):
    torch = _torch()
    from tlc_gnn_amd import _lib, ops
    rowptr, src = _ring_csr(n)
    x, wl, att, wij, bias = _layer_params(c_in, c_out, n, 10 * c_in + c_out)
    want = ops.gat_layer(rowptr, src, x, wl, att, wij, bias, prelu_slope=0.1)
    g = Guarded("tlc_gat_layer_fwd_work_floats", (n, c_in, c_out))
    got = torch.empty_like(want)
    rc = _lib.lib().tlc_gat_layer_fwd(n, _lib.ptr(rowptr), _lib.ptr(src), _lib.ptr(x), c_in, c_out, _lib.ptr(wl), _lib.ptr(att), _lib.ptr(wij),
                                      _lib.ptr(bias), 0.1, g.ptr, _lib.ptr(got), _lib.stream_ptr())
    _lib.check(rc, "tlc_gat_layer_fwd")
    torch.cuda.synchronize()
    assert g.guard_intact()
    assert _same_bits(got, want)


@pytest.mark.parametrize("c_in,c_out", [(1, 32), (64, 16)])
def test_gat_layer_tiled_fwd(c_in, c_out):
    torch = _torch()
    from tlc_gnn_amd import _lib, ops
    n, ei = _block_batch(BATCHES["193 nodes in 5-node graphs"])
    rowptr, col = ops.csr_by_target(ei, n)
    tiles = ops.gat_tiles(rowptr, col, n)
    assert tiles is not None and tiles.numel() > 2
    x, wl, att, wij, bias = _layer_params(c_in, c_out, n, 7 * c_in + c_out)
    want = ops.gat_layer_tiled(rowptr, col, tiles, x, wl, att, wij, bias, prelu_slope=0.1)
    g = Guarded("tlc_gat_layer_tiled_fwd_work_floats", (c_in, c_out))
    got = torch.empty_like(want)
    rc = _lib.lib().tlc_gat_layer_tiled_fwd(n, _lib.ptr(rowptr), _lib.ptr(col), tiles.numel() - 1, _lib.ptr(tiles), _lib.ptr(x), c_in, c_out,
                                            _lib.ptr(wl), _lib.ptr(att), _lib.ptr(wij), _lib.ptr(bias), 0.1, g.ptr, _lib.ptr(got),
                                            _lib.stream_ptr())
    _lib.check(rc, "tlc_gat_layer_tiled_fwd")
    torch.cuda.synchronize()
    assert g.guard_intact()
    assert _same_bits(got, want)


def _bwd_graph(n):
    """A CSR by target on which tlc_gat_layer_bwd's atomic sums have at most two terms each, whatever the order of the wavefronts.
    Twelve targets have two in-edges each from 24 sources of their own, so a source's gQ row and gAlpha get one term and a target's
    gAlpha one.  All 36 sit at node ids with id % 32 < 16: xty_kernel's four row groups take rows 0-7, 8-15, 16-23, 24-31 of every
    32 and each adds its partial sum to the weight gradients atomically -- here two of the four are zero.  (d bias sums the rows of
    d out from many workgroups: the test gives d out integer values, whose sums are exact.)  n = 1: one node with its self loop."""
    torch = _torch()
    if n == 1:
        return torch.tensor([0, 1], dtype=torch.int32).cuda(), torch.tensor([0], dtype=torch.int32).cuda()
    live = [i for i in range(n) if i % 32 < 16]
    assert len(live) >= 36
    rows = {live[t]: sorted((live[12 + 2 * t], live[13 + 2 * t])) for t in range(12)}
    rowptr = np.concatenate([[0], np.cumsum([len(rows.get(i, ())) for i in range(n)])]).astype(np.int32)
    src = np.array([s for i in range(n) for s in rows.get(i, ())], dtype=np.int32)
    return torch.from_numpy(rowptr).cuda(), torch.from_numpy(src).cuda()


@pytest.mark.parametrize("n", [1, 70])
@pytest.mark.parametrize("c_in,c_out", [(64, 32), (3, 32),      # rows by the MFMA product, stride 2 C + 4
                                        (64, 64), (3, 64)])     # per-node rows, stride 2 C + 1
def test_gat_layer_bwd(c_in, c_out, n):
    torch = _torch()
    from tlc_gnn_amd import _lib, ops
    rowptr, src = _bwd_graph(n)
    x, wl, att, wij, _ = _layer_params(c_in, c_out, n, 3 * c_in + c_out + n)
    gout = _dyadic((n, 2 * c_out), 5, denom=1, span=3)
    want = ops.gat_layer_bwd(rowptr, src, x, wl, att, wij, -1.0, None, gout)
    g = Guarded("tlc_gat_layer_bwd_work_floats", (n, c_in, c_out))
    got = [torch.empty_like(t) for t in want]
    rc = _lib.lib().tlc_gat_layer_bwd(n, _lib.ptr(rowptr), _lib.ptr(src), _lib.ptr(x), c_in, c_out, _lib.ptr(wl), _lib.ptr(att), _lib.ptr(wij),
                                      -1.0, None, _lib.ptr(gout), *[_lib.ptr(t) for t in got], g.ptr, _lib.stream_ptr())
    _lib.check(rc, "tlc_gat_layer_bwd")
    torch.cuda.synchronize()
    assert g.guard_intact()
    for name, a, b in zip(("gX", "gWl", "gatt", "gWij", "gbias"), got, want):
        assert _same_bits(a, b), name
    if n > 1:
        assert all(bool(t.abs().sum() > 0) for t in got)


# ---- the edge head -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,hidden,uses_scratch", [(16, 32, True), (32, 32, False)])          # (32, 32): the MFMA kernel, no scratch
def test_edge_head_fwd(c, hidden, uses_scratch):
    torch = _torch()
    from tlc_gnn_amd import _lib, ops
    n, E = 50, 300
    rs = np.random.RandomState(c)
    src = torch.from_numpy(rs.randint(0, n, E).astype(np.int32)).cuda()
    dst = torch.from_numpy(rs.randint(0, n, E).astype(np.int32)).cuda()
    x, w5, b5, w6, b6 = _randn((n, c), 1), _randn((hidden, 2 * c), 2), _randn((hidden,), 3), _randn((2, hidden), 4), _randn((2,), 5)
    want = ops.edge_head(src, dst, x, w5, b5, 0.1, w6, b6)
    g = Guarded("tlc_edge_head_fwd_work_floats", (n, c, hidden))
    got = torch.empty_like(want)
    rc = _lib.lib().tlc_edge_head_fwd(E, _lib.ptr(src), _lib.ptr(dst), _lib.ptr(x), c, _lib.ptr(w5), _lib.ptr(b5), hidden, 0.1, _lib.ptr(w6),
                                      _lib.ptr(b6), _lib.ptr(got), n, g.ptr, _lib.stream_ptr())
    _lib.check(rc, "tlc_edge_head_fwd")
    torch.cuda.synchronize()
    assert g.guard_intact()
    assert g.untouched() != uses_scratch
    assert _same_bits(got, want)


@pytest.mark.parametrize("E", [1, 300])
def test_edge_head_bwd(E):
    """Dyadic inputs and a PReLU slope of 1/4: every product and sum of this backward is exact, so its atomics commute."""
    torch = _torch()
    from tlc_gnn_amd import _lib, ops
    n, c, hidden = max(E, 2), 16, 32
    src = torch.arange(E, dtype=torch.int32).cuda()
    dst = ((torch.arange(E) + 1) % n).to(torch.int32).cuda()
    x, w5, b5, w6, gpd = _dyadic((n, c), 1), _dyadic((hidden, 2 * c), 2), _dyadic((hidden,), 3), _dyadic((2, hidden), 4), _dyadic((E, 2), 5)
    want = ops.edge_head_bwd(src, dst, x, w5, b5, 0.25, w6, gpd)
    g = Guarded("tlc_edge_head_bwd_work_floats", (E, c, hidden))
    got = [torch.zeros_like(want[0])] + [torch.empty_like(t) for t in want[1:]]
    rc = _lib.lib().tlc_edge_head_bwd(E, _lib.ptr(src), _lib.ptr(dst), _lib.ptr(x), c, _lib.ptr(w5), _lib.ptr(b5), hidden, 0.25, _lib.ptr(w6),
                                      _lib.ptr(gpd), *[_lib.ptr(t) for t in got], g.ptr, _lib.stream_ptr())
    _lib.check(rc, "tlc_edge_head_bwd")
    torch.cuda.synchronize()
    assert g.guard_intact()
    for name, a, b in zip(("gX", "gW5", "gb5", "gW6", "gb6"), got, want):
        assert _same_bits(a, b), name
    assert all(bool(t.abs().sum() > 0) for t in got)


# ---- the batch's structure -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", sorted(BATCHES))
def test_csr_by_target_and_tile_cut(batch):
    torch = _torch()
    from tlc_gnn_amd import _lib, ops
    L = _lib.lib()
    n, ei = _block_batch(BATCHES[batch])
    E = ei.shape[1]
    want_rowptr, want_col = ops.csr_by_target(ei, n)
    g = Guarded("tlc_csr_by_target_work_ints", (n, E), ints=True)
    rowptr = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    col = torch.empty(E + n, dtype=torch.int32, device="cuda")
    nnz = torch.empty(1, dtype=torch.int32, device="cuda")
    _lib.check(L.tlc_csr_by_target(n, E, _lib.ptr(ei), _lib.ptr(rowptr), _lib.ptr(col), _lib.ptr(nnz), g.ptr, _lib.stream_ptr()), "tlc_csr_by_target")
    torch.cuda.synchronize()
    assert g.guard_intact()
    k = int(nnz.item())
    assert k == E + n == int(rowptr[-1])
    assert torch.equal(rowptr, want_rowptr) and torch.equal(col[:k], want_col[:k])
    # the cut: d_work and d_tile_ptr both at their counts, both guarded
    want_tiles = ops.gat_tiles(rowptr, col, n)
    assert want_tiles is not None
    g = Guarded("tlc_gat_tile_cut_work_ints", (n,), ints=True)
    t = Guarded("tlc_gat_tile_cut_max_tiles", (n, ops.GAT_TILE_NODES), ints=True)
    nt = C.c_int32(0)
    _lib.check(L.tlc_gat_tile_cut(n, _lib.ptr(rowptr), _lib.ptr(col), ops.GAT_TILE_NODES, g.ptr, t.ptr, C.byref(nt), _lib.stream_ptr()), "tlc_gat_tile_cut")
    assert g.guard_intact() and t.guard_intact()
    assert nt.value + 1 == want_tiles.numel() <= t.count
    assert torch.equal(t.work[:nt.value + 1], want_tiles)


# ---- link prediction and node classification ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K,splits,column_sums", [(5, 5, 7937, 32, False),      # 32 splits: the whole scratch
                                                      (5, 5, 10, 1, False),         # one split: straight into C
                                                      (1, 5, 7937, 32, True)])      # d_A NULL
def test_gemm_tn(M, N, K, splits, column_sums):
    torch = _torch()
    from tlc_gnn_amd import _lib, ops
    a, b = (None if column_sums else _randn((K, M), 1)), _randn((K, N), 2)
    want = ops.gemm_tn(a, b)
    g = Guarded("tlc_gemm_tn_work_floats", (M, N))
    got = torch.empty_like(want)
    _lib.check(_lib.lib().tlc_gemm_tn_f32(M, N, K, _lib.ptr(a), _lib.ptr(b), _lib.ptr(got), g.ptr, _lib.stream_ptr()), "tlc_gemm_tn_f32")
    torch.cuda.synchronize()
    assert g.guard_intact()
    if splits == 1:
        assert g.untouched()
    else:
        assert bool((g.buf[:g.count] != PATTERN).all())                 # splits * M * N partials: all of it
    assert _same_bits(got, want)


@pytest.mark.parametrize("N,K", [(7, 3), (3, 7)])
def test_nc_linear_bwd(N, K):
    torch = _torch()
    from tlc_gnn_amd import _lib, ops
    M = 8000
    x, w, gy = _randn((M, K), 1), _randn((N, K), 2), _randn((M, N), 3)
    want = ops.nc_linear_bwd(x, w, gy)
    g = Guarded("tlc_nc_linear_bwd_work_floats", (N, K))
    got = [torch.empty_like(t) for t in want]
    rc = _lib.lib().tlc_nc_linear_bwd_f32(M, N, K, _lib.ptr(x), _lib.ptr(w), _lib.ptr(gy), *[_lib.ptr(t) for t in got], g.ptr, _lib.stream_ptr())
    _lib.check(rc, "tlc_nc_linear_bwd_f32")
    torch.cuda.synchronize()
    assert g.guard_intact()
    for name, a, b in zip(("gx", "gw", "gb"), got, want):
        assert _same_bits(a, b), name


@pytest.mark.parametrize("n_pairs", [1, 129, 70000])             # one tile, two, more tiles than the 512 workgroups
def test_lp_decode_bwd(n_pairs):
    torch = _torch()
    from tlc_gnn_amd import _lib, ops
    n = 50
    rs = np.random.RandomState(n_pairs)
    pairs = torch.from_numpy(rs.randint(0, n, (n_pairs, 2)).astype(np.int32)).cuda()
    emb_pre = _randn((n, 16), 1, 0.4)
    emb = ops.renorm_rows_(emb_pre.clone())
    pi, w1, b1, w2, b2 = _randn((n_pairs, 25), 2).abs(), _randn((25, 41), 3, 0.3), _randn((25,), 4, 0.1), _randn((1, 25), 5, 0.3), _randn((1,), 6, 0.1)
    gprob = _randn((n_pairs,), 7)
    groups = ops.endpoint_groups(pairs, n)
    want = ops.lp_decode_bwd(pairs, emb_pre, emb, pi, w1, b1, w2, b2, gprob, groups=groups)
    g = Guarded("tlc_lp_decode_bwd_work_floats", (n_pairs,))
    gemb = torch.empty((n, 16), dtype=torch.float32, device="cuda")
    gw = torch.empty(1076, dtype=torch.float32, device="cuda")
    rc = _lib.lib().tlc_lp_decode_bwd_f32(n_pairs, _lib.ptr(pairs), _lib.ptr(emb_pre), _lib.ptr(emb), n, 16, _lib.ptr(pi), 25, _lib.ptr(w1), _lib.ptr(b1),
                                          _lib.ptr(w2.reshape(-1)), _lib.ptr(b2), _lib.ptr(gprob), _lib.ptr(groups[0]), _lib.ptr(groups[1]),
                                          _lib.ptr(gemb), _lib.ptr(gw), g.ptr, _lib.stream_ptr())
    _lib.check(rc, "tlc_lp_decode_bwd_f32")
    torch.cuda.synchronize()
    assert g.guard_intact()
    assert _same_bits(gemb, want[0])
    assert _same_bits(gw, torch.cat([t.reshape(-1) for t in want[1:]]))


@pytest.mark.parametrize("hidden,out_dim,n", [(6, 16, 3),        # n hidden = 18: both pad4 gaps are two floats wide
                                              (32, 16, 37),      # conv2's projection in conv1's epilogue: three kernels
                                              (32, 7, 37)])      # four kernels
def test_gcn2_encode(hidden, out_dim, n):
    torch = _torch()
    from tlc_gnn_amd import _lib, ops
    f_in = 8
    _, ei = _block_batch([n])
    rowptr, col, val = ops.gcn_norm_csr(ei, n)
    x, w1, b1, w2, b2 = _randn((n, f_in), 1), _randn((f_in, hidden), 2), _randn((hidden,), 3, 0.1), _randn((hidden, out_dim), 4), _randn((out_dim,), 5, 0.1)
    want = ops.gcn2_encode(rowptr, col, val, x, w1, b1, w2, b2, relu=True, renorm=True)
    g = Guarded("tlc_gcn2_encode_work_floats", (n, hidden, out_dim))
    got = torch.empty_like(want)
    rc = _lib.lib().tlc_gcn2_encode_f32(n, _lib.ptr(rowptr), _lib.ptr(col), _lib.ptr(val), _lib.ptr(x), f_in, _lib.ptr(w1), _lib.ptr(b1), hidden,
                                        _lib.ptr(w2), _lib.ptr(b2), out_dim, 3, g.ptr, _lib.ptr(got), _lib.stream_ptr())
    _lib.check(rc, "tlc_gcn2_encode_f32")
    torch.cuda.synchronize()
    assert g.guard_intact()
    assert _same_bits(got, want)

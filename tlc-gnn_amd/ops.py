"""Typed wrappers over the LP-forward / PDGNN entry points of the C ABI (include/tlcgnn.h).

torch tensors in, torch tensors out; every call enqueues hand-written HIP kernels on the current stream.
No autograd here: autograd.py connects the backward entry points (gcn_norm_csr_t, gemm_tn, lp_decode_bwd) to loss.backward().
"""
import ctypes as C

from . import _lib


def _f32(t):
    import torch
    assert t.is_cuda and t.dtype == torch.float32, "expected a float32 CUDA tensor"
    return t.contiguous()


def _scratch(size_fn, sizes, dtype, device, extra=0):
    """The scratch of an entry that takes a bare d_work: `size_fn` (its tlc_*_work_floats / tlc_*_work_ints, host arithmetic over
    csrc/scratch_layouts.h, the layout the launch carves) gives the element count (tlc_gat_tile_cut_max_tiles: of an output's room); `extra` elements of the caller's own behind it."""
    import torch
    count = getattr(_lib.lib(), size_fn)(*map(int, sizes))
    if count < 0:
        raise ValueError("%s%r: negative size" % (size_fn, tuple(sizes)))
    return torch.empty(count + extra, dtype=dtype, device=device)


@_lib.on_device_of
def gcn_norm_csr(edge_index, num_nodes):
    """gcn_norm of GCNConv(cached=True) (Knowledge_Distillation/PD_conv.py:35-70) as CSR by target.

    edge_index: int64 CUDA [2,E] (row 0 source, row 1 target).  Returns (rowptr int32[N+1], col int32[nnz], val f32[nnz]).
    """
    torch = _lib.require_gpu()
    assert edge_index.is_cuda and edge_index.dtype == torch.int64 and edge_index.shape[0] == 2
    ei = edge_index.contiguous()
    E = ei.shape[1]
    dev = ei.device
    rowptr = torch.empty(num_nodes + 1, dtype=torch.int32, device=dev)
    col = torch.empty(E + num_nodes, dtype=torch.int32, device=dev)
    val = torch.empty(E + num_nodes, dtype=torch.float32, device=dev)
    nnz = torch.zeros(1, dtype=torch.int32, device=dev)
    rc = _lib.lib().tlc_gcn_norm_csr(C.c_int32(num_nodes), C.c_int64(E), _lib.ptr(ei), _lib.ptr(rowptr), _lib.ptr(col),
                                     _lib.ptr(val), _lib.ptr(nnz), _lib.stream_ptr())
    _lib.check(rc, "tlc_gcn_norm_csr")
    k = int(nnz.item())
    return rowptr, col[:k].contiguous(), val[:k].contiguous()


@_lib.on_device_of
def csr_by_target(edge_index, num_nodes):
    """remove_self_loops + add_self_loops + grouping by target (Knowledge_Distillation/gat_conv.py:146-152), the structure alone:
    (rowptr int32[N+1], col int32[E+N] of which the first rowptr[N] are written).  tlc_csr_by_target: temporaries from the caching
    allocator, no host read -- the per-batch form of gcn_norm_csr (whose one-off build allocates, waits and frees)."""
    torch = _lib.require_gpu()
    assert edge_index.is_cuda and edge_index.dtype == torch.int64 and edge_index.shape[0] == 2
    ei = edge_index.contiguous()
    E, dev = ei.shape[1], ei.device
    rowptr = torch.empty(num_nodes + 1, dtype=torch.int32, device=dev)
    col = torch.empty(E + num_nodes, dtype=torch.int32, device=dev)
    work = _scratch("tlc_csr_by_target_work_ints", (num_nodes, E), torch.int32, dev, extra=1)          # [temporaries | nnz]
    rc = _lib.lib().tlc_csr_by_target(C.c_int32(num_nodes), C.c_int64(E), _lib.ptr(ei), _lib.ptr(rowptr), _lib.ptr(col),
                                      _lib.ptr(work[-1:]), _lib.ptr(work), _lib.stream_ptr())
    _lib.check(rc, "tlc_csr_by_target")
    return rowptr, col


@_lib.on_device_of
def pdgnn_forward(x, edge_index, params, edge_ptr, res=5, hidden=32, rowptr=None, col=None, tiles=None):
    """Teacher_Model.forward(compute_loss=False) without gradients as one library call (tlc_pdgnn_forward): x float32 [n,1],
    edge_index int64 [2, m+n] (self loops last), params = the 20 float32 tensors in the header's order, edge_ptr int64 [B+1]
    -> (points float32 [m,2], images float64 [B, res*res]).  rowptr / col / tiles: the structure of a batch the caller holds."""
    torch = _lib.require_gpu()
    n, E, B = int(x.shape[0]), int(edge_index.shape[1]), int(edge_ptr.numel()) - 1
    ei = edge_index.contiguous()
    L = _lib.lib()
    nbytes = int(L.tlc_pdgnn_forward_work_bytes(C.c_int32(n), C.c_int64(E), C.c_int32(hidden)))
    if nbytes < 0:
        raise ValueError("pdgnn_forward: needs n >= 1 nodes and an edge_index that ends in the n self loops (train_Teacher_Model.py:43-44)")
    work = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    points = torch.empty((E - n, 2), dtype=torch.float32, device=x.device)
    img = torch.empty((max(B, 1), res * res), dtype=torch.float64, device=x.device)
    keep = [_f32(p) for p in params]
    arr = (C.c_void_p * 20)(*[p.data_ptr() for p in keep])
    nt = 0 if tiles is None else tiles.numel() - 1
    rc = L.tlc_pdgnn_forward(C.c_int32(n), C.c_int64(E), _lib.ptr(ei), _lib.ptr(_f32(x)), C.c_int32(hidden), arr, C.c_int64(B),
                             _lib.ptr(edge_ptr.contiguous()), C.c_int32(res), _lib.ptr(rowptr), _lib.ptr(col), _lib.ptr(tiles), C.c_int32(nt),
                             _lib.ptr(work), C.c_int64(nbytes), _lib.ptr(points), _lib.ptr(img), _lib.stream_ptr())
    _lib.check(rc, "tlc_pdgnn_forward")
    return points, img[:B]


@_lib.on_device_of
def gemm(a, b, bias=None, relu=False, out=None):
    """C = A @ B (+bias)(ReLU) on the f32 MFMA; A [M,K], B [K,N<=128] float32 CUDA."""
    torch = _lib.require_gpu()
    a, b = _f32(a), _f32(b)
    M, K = a.shape
    K2, N = b.shape
    assert K == K2
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    rc = _lib.lib().tlc_gemm_f32(C.c_int32(M), C.c_int32(N), C.c_int32(K), _lib.ptr(a), _lib.ptr(b),
                                 _lib.ptr(_f32(bias)) if bias is not None else None, C.c_int(1 if relu else 0),
                                 _lib.ptr(out), _lib.stream_ptr())
    _lib.check(rc, "tlc_gemm_f32")
    return out


class SparseRows:
    """CSR of a feature matrix (the zeros of bag-of-words / TF-IDF features dropped), built once: rowptr int32[M+1],
    col int32[nnz], val f32[nnz] on the matrix's device.  The conversion is a data-format step (torch index plumbing)."""

    def __init__(self, x):
        import torch
        x = _f32(x)
        self.shape = tuple(x.shape)
        nz = x != 0
        counts = nz.sum(dim=1, dtype=torch.int64)
        self.rowptr = torch.zeros(x.shape[0] + 1, dtype=torch.int32, device=x.device)
        self.rowptr[1:] = torch.cumsum(counts, 0).to(torch.int32)
        idx = nz.nonzero(as_tuple=False)                                  # row-major: rows ascending, columns ascending
        self.nnz = int(idx.shape[0])
        if self.nnz:
            self.col = idx[:, 1].to(torch.int32).contiguous()
            self.val = x[nz].contiguous()
        else:                                                              # (an all-zero matrix: the arrays still need an address)
            self.col = torch.zeros(1, dtype=torch.int32, device=x.device)
            self.val = torch.zeros(1, dtype=torch.float32, device=x.device)

    @property
    def density(self):
        return self.nnz / float(max(self.shape[0] * self.shape[1], 1))


SPARSE_GEMM_MAX_K = 636          # a 64-column slice of B in LDS: K * 256 B + 1 KiB <= 160 KiB (narrower slices take more: sparse_gemm_fits)
SPARSE_GEMM_MAX_NNZ = 1 << 29    # the kernel addresses entries by 32-bit BYTE offsets through a buffer descriptor (include/tlcgnn.h)


def _check_sparse_rows(xs):
    """Entries beyond 2^29 would read back as zeros (offsets behind the descriptor's range): refused, never truncated."""
    if xs.nnz >= SPARSE_GEMM_MAX_NNZ:
        raise _lib.TlcError("sparse feature projection: %d stored entries, the kernel takes fewer than 2^29 (use the dense ops.gemm)" % xs.nnz)


def sparse_gemm_fits(k, n):
    """Whether tlc_spgemm_csr_dense_f32 takes a [*, k] @ [k, n] product: its column slice of B ([k][<= 64], equal widths, a
    multiple of four: 52 + 48 for n = 100) and 1 KiB must fit the 160 KiB of LDS."""
    slices = (n + 63) // 64
    sw = (((n + slices - 1) // slices) + 3) & ~3
    return k > 0 and n > 0 and k * sw * 4 + 1024 <= 160 * 1024


@_lib.on_device_of
def sparse_gemm(xs, b, bias=None, relu=False, out=None):
    """C = X @ B (+bias)(ReLU) for X given as SparseRows: the zeros of X cost nothing (tlc_spgemm_csr_dense_f32; fp32 sums in an
    order of its own)."""
    torch = _lib.require_gpu()
    b = _f32(b)
    M, K = xs.shape
    assert b.shape[0] == K
    _check_sparse_rows(xs)
    N = b.shape[1]
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=b.device)
    rc = _lib.lib().tlc_spgemm_csr_dense_f32(C.c_int32(M), C.c_int32(K), C.c_int32(N), _lib.ptr(xs.rowptr), _lib.ptr(xs.col),
                                             _lib.ptr(xs.val), _lib.ptr(b), _lib.ptr(_f32(bias)) if bias is not None else None,
                                             C.c_int(1 if relu else 0), _lib.ptr(out), _lib.stream_ptr())
    _lib.check(rc, "tlc_spgemm_csr_dense_f32")
    return out


@_lib.on_device_of
def spmm(rowptr, col, val, x, bias=None, relu=False, out=None, renorm=False):
    """Y = act(CSR @ X + bias): the normalised scatter-add of GCNConv as a row-owned gather; renorm=True also applies
    emb.renorm_(2, 0, 1) (TLCGNN.py:48) to every output row in the same pass."""
    torch = _lib.require_gpu()
    x = _f32(x)
    n = rowptr.numel() - 1
    k = x.shape[1]
    if out is None:
        out = torch.empty((n, k), dtype=torch.float32, device=x.device)
    rc = _lib.lib().tlc_spmm_csr_f32(C.c_int32(n), _lib.ptr(rowptr), _lib.ptr(col), _lib.ptr(val), _lib.ptr(x), C.c_int32(k),
                                     _lib.ptr(_f32(bias)) if bias is not None else None, C.c_int((1 if relu else 0) | (2 if renorm else 0)),
                                     _lib.ptr(out), _lib.stream_ptr())
    _lib.check(rc, "tlc_spmm_csr_f32")
    return out


_GCN2_WS = {}


def gcn2_encode(rowptr, col, val, x, w1, b1, w2, b2, relu=True, renorm=False, out=None, x_sparse=None):
    """Net.encode in eval mode behind one library call (tlc_gcn2_encode_f32): relu(A (relu(A (x w1) + b1)) w2 + b2), rows
    renormalised when renorm=True (TLCGNN.py:19-26,48).  Same four kernels as gemm / spmm / gemm / spmm; the scratch for
    the intermediates is kept per (device, stream, sizes): two forwards in flight on two streams do not share it.
    x_sparse: SparseRows of x -- the first projection then runs over the stored entries (tlc_gcn2_encode_csr_f32)."""
    torch = _lib.require_gpu()
    w1, w2 = _f32(w1), _f32(w2)
    if x_sparse is None:
        x = _f32(x)
        n, f_in = x.shape[0], x.shape[1]
    else:
        n, f_in = x_sparse.shape
        _check_sparse_rows(x_sparse)
    hidden, d = w1.shape[1], w2.shape[1]
    dev = w1.device
    key = (dev, torch.cuda.current_stream(dev).cuda_stream, n, hidden, d)
    ws = _GCN2_WS.get(key)
    if ws is None:
        if len(_GCN2_WS) >= 4:
            _GCN2_WS.clear()
        ws = _GCN2_WS[key] = _scratch("tlc_gcn2_encode_work_floats", (n, hidden, d), torch.float32, dev)
    if out is None:
        out = torch.empty((n, d), dtype=torch.float32, device=dev)
    flags = C.c_int((1 if relu else 0) | (2 if renorm else 0))
    pb1 = _lib.ptr(_f32(b1)) if b1 is not None else None
    pb2 = _lib.ptr(_f32(b2)) if b2 is not None else None
    with torch.cuda.device(dev):
        if x_sparse is None:
            rc = _lib.lib().tlc_gcn2_encode_f32(C.c_int32(n), _lib.ptr(rowptr), _lib.ptr(col), _lib.ptr(val), _lib.ptr(x), C.c_int32(f_in),
                                                _lib.ptr(w1), pb1, C.c_int32(hidden), _lib.ptr(w2), pb2, C.c_int32(d),
                                                flags, _lib.ptr(ws), _lib.ptr(out), _lib.stream_ptr(dev))
        else:
            rc = _lib.lib().tlc_gcn2_encode_csr_f32(C.c_int32(n), _lib.ptr(rowptr), _lib.ptr(col), _lib.ptr(val), _lib.ptr(x_sparse.rowptr),
                                                    _lib.ptr(x_sparse.col), _lib.ptr(x_sparse.val), C.c_int32(f_in),
                                                    _lib.ptr(w1), pb1, C.c_int32(hidden), _lib.ptr(w2), pb2, C.c_int32(d),
                                                    flags, _lib.ptr(ws), _lib.ptr(out), _lib.stream_ptr(dev))
    _lib.check(rc, "tlc_gcn2_encode_f32" if x_sparse is None else "tlc_gcn2_encode_csr_f32")
    return out


@_lib.on_device_of
def renorm_rows_(emb):
    """emb.renorm_(2, 0, 1) in place (baselines/TLCGNN.py:48)."""
    emb_c = _f32(emb)
    assert emb_c.data_ptr() == emb.data_ptr(), "renorm_rows_ needs a contiguous tensor (in place)"
    rc = _lib.lib().tlc_renorm_rows_f32(C.c_int32(emb.shape[0]), C.c_int32(emb.shape[1]), _lib.ptr(emb), _lib.stream_ptr())
    _lib.check(rc, "tlc_renorm_rows_f32")
    return emb


@_lib.on_device_of
def lp_decode(pairs, emb, pi, w1, b1, w2, b2, out=None):
    """Fused Net.decode tail (baselines/TLCGNN.py:52-61).  pairs int32 [E,2], emb f32 [N,D], pi [E,P] float64 (the raw output of
    pd_pi_batch: cast to float32 on load) or float32 (cast once by the caller, as Net._tables does: the reference's
    torch.Tensor(PI) of :52-53 hoisted out of the per-decode path; same values, half the bytes)."""
    torch = _lib.require_gpu()
    assert pairs.dtype == torch.int32 and pi.dtype in (torch.float64, torch.float32)
    E = pairs.shape[0]
    if out is None:
        out = torch.empty(E, dtype=torch.float32, device=emb.device)
    fn = _lib.lib().tlc_lp_decode_fused if pi.dtype == torch.float64 else _lib.lib().tlc_lp_decode_fused_f32
    rc = fn(C.c_int64(E), _lib.ptr(pairs.contiguous()), _lib.ptr(_f32(emb)), C.c_int32(emb.shape[1]),
            _lib.ptr(pi.contiguous()), C.c_int32(pi.shape[1]), _lib.ptr(_f32(w1)), _lib.ptr(_f32(b1)),
            _lib.ptr(_f32(w2).reshape(-1)), _lib.ptr(_f32(b2)), _lib.ptr(out), _lib.stream_ptr())
    _lib.check(rc, "tlc_lp_decode_fused")
    return out


# ---- backward of the LP training step (lp_backward.hip; autograd.GcnLayer / autograd.LpDecode) ---------------------------------
@_lib.on_device_of
def gcn_norm_csr_t(edge_index, num_nodes, rowptr):
    """A^T of gcn_norm_csr's operator (rowptr: its row pointers) as CSR by source: (rowptr_t, col_t, val_t) -- what
    d(XW) = A^T G of the GCN backward runs on with spmm.  Holds for a non-symmetric edge_index too."""
    torch = _lib.require_gpu()
    assert edge_index.is_cuda and edge_index.dtype == torch.int64 and edge_index.shape[0] == 2
    ei = edge_index.contiguous()
    E, dev = ei.shape[1], ei.device
    rowptr_t = torch.empty(num_nodes + 1, dtype=torch.int32, device=dev)
    col_t = torch.empty(E + num_nodes, dtype=torch.int32, device=dev)
    val_t = torch.empty(E + num_nodes, dtype=torch.float32, device=dev)
    nnz = torch.zeros(1, dtype=torch.int32, device=dev)
    rc = _lib.lib().tlc_gcn_norm_csr_t(C.c_int32(num_nodes), C.c_int64(E), _lib.ptr(ei), _lib.ptr(rowptr.contiguous()), _lib.ptr(rowptr_t),
                                       _lib.ptr(col_t), _lib.ptr(val_t), _lib.ptr(nnz), _lib.stream_ptr())
    _lib.check(rc, "tlc_gcn_norm_csr_t")
    k = int(nnz.item())
    return rowptr_t, col_t[:k].contiguous(), val_t[:k].contiguous()


@_lib.on_device_of
def gemm_tn(a, b, out=None):
    """C = A^T @ B for A [K,M], B [K,N] float32 CUDA (tlc_gemm_tn_f32: split-K on the f32 MFMA, partials added in a fixed order).
    a None: the column sums of b as [1,N]."""
    torch = _lib.require_gpu()
    b = _f32(b)
    K, N = b.shape
    if a is not None:
        a = _f32(a)
        assert a.shape[0] == K
        M = a.shape[1]
    else:
        M = 1
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=b.device)
    work = _scratch("tlc_gemm_tn_work_floats", (M, N), torch.float32, b.device)
    rc = _lib.lib().tlc_gemm_tn_f32(C.c_int32(M), C.c_int32(N), C.c_int64(K), _lib.ptr(a), _lib.ptr(b), _lib.ptr(out), _lib.ptr(work),
                                    _lib.stream_ptr())
    _lib.check(rc, "tlc_gemm_tn_f32")
    return out


def colsum(b):
    """Column sums of b [K,N] -> [N] (the bias gradient of a layer), tlc_gemm_tn_f32 with a column of ones."""
    return gemm_tn(None, b).reshape(-1)


def endpoint_groups(pairs, num_nodes):
    """The endpoints of `pairs` [E,2] grouped by node, in slot order (slot 2 i / 2 i + 1 = pair i's first / second endpoint):
    (node_ptr int32[N+1], slots int32[2E]).  A sort on unique keys (node * 2E + slot): the order is fixed by the pairs alone."""
    import torch
    flat = pairs.reshape(-1).to(torch.int64)
    n2 = flat.numel()
    keys = flat * max(n2, 1) + torch.arange(n2, device=flat.device)
    sk, _ = torch.sort(keys)
    nodes = torch.div(sk, max(n2, 1), rounding_mode="floor")
    slots = (sk - nodes * max(n2, 1)).to(torch.int32)
    node_ptr = torch.searchsorted(nodes, torch.arange(num_nodes + 1, device=flat.device)).to(torch.int32)
    return node_ptr, slots.contiguous()


@_lib.on_device_of
def lp_decode_bwd(pairs, emb_pre, emb, pi, w1, b1, w2, b2, gprob, groups=None):
    """Backward of renorm_rows_ + lp_decode (tlc_lp_decode_bwd_f32).  pairs int32 [E,2]; emb_pre f32 [N,16] (before the renorm), emb
    (after it); pi f32 [E,25]; gprob f32 [E] -> (d emb_pre [N,16], dW1 [25,41], db1 [25], dW2 [1,25], db2 [1])."""
    torch = _lib.require_gpu()
    assert pairs.dtype == torch.int32 and pi.dtype == torch.float32
    E, n = pairs.shape[0], emb_pre.shape[0]
    dev = emb_pre.device
    node_ptr, slots = endpoint_groups(pairs, n) if groups is None else groups
    gemb = torch.empty((n, emb_pre.shape[1]), dtype=torch.float32, device=dev)
    gw = torch.empty(1076, dtype=torch.float32, device=dev)
    work = _scratch("tlc_lp_decode_bwd_work_floats", (E,), torch.float32, dev)
    pairs_c = pairs.contiguous()
    rc = _lib.lib().tlc_lp_decode_bwd_f32(C.c_int64(E), _lib.ptr(pairs_c), _lib.ptr(_f32(emb_pre)), _lib.ptr(_f32(emb)), C.c_int32(n),
                                          C.c_int32(emb_pre.shape[1]), _lib.ptr(pi.contiguous()), C.c_int32(pi.shape[1]),
                                          _lib.ptr(_f32(w1)), _lib.ptr(_f32(b1)), _lib.ptr(_f32(w2).reshape(-1)), _lib.ptr(_f32(b2)),
                                          _lib.ptr(_f32(gprob)), _lib.ptr(node_ptr), _lib.ptr(slots), _lib.ptr(gemb), _lib.ptr(gw),
                                          _lib.ptr(work), _lib.stream_ptr())
    _lib.check(rc, "tlc_lp_decode_bwd_f32")
    return gemb, gw[:1025].view(25, 41), gw[1025:1050], gw[1050:1075].view(1, 25), gw[1075:1076]


# ---- node classification: curvGN (nc_curv.hip; autograd.CurvConv / autograd.NcLinear, Knowledge_Distillation/ConvCurv_GIN.py) --
@_lib.on_device_of
def nc_group(edge_index, num_nodes):
    """The edges of edge_index int64 CUDA [2,E] grouped by source and by target (tlc_nc_group), built once per graph:
    int32 [2 (n + 1) + 4 E] = src_ptr | tgt_ptr | src_eid | tgt_eid | src | dst.  Reads one int back (the count of ids outside
    [0, num_nodes)) and raises ValueError if there are any."""
    torch = _lib.require_gpu()
    assert edge_index.is_cuda and edge_index.dtype == torch.int64 and edge_index.dim() == 2 and edge_index.shape[0] == 2
    ei = edge_index.contiguous()
    E, n, dev = int(ei.shape[1]), int(num_nodes), ei.device
    L = _lib.lib()
    groups = torch.empty(2 * (n + 1) + 4 * E, dtype=torch.int32, device=dev)
    work = torch.empty(max(1, int(L.tlc_nc_group_work_ints(C.c_int32(n), C.c_int64(E)))), dtype=torch.int32, device=dev)
    bad = torch.empty(1, dtype=torch.int32, device=dev)
    rc = L.tlc_nc_group(C.c_int32(n), C.c_int64(E), _lib.ptr(ei) if E else None, _lib.ptr(groups), _lib.ptr(work), _lib.ptr(bad),
                        _lib.stream_ptr())
    _lib.check(rc, "tlc_nc_group")
    nbad = int(bad.item())
    if nbad:
        raise ValueError("nc_group: %d edge(s) with a node id outside [0, %d)" % (nbad, n))
    return groups


@_lib.on_device_of
def nc_linear(x, w, b=None):
    """x [M,K] @ w[N,K]^T + b on the f32 MFMA (tlc_nc_linear_f32): torch.nn.Linear's forward for any N and K."""
    torch = _lib.require_gpu()
    x, w = _f32(x), _f32(w)
    M, K = x.shape
    N = w.shape[0]
    assert w.shape[1] == K
    y = torch.empty((M, N), dtype=torch.float32, device=x.device)
    rc = _lib.lib().tlc_nc_linear_f32(C.c_int32(M), C.c_int32(N), C.c_int32(K), _lib.ptr(x), _lib.ptr(w),
                                      _lib.ptr(_f32(b)) if b is not None else None, _lib.ptr(y), _lib.stream_ptr())
    _lib.check(rc, "tlc_nc_linear_f32")
    return y


@_lib.on_device_of
def nc_linear_bwd(x, w, gy, need_gx=True):
    """Backward of nc_linear (tlc_nc_linear_bwd_f32) -> (gx [M,K] or None, gw [N,K], gb [N])."""
    torch = _lib.require_gpu()
    x, w, gy = _f32(x), _f32(w), _f32(gy)
    M, K = x.shape
    N = w.shape[0]
    dev = x.device
    gx = torch.empty((M, K), dtype=torch.float32, device=dev) if need_gx else None
    gw = torch.empty((N, K), dtype=torch.float32, device=dev)
    gb = torch.empty(N, dtype=torch.float32, device=dev)
    work = _scratch("tlc_nc_linear_bwd_work_floats", (N, K), torch.float32, dev)
    rc = _lib.lib().tlc_nc_linear_bwd_f32(C.c_int32(M), C.c_int32(N), C.c_int32(K), _lib.ptr(x), _lib.ptr(w), _lib.ptr(gy), _lib.ptr(gx),
                                          _lib.ptr(gw), _lib.ptr(gb), _lib.ptr(work), _lib.stream_ptr())
    _lib.check(rc, "tlc_nc_linear_bwd_f32")
    return gx, gw, gb


def _nc_ptr(t):
    return _lib.ptr(t) if t.numel() else None


@_lib.on_device_of
def nc_curv_fwd(groups, xl, w_mul, w1, prelu, w2, b2):
    """curvGN after the projection (tlc_nc_curv_fwd_f32): groups from nc_group, xl f32 [n,C], w_mul f32 [E,D], the edge MLP's
    w1 [C,D], prelu [C], w2 [C,C], b2 [C] -> (out [n,C], alpha [E,C])."""
    torch = _lib.require_gpu()
    xl, w_mul = _f32(xl), _f32(w_mul)
    n, Cc = xl.shape
    E, D = w_mul.shape
    assert groups.numel() == 2 * (n + 1) + 4 * E, "groups were built for another graph"
    out = torch.empty((n, Cc), dtype=torch.float32, device=xl.device)
    alpha = torch.empty((E, Cc), dtype=torch.float32, device=xl.device)
    rc = _lib.lib().tlc_nc_curv_fwd_f32(C.c_int32(n), C.c_int64(E), C.c_int32(Cc), C.c_int32(D), _lib.ptr(groups), _lib.ptr(xl),
                                        _nc_ptr(w_mul), _lib.ptr(_f32(w1)), _lib.ptr(_f32(prelu)), _lib.ptr(_f32(w2)), _lib.ptr(_f32(b2)),
                                        _nc_ptr(alpha), _lib.ptr(out), _lib.stream_ptr())
    _lib.check(rc, "tlc_nc_curv_fwd_f32")
    return out, alpha


@_lib.on_device_of
def nc_curv_bwd(groups, xl, w_mul, w1, prelu, w2, alpha, gout):
    """Backward of nc_curv_fwd (tlc_nc_curv_bwd_f32) -> (d xl [n,C], d w1 [C,D], d prelu [C], d w2 [C,C], d b2 [C])."""
    torch = _lib.require_gpu()
    xl, w_mul, gout = _f32(xl), _f32(w_mul), _f32(gout)
    n, Cc = xl.shape
    E, D = w_mul.shape
    dev = xl.device
    L = _lib.lib()
    nbytes = int(L.tlc_nc_curv_work_bytes(C.c_int32(n), C.c_int64(E), C.c_int32(Cc), C.c_int32(D)))
    if nbytes < 0:
        raise ValueError("nc_curv_bwd: C = %d (1..256) / D = %d (1..64) outside the built range" % (Cc, D))
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    gxl = torch.empty((n, Cc), dtype=torch.float32, device=dev)
    gw1 = torch.empty((Cc, D), dtype=torch.float32, device=dev)
    gp = torch.empty(Cc, dtype=torch.float32, device=dev)
    gw2 = torch.empty((Cc, Cc), dtype=torch.float32, device=dev)
    gb2 = torch.empty(Cc, dtype=torch.float32, device=dev)
    rc = L.tlc_nc_curv_bwd_f32(C.c_int32(n), C.c_int64(E), C.c_int32(Cc), C.c_int32(D), _lib.ptr(groups), _lib.ptr(xl), _nc_ptr(w_mul),
                               _lib.ptr(_f32(w1)), _lib.ptr(_f32(prelu)), _lib.ptr(_f32(w2)), _nc_ptr(_f32(alpha)), _lib.ptr(gout),
                               _lib.ptr(gxl), _lib.ptr(gw1), _lib.ptr(gp), _lib.ptr(gw2), _lib.ptr(gb2), _lib.ptr(work), C.c_int64(nbytes),
                               _lib.stream_ptr())
    _lib.check(rc, "tlc_nc_curv_bwd_f32")
    return gxl, gw1, gp, gw2, gb2


# ---- link-prediction scoring (lp_metrics.hip; metrics.py, pipelines.test(metrics="device")) -----------------------------------
RANK_LDS_CAP = 16384             # include/tlcgnn.h TLC_RANK_LDS_CAP: longer segments take the radix tier
RANK_FORCE_RADIX = 0x1
RANK_NONFINITE, RANK_BAD_LABEL, RANK_EMPTY = 0x1, 0x2, 0x4


def _rank_dtypes(scores, labels):
    import torch
    sdt = {torch.float32: 0, torch.float64: 1}.get(scores.dtype)
    if sdt is None:
        raise TypeError("binary_rank_metrics: scores must be float32 or float64, not %s" % scores.dtype)
    if labels.dtype == torch.bool:
        labels = labels.view(torch.uint8)
    ldt = {torch.uint8: 0, torch.int64: 1, torch.float32: 2}.get(labels.dtype)
    if ldt is None:
        raise TypeError("binary_rank_metrics: labels must be bool, uint8, int64 or float32, not %s" % labels.dtype)
    return sdt, labels, ldt


@_lib.on_device_of
def binary_rank_metrics(scores, labels, seg_ptr=None, force_radix=False):
    """ROC-AUC and average precision per segment (tlc_binary_rank_metrics, sklearn's binary semantics with pos_label 1).

    scores: 1-D float32 / float64 CUDA; labels: 1-D bool / uint8 / int64 / float32 CUDA of the same length, 0 or 1.
    seg_ptr: host offsets [S+1] (a list, numpy array or CPU tensor; None: one segment of everything).  Enqueued on the current
    stream, workspace from torch's allocator, no host synchronisation: returns device tensors (auc f64 [S], ap f64 [S],
    n_pos int64 [S], n_neg int64 [S], status int32 [S]) -- status bits RANK_NONFINITE / RANK_BAD_LABEL / RANK_EMPTY, 0 = valid.
    force_radix: every non-empty segment through the multi-workgroup radix tier (tests compare the two tiers)."""
    import numpy as np
    torch = _lib.require_gpu()
    assert scores.is_cuda and labels.is_cuda and scores.device == labels.device, "scores and labels must be on one CUDA device"
    scores, labels = scores.reshape(-1).contiguous(), labels.reshape(-1).contiguous()
    if scores.numel() != labels.numel():
        raise ValueError("binary_rank_metrics: %d scores but %d labels" % (scores.numel(), labels.numel()))
    sdt, labels, ldt = _rank_dtypes(scores, labels)
    if seg_ptr is None:
        seg_ptr = [0, scores.numel()]
    if isinstance(seg_ptr, torch.Tensor):
        if seg_ptr.is_cuda:
            raise TypeError("binary_rank_metrics: seg_ptr is read on the host; pass it as a list or CPU tensor")
        seg_ptr = seg_ptr.numpy()
    sp = np.ascontiguousarray(np.asarray(seg_ptr, dtype=np.int64))
    if sp.ndim != 1 or sp.size < 2:
        raise ValueError("binary_rank_metrics: seg_ptr needs S + 1 >= 2 offsets")
    if sp[-1] > scores.numel():
        raise ValueError("binary_rank_metrics: seg_ptr ends at %d, past the %d scores" % (sp[-1], scores.numel()))
    S = sp.size - 1
    flags = RANK_FORCE_RADIX if force_radix else 0
    L = _lib.lib()
    hp = sp.ctypes.data_as(C.c_void_p)
    nbytes = int(L.tlc_binary_rank_metrics_work_bytes(hp, C.c_int32(S), C.c_int(sdt), C.c_uint32(flags)))
    if nbytes < 0:
        raise ValueError("binary_rank_metrics: malformed seg_ptr (must start at >= 0 and be non-decreasing)")
    dev = scores.device
    work = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    f64 = torch.empty(2 * S, dtype=torch.float64, device=dev)
    i64 = torch.empty(2 * S, dtype=torch.int64, device=dev)
    status = torch.empty(S, dtype=torch.int32, device=dev)
    rc = L.tlc_binary_rank_metrics(_lib.ptr(scores), C.c_int(sdt), _lib.ptr(labels), C.c_int(ldt), hp, C.c_int32(S), C.c_uint32(flags),
                                   _lib.ptr(f64), _lib.ptr(f64[S:]), _lib.ptr(i64), _lib.ptr(i64[S:]), _lib.ptr(status), _lib.ptr(work),
                                   C.c_int64(nbytes), _lib.stream_ptr())
    _lib.check(rc, "tlc_binary_rank_metrics")
    return f64[:S], f64[S:], i64[:S], i64[S:], status


@_lib.on_device_of
def gat_layer(rowptr, src, x, wl, att, wij, bias, prelu_slope=-1.0, out=None):
    """One PDGNN layer (Knowledge_Distillation/gat_conv.py:113-216) on a CSR-by-target batch."""
    torch = _lib.require_gpu()
    x = _f32(x)
    n, c_in = x.shape
    c_out = wl.shape[0]
    if out is None:
        out = torch.empty((n, 2 * c_out), dtype=torch.float32, device=x.device)
    work = _scratch("tlc_gat_layer_fwd_work_floats", (max(n, 1), c_in, c_out), torch.float32, x.device)
    rc = _lib.lib().tlc_gat_layer_fwd(C.c_int32(n), _lib.ptr(rowptr), _lib.ptr(src), _lib.ptr(x), C.c_int32(c_in),
                                      C.c_int32(c_out), _lib.ptr(_f32(wl)), _lib.ptr(_f32(att).reshape(-1)), _lib.ptr(_f32(wij)),
                                      _lib.ptr(_f32(bias)), C.c_float(prelu_slope), _lib.ptr(work), _lib.ptr(out),
                                      _lib.stream_ptr())
    _lib.check(rc, "tlc_gat_layer_fwd")
    return out


GAT_TILE_NODES = 192          # GT_TM of csrc/gat_forward.hip


def gat_tiles(rowptr, col, n, tile_nodes=GAT_TILE_NODES):
    """Cuts a block-diagonal batch (CSR by target: rowptr int32 [n+1], col = the sources) into self-contained tiles for
    tlc_gat_layer_tiled_fwd: int32 [T+1] node offsets of tiles of at most `tile_nodes` consecutive nodes, cut only at positions no
    edge crosses -- or None when the batch has no such cuts close enough together (one big graph: the two-kernel layer serves it).
    All on the device (tlc_gat_tile_cut; one host read, of the tile count)."""
    if not 2 <= int(tile_nodes) <= GAT_TILE_NODES:
        raise ValueError("gat_tiles: tile_nodes %r; gat_tile_kernel's LDS tile holds at most %d rows" % (tile_nodes, GAT_TILE_NODES))
    torch = _lib.require_gpu()
    n = int(n)
    if n == 0:
        return None
    dev = rowptr.device
    work = _scratch("tlc_gat_tile_cut_work_ints", (n,), torch.int32, dev)
    tiles = _scratch("tlc_gat_tile_cut_max_tiles", (n, tile_nodes), torch.int32, dev)
    nt = C.c_int32(0)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().tlc_gat_tile_cut(C.c_int32(n), _lib.ptr(rowptr), _lib.ptr(col), C.c_int32(tile_nodes), _lib.ptr(work),
                                               _lib.ptr(tiles), C.byref(nt), _lib.stream_ptr(dev)), "tlc_gat_tile_cut")
    return tiles[:nt.value + 1] if nt.value > 0 else None


@_lib.on_device_of
def gat_layer_tiled(rowptr, src, tiles, x, wl, att, wij, bias, prelu_slope=-1.0, out=None):
    """One PDGNN layer (gat_conv.py:113-216) on a block-diagonal batch cut by gat_tiles: the node rows stay in LDS
    (tlc_gat_layer_tiled_fwd).  Shapes it does not take raise _lib.TlcError(TLC_ERR_UNSUPPORTED): callers check `gat_tiled_ok`."""
    torch = _lib.require_gpu()
    x = _f32(x)
    n, c_in = x.shape
    c_out = wl.shape[0]
    if out is None:
        out = torch.empty((n, 2 * c_out), dtype=torch.float32, device=x.device)
    work = _scratch("tlc_gat_layer_tiled_fwd_work_floats", (c_in, c_out), torch.float32, x.device)
    rc = _lib.lib().tlc_gat_layer_tiled_fwd(C.c_int32(n), _lib.ptr(rowptr), _lib.ptr(src), C.c_int32(tiles.numel() - 1), _lib.ptr(tiles),
                                            _lib.ptr(x), C.c_int32(c_in), C.c_int32(c_out), _lib.ptr(_f32(wl)),
                                            _lib.ptr(_f32(att).reshape(-1)), _lib.ptr(_f32(wij)), _lib.ptr(_f32(bias)),
                                            C.c_float(prelu_slope), _lib.ptr(work), _lib.ptr(out), _lib.stream_ptr())
    _lib.check(rc, "tlc_gat_layer_tiled_fwd")
    return out


def gat_tiled_ok(c_in, c_out):
    return c_in in (1, 64) and c_out in (16, 32)


@_lib.on_device_of
def edge_head(src, dst, x, w5, b5, prelu_slope, w6, b6, out=None):
    """Edge head of Teacher_Model.forward (Knowledge_Distillation/Teacher_model.py:54-59) -> f32 [E,2]."""
    torch = _lib.require_gpu()
    x = _f32(x)
    E = src.numel()
    if out is None:
        out = torch.empty((E, 2), dtype=torch.float32, device=x.device)
    n, c, hidden = x.shape[0], x.shape[1], w5.shape[0]
    work = _scratch("tlc_edge_head_fwd_work_floats", (n, c, hidden), torch.float32, x.device)
    rc = _lib.lib().tlc_edge_head_fwd(C.c_int64(E), _lib.ptr(src), _lib.ptr(dst), _lib.ptr(x), C.c_int32(c),
                                      _lib.ptr(_f32(w5)), _lib.ptr(_f32(b5)), C.c_int32(hidden), C.c_float(prelu_slope),
                                      _lib.ptr(_f32(w6)), _lib.ptr(_f32(b6)), _lib.ptr(out), C.c_int32(n), _lib.ptr(work),
                                      _lib.stream_ptr())
    _lib.check(rc, "tlc_edge_head_fwd")
    return out


@_lib.on_device_of
def gat_layer_bwd(rowptr, src, x, wl, att, wij, prelu_slope, out, gout, need_gx=True):
    """Gradients of `gat_layer` (what autograd runs through Knowledge_Distillation/gat_conv.py:113-216):
    -> (gX or None, gWl, gatt, gWij, gbias).  `out` is the forward's output (read for the fused PReLU only)."""
    torch = _lib.require_gpu()
    x = _f32(x)
    n, c_in = x.shape
    c_out = wl.shape[0]
    dev = x.device
    gx = torch.empty((n, c_in), dtype=torch.float32, device=dev) if need_gx else None
    gwl = torch.empty((c_out, c_in), dtype=torch.float32, device=dev)
    gatt = torch.empty(c_out, dtype=torch.float32, device=dev)
    gwij = torch.empty((c_out, 2 * c_out), dtype=torch.float32, device=dev)
    gbias = torch.empty(2 * c_out, dtype=torch.float32, device=dev)
    work = _scratch("tlc_gat_layer_bwd_work_floats", (max(n, 1), c_in, c_out), torch.float32, dev)
    rc = _lib.lib().tlc_gat_layer_bwd(C.c_int32(n), _lib.ptr(rowptr), _lib.ptr(src), _lib.ptr(x), C.c_int32(c_in), C.c_int32(c_out),
                                      _lib.ptr(_f32(wl)), _lib.ptr(_f32(att).reshape(-1)), _lib.ptr(_f32(wij)), C.c_float(prelu_slope),
                                      _lib.ptr(_f32(out)) if out is not None else None, _lib.ptr(_f32(gout)), _lib.ptr(gx),
                                      _lib.ptr(gwl), _lib.ptr(gatt), _lib.ptr(gwij), _lib.ptr(gbias), _lib.ptr(work), _lib.stream_ptr())
    _lib.check(rc, "tlc_gat_layer_bwd")
    return gx, gwl, gatt, gwij, gbias


@_lib.on_device_of
def edge_head_bwd(src, dst, x, w5, b5, prelu_slope, w6, gpd):
    """Gradients of `edge_head` (Teacher_model.py:54-59): -> (gX, gW5, gb5, gW6, gb6)."""
    torch = _lib.require_gpu()
    x = _f32(x)
    E = src.numel()
    n, c, hidden = x.shape[0], x.shape[1], w5.shape[0]
    dev = x.device
    gx = torch.zeros((n, c), dtype=torch.float32, device=dev)
    gw5 = torch.empty((hidden, 2 * c), dtype=torch.float32, device=dev)
    gb5 = torch.empty(hidden, dtype=torch.float32, device=dev)
    gw6 = torch.empty((2, hidden), dtype=torch.float32, device=dev)
    gb6 = torch.empty(2, dtype=torch.float32, device=dev)
    work = _scratch("tlc_edge_head_bwd_work_floats", (max(E, 1), c, hidden), torch.float32, dev)
    rc = _lib.lib().tlc_edge_head_bwd(C.c_int64(E), _lib.ptr(src), _lib.ptr(dst), _lib.ptr(x), C.c_int32(c), _lib.ptr(_f32(w5)),
                                      _lib.ptr(_f32(b5)), C.c_int32(hidden), C.c_float(prelu_slope), _lib.ptr(_f32(w6)),
                                      _lib.ptr(_f32(gpd)), _lib.ptr(gx), _lib.ptr(gw5), _lib.ptr(gb5), _lib.ptr(gw6), _lib.ptr(gb6),
                                      _lib.ptr(work), _lib.stream_ptr())
    _lib.check(rc, "tlc_edge_head_bwd")
    return gx, gw5, gb5, gw6, gb6


# ---- the sum-aggregating baselines of the PDGNN teacher (gnn_layers.hip; autograd.GnnLayer; Knowledge_Distillation/gnn_layers.py) ----
GNN_ACTS = {None: _lib.GNN_ACT_NONE, "none": _lib.GNN_ACT_NONE, "relu": _lib.GNN_ACT_RELU, "prelu": _lib.GNN_ACT_PRELU}


def _opt_f32(t):
    return None if t is None else _f32(t)


@_lib.on_device_of
def gnn_layer(rowptr, src, coef, self_scale, x, wa, ws=None, bias=None, act=None, slope=0.0, want_agg=False, out=None):
    """One layer of the teacher's GIN / GCN / SAGE baselines (tlc_gnn_layer_fwd) on a CSR by target:
    y = act(Wa (sum_e coef[e] x_src[e] + self_scale x_i) + Ws x_i + b).  coef None: all 1; act None / 'relu' / 'prelu' (slope).
    -> out f32 [n, c_out], or (out, agg f32 [n, c_in]) with want_agg (the aggregate the backward reads)."""
    torch = _lib.require_gpu()
    x = _f32(x)
    n, c_in = x.shape
    c_out = wa.shape[0]
    if out is None:
        out = torch.empty((n, c_out), dtype=torch.float32, device=x.device)
    agg = torch.empty((n, c_in), dtype=torch.float32, device=x.device) if want_agg else None
    keep = (_f32(wa), _opt_f32(ws), _opt_f32(bias), _opt_f32(coef))
    rc = _lib.lib().tlc_gnn_layer_fwd(C.c_int32(n), _lib.ptr(rowptr), _lib.ptr(src), _lib.ptr(keep[3]), C.c_float(self_scale), _lib.ptr(x),
                                      C.c_int32(c_in), C.c_int32(c_out), _lib.ptr(keep[0]), _lib.ptr(keep[1]), _lib.ptr(keep[2]),
                                      C.c_int32(GNN_ACTS[act]), C.c_float(slope), _lib.ptr(out), _lib.ptr(agg), _lib.stream_ptr())
    _lib.check(rc, "tlc_gnn_layer_fwd")
    return (out, agg) if want_agg else out


@_lib.on_device_of
def gnn_layer_bwd(rowptr_t, col_t, coef_t, self_scale, x, agg, out, gout, wa, ws=None, has_bias=True, act=None, slope=0.0, need_gx=True):
    """Gradients of `gnn_layer` (tlc_gnn_layer_bwd; no atomics): -> (gX or None, gWa, gWs or None, gb or None).  rowptr_t / col_t /
    coef_t: the structure's transpose as a CSR by source (GnnBatch holds it); x, agg, out: the forward's input, aggregate and output."""
    torch = _lib.require_gpu()
    x, gout = _f32(x), _f32(gout)
    n, c_in = x.shape
    c_out = wa.shape[0]
    dev = x.device
    gx = torch.empty((n, c_in), dtype=torch.float32, device=dev) if need_gx else None
    gwa = torch.empty((c_out, c_in), dtype=torch.float32, device=dev)
    gws = torch.empty((c_out, c_in), dtype=torch.float32, device=dev) if ws is not None else None
    gb = torch.empty(c_out, dtype=torch.float32, device=dev) if has_bias else None
    L = _lib.lib()
    nbytes = int(L.tlc_gnn_layer_bwd_work_bytes(C.c_int32(n), C.c_int32(c_in), C.c_int32(c_out)))
    if nbytes < 0:
        raise ValueError("gnn_layer_bwd: negative size")
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    keep = (_f32(wa), _opt_f32(ws), _opt_f32(coef_t), _f32(agg), _f32(out))
    rc = L.tlc_gnn_layer_bwd(C.c_int32(n), _lib.ptr(rowptr_t), _lib.ptr(col_t), _lib.ptr(keep[2]), C.c_float(self_scale), _lib.ptr(x),
                             _lib.ptr(keep[3]), _lib.ptr(keep[4]), _lib.ptr(gout), C.c_int32(c_in), C.c_int32(c_out), _lib.ptr(keep[0]),
                             _lib.ptr(keep[1]), C.c_int32(GNN_ACTS[act]), C.c_float(slope), _lib.ptr(gx), _lib.ptr(gwa), _lib.ptr(gws),
                             _lib.ptr(gb), _lib.ptr(work), C.c_int64(nbytes), _lib.stream_ptr())
    _lib.check(rc, "tlc_gnn_layer_bwd")
    return gx, gwa, gws, gb


def gnn_stack_ok(c_in, hidden, tiles):
    """Whether `gnn_stack` takes the batch: the reference's widths (in_dim 1, hidden 32) and a tile cut (ops.gat_tiles; None for a batch
    without close enough cuts, e.g. one big graph).  Everything else runs layer by layer (`gnn_layer`), with the same bits."""
    return int(c_in) == 1 and int(hidden) == 32 and tiles is not None and tiles.numel() >= 2


@_lib.on_device_of
def gnn_stack(rowptr, src, coef, self_scale, tiles, x, layers, out=None):
    """conv1 -> conv2 -> conv4 -> conv3 of Base_Model.forward (Teacher_model.py:213-241) without gradients in ONE launch
    (tlc_gnn_stack_fwd): x f32 [n, 1]; layers: four (wa, ws or None, bias or None, act, slope) in that order -> f32 [n, 32]."""
    torch = _lib.require_gpu()
    x = _f32(x).reshape(-1)
    n = x.shape[0]
    hidden = layers[0][0].shape[0]
    if out is None:
        out = torch.empty((n, hidden), dtype=torch.float32, device=x.device)
    keep, ptrs = [_opt_f32(coef)], []
    for wa, ws, b, _a, _s in layers:
        for t in (wa, ws, b):
            keep.append(_opt_f32(t))
            ptrs.append(None if t is None else keep[-1].data_ptr())
    arr = (C.c_void_p * 12)(*ptrs)
    acts = (C.c_int32 * 4)(*[GNN_ACTS[l[3]] for l in layers])
    slopes = (C.c_float * 4)(*[float(l[4]) for l in layers])
    rc = _lib.lib().tlc_gnn_stack_fwd(C.c_int32(n), _lib.ptr(rowptr), _lib.ptr(src), _lib.ptr(keep[0]), C.c_float(self_scale),
                                      C.c_int32(tiles.numel() - 1), _lib.ptr(tiles), _lib.ptr(x), C.c_int32(hidden), arr, acts, slopes,
                                      _lib.ptr(out), _lib.stream_ptr())
    _lib.check(rc, "tlc_gnn_stack_fwd")
    return out


# ---- the PDGNN layer family: GATConv's ablations and PDConv (msg_layers.hip; autograd.MsgLayer; gat_conv.py, PD_conv.py) ----
MSG_AGGS = {"sum_minmax": _lib.MSG_AGG_SUM_MINMAX, "sum_min": _lib.MSG_AGG_SUM_MIN}


def msg_mode(new_node_feat, use_edge_attn):
    return (_lib.MSG_NODE_FEAT if new_node_feat else 0) | (_lib.MSG_EDGE_ATTN if use_edge_attn else 0)


def csr_transpose_pos(rowptr, col, n):
    """The CSR by source of a `csr_by_target` structure (rowptr int32 [n + 1], col = the sources, of which the first rowptr[n] count):
    -> (rowptr_t int32 [n + 1], col_t int32 [nnz] = the targets, pos_t int32 [nnz] = each entry's position in `col`).  A stable sort, so a
    source's entries keep the order of their positions.  Torch ops on the tensors' device (CPU tensors work too); one host read, of nnz:
    built once per batch (GraphBatch.transpose)."""
    import torch
    n = int(n)
    nnz = int(rowptr[n]) if n > 0 else 0
    src = col[:nnz].to(torch.int64)
    counts = (rowptr[1:n + 1] - rowptr[:n]).to(torch.int64)
    tgt = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=rowptr.device), counts)
    order = torch.sort(src, stable=True).indices
    rowptr_t = torch.zeros(n + 1, dtype=torch.int32, device=rowptr.device)
    rowptr_t[1:] = torch.cumsum(torch.bincount(src, minlength=n), 0)
    return rowptr_t, tgt[order].to(torch.int32).contiguous(), order.to(torch.int32).contiguous()


def _msg_operands(x, wl, att, wij, mode):
    """(wl, att or None, wij or None) as the C ABI reads them, shapes checked against x [n, c_in] and c_out = wl.shape[0]: the library
    cannot see a tensor's size, so a wrong-shaped operand would be read out of bounds on the device."""
    c_out = wl.shape[0]
    if x.dim() != 2 or tuple(wl.shape) != (c_out, x.shape[1]):
        raise ValueError("msg_layer: x %s and wl %s do not fit [n, c_in] and [c_out, c_in]" % (tuple(x.shape), tuple(wl.shape)))
    att = _f32(att).reshape(-1) if mode & _lib.MSG_EDGE_ATTN else None
    wij = _f32(wij) if mode & _lib.MSG_NODE_FEAT else None
    if att is not None and att.numel() != c_out:
        raise ValueError("msg_layer: att has %d elements for c_out %d" % (att.numel(), c_out))
    if wij is not None and tuple(wij.shape) != (c_out, 2 * c_out):
        raise ValueError("msg_layer: wij %s is not [c_out, 2 c_out] = [%d, %d]" % (tuple(wij.shape), c_out, 2 * c_out))
    return _f32(wl), att, wij


def _msg_rows(name, t, n, c_out):
    if t is not None and tuple(t.shape) != (n, 2 * c_out):
        raise ValueError("msg_layer: %s %s is not [n, 2 c_out] = [%d, %d]" % (name, tuple(t.shape), n, 2 * c_out))


@_lib.on_device_of
def msg_layer(rowptr, src, x, wl, att, wij, bias, mode, agg="sum_minmax", prelu_slope=-1.0, out=None):
    """One layer of the PDGNN family (tlc_msg_layer_fwd) on a CSR by target with self loops (`csr_by_target`): mode = msg_mode(new_node_feat,
    use_edge_attn); agg 'sum_minmax' (gat_conv.py:216) or 'sum_min' (PD_conv.py:219).  att / wij are not read (and may be None) when their
    switch is off.  -> f32 [n, 2 c_out]."""
    torch = _lib.require_gpu()
    x = _f32(x)
    n, c_in = x.shape
    c_out = wl.shape[0]
    if bias.numel() != 2 * c_out or rowptr.numel() != n + 1:
        raise ValueError("msg_layer: bias of %d elements / rowptr of %d for c_out %d and %d nodes" % (bias.numel(), rowptr.numel(), c_out, n))
    if out is None:
        out = torch.empty((n, 2 * c_out), dtype=torch.float32, device=x.device)
    _msg_rows("out", out, n, c_out)
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous()
    L = _lib.lib()
    nbytes = int(L.tlc_msg_layer_fwd_work_bytes(C.c_int32(n), C.c_int32(c_in), C.c_int32(c_out), C.c_int32(mode)))
    if nbytes < 0:
        raise ValueError("msg_layer: negative size or unknown mode bits")
    work = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=x.device)
    keep = _msg_operands(x, wl, att, wij, mode) + (_f32(bias).reshape(-1),)
    rc = L.tlc_msg_layer_fwd(C.c_int32(n), _lib.ptr(rowptr), _lib.ptr(src), _lib.ptr(x), C.c_int32(c_in), C.c_int32(c_out), _lib.ptr(keep[0]),
                             _lib.ptr(keep[1]), _lib.ptr(keep[2]), _lib.ptr(keep[3]), C.c_int32(mode), C.c_int32(MSG_AGGS[agg]),
                             C.c_float(prelu_slope), _lib.ptr(work), C.c_int64(nbytes), _lib.ptr(out), _lib.stream_ptr())
    _lib.check(rc, "tlc_msg_layer_fwd")
    return out


@_lib.on_device_of
def msg_layer_bwd(rowptr, src, rowptr_t, col_t, pos_t, x, wl, att, wij, mode, agg, prelu_slope, out, gout, need_gx=True):
    """Gradients of `msg_layer` (tlc_msg_layer_bwd; no floating-point atomics): -> (gX or None, gWl, gatt or None, gWij or None, gbias).
    rowptr_t / col_t / pos_t: `csr_transpose_pos` of the structure; `out`: the forward's output (read for the fused PReLU only)."""
    torch = _lib.require_gpu()
    x, gout = _f32(x), _f32(gout)
    n, c_in = x.shape
    c_out = wl.shape[0]
    dev = x.device
    _msg_rows("gout", gout, n, c_out)
    _msg_rows("out", out, n, c_out)
    if rowptr.numel() != n + 1 or rowptr_t.numel() != n + 1 or col_t.numel() != pos_t.numel() or src.numel() < col_t.numel():
        raise ValueError("msg_layer_bwd: the CSR by target and its transpose (csr_transpose_pos) do not fit %d nodes" % n)
    gx = torch.empty((n, c_in), dtype=torch.float32, device=dev) if need_gx else None
    gwl = torch.empty((c_out, c_in), dtype=torch.float32, device=dev)
    gatt = torch.empty(c_out, dtype=torch.float32, device=dev) if mode & _lib.MSG_EDGE_ATTN else None
    gwij = torch.empty((c_out, 2 * c_out), dtype=torch.float32, device=dev) if mode & _lib.MSG_NODE_FEAT else None
    gbias = torch.empty(2 * c_out, dtype=torch.float32, device=dev)
    L = _lib.lib()
    nbytes = int(L.tlc_msg_layer_bwd_work_bytes(C.c_int32(n), C.c_int64(col_t.numel()), C.c_int32(c_in), C.c_int32(c_out), C.c_int32(mode)))
    if nbytes < 0:
        raise ValueError("msg_layer_bwd: negative size or unknown mode bits")
    work = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    keep = _msg_operands(x, wl, att, wij, mode) + (_opt_f32(out),)
    rc = L.tlc_msg_layer_bwd(C.c_int32(n), _lib.ptr(rowptr), _lib.ptr(src), _lib.ptr(rowptr_t), _lib.ptr(col_t), _lib.ptr(pos_t), _lib.ptr(x),
                             C.c_int32(c_in), C.c_int32(c_out), _lib.ptr(keep[0]), _lib.ptr(keep[1]), _lib.ptr(keep[2]), C.c_int32(mode),
                             C.c_int32(MSG_AGGS[agg]), C.c_float(prelu_slope), _lib.ptr(keep[3]), _lib.ptr(gout), _lib.ptr(gx), _lib.ptr(gwl),
                             _lib.ptr(gatt), _lib.ptr(gwij), _lib.ptr(gbias), _lib.ptr(work), C.c_int64(nbytes), _lib.stream_ptr())
    _lib.check(rc, "tlc_msg_layer_bwd")
    return gx, gwl, gatt, gwij, gbias


REDUCE = {"add": 0, "sum": 0, "mean": 1, "min": 2, "max": 3}


@_lib.on_device_of
def scatter(src, index, dim_size, reduce="sum"):
    """torch_scatter.scatter(src, index, dim=0, dim_size=dim_size, reduce=...) (message_passing.py:292).

    src float32 CUDA [E, ...] (trailing dims flattened), index int64 CUDA [E] -> [dim_size, ...]; empty segments are 0."""
    torch = _lib.require_gpu()
    src = _f32(src)
    E = src.shape[0]
    tail = tuple(src.shape[1:])
    k = 1
    for d in tail:
        k *= int(d)
    k = max(k, 1)
    out = torch.empty((dim_size,) + tail, dtype=torch.float32, device=src.device)
    r = REDUCE[reduce]
    cnt = torch.empty(max(dim_size, 1), dtype=torch.int32, device=src.device) if r != 0 else None
    rc = _lib.lib().tlc_scatter_f32(C.c_int64(E), _lib.ptr(index.contiguous()), _lib.ptr(src), C.c_int32(k), C.c_int(r),
                                    C.c_int32(dim_size), _lib.ptr(out), _lib.ptr(cnt), _lib.stream_ptr())
    _lib.check(rc, "tlc_scatter_f32")
    return out


@_lib.on_device_of
def w2_partial_matching(xoff, X, yoff, Y, order=2, want_grad=True, max_points=None, large="refuse"):
    """PDGNN's diagram loss for a batch of (predicted, target) diagram pairs (Knowledge_Distillation/wasserstein.py:198-379 with
    num_models = 1): xoff / yoff int64[B+1] offsets, X / Y float64[., 2] CUDA tensors.
    -> dict(loss[B], wxy[B], wxd[B], assign[sum n] (target index or -1 = diagonal), grad[sum n, 2] (d loss / d X), status[B]).
    large: 'refuse': a problem of more than 4 096 predicted points gets status 2; 'device': a second call (`w2_large_matching` with
    min_rows = 4096) solves those of up to 65 536 into the same tensors."""
    check_w2_large(large)
    torch = _lib.require_gpu()
    B = xoff.numel() - 1
    dev = X.device
    X = X.to(torch.float64).contiguous()
    Y = Y.to(torch.float64).contiguous()
    nx = int(X.shape[0])
    if B > 0:
        # (offsets beyond the arrays would be read out of bounds on the device; one host read, with max_points below)
        ends = torch.stack([xoff[-1], yoff[-1], (xoff[1:] - xoff[:-1]).max()]).tolist()
        if ends[0] > nx or ends[1] > int(Y.shape[0]):
            raise ValueError("w2_partial_matching: offsets end at (%d, %d) but X / Y hold (%d, %d) points"
                             % (ends[0], ends[1], nx, int(Y.shape[0])))
        if max_points is None:
            max_points = int(ends[2])
    elif max_points is None:
        max_points = 0
    loss = torch.zeros(max(B, 1), dtype=torch.float64, device=dev)
    wxy = torch.zeros_like(loss)
    wxd = torch.zeros_like(loss)
    assign = torch.full((max(nx, 1),), -1, dtype=torch.int32, device=dev)
    grad = torch.zeros((max(nx, 1), 2), dtype=torch.float64, device=dev) if want_grad else None
    status = torch.zeros(max(B, 1), dtype=torch.uint8, device=dev)
    rc = _lib.lib().tlc_w2_partial_matching(C.c_int32(B), _lib.ptr(xoff.to(torch.int64).contiguous()), _lib.ptr(X) if nx else None,
                                            _lib.ptr(yoff.to(torch.int64).contiguous()), _lib.ptr(Y) if Y.numel() else None,
                                            C.c_int(order), C.c_int32(max_points), _lib.ptr(loss), _lib.ptr(wxy), _lib.ptr(wxd),
                                            _lib.ptr(assign), _lib.ptr(grad), _lib.ptr(status), _lib.stream_ptr())
    _lib.check(rc, "tlc_w2_partial_matching")
    if large == "device" and max_points > _lib.W2_LDS_NMAX:
        w2_large_matching(xoff, X, yoff, Y, order=order, infer=False, min_rows=_lib.W2_LDS_NMAX, want_grad=want_grad,
                          _out=dict(loss=loss, wxy=wxy, wxd=wxd, wyd=None, assign_x=assign, assign_y=None, grad=grad, status=status))
    return dict(loss=loss[:B], wxy=wxy[:B], wxd=wxd[:B], assign=assign[:nx], grad=None if grad is None else grad[:nx], status=status[:B])


@_lib.on_device_of
def w2_inference_matching(xoff, X, yoff, Y, order=2, want_grad=False, max_points=None, large="refuse"):
    """The evaluation distance of PDGNN (`wasserstein_distance_inference`, Knowledge_Distillation/wasserstein.py:93-195: both
    diagrams may use the diagonal) for a batch of (predicted, target) pairs.
    -> dict(loss[B], wxy[B], wxd[B], wyd[B], assign_x[sum n], assign_y[sum m], grad or None, status[B]).
    large: 'refuse': a pair of more than 4 096 points in all gets status 2; 'device': a second call (`w2_large_matching` with
    min_rows = 4096) solves those of up to 65 536 into the same tensors."""
    check_w2_large(large)
    torch = _lib.require_gpu()
    B = xoff.numel() - 1
    dev = X.device
    X = X.to(torch.float64).contiguous()
    Y = Y.to(torch.float64).contiguous()
    xoff = xoff.to(torch.int64).contiguous()
    yoff = yoff.to(torch.int64).contiguous()
    nx, ny = int(X.shape[0]), int(Y.shape[0])
    if B > 0:
        ends = torch.stack([xoff[-1], yoff[-1]]).tolist()
        if ends[0] > nx or ends[1] > ny:
            raise ValueError("w2_inference_matching: offsets end at (%d, %d) but X / Y hold (%d, %d) points" % (ends[0], ends[1], nx, ny))
    if max_points is None:
        max_points = int(((xoff[1:] - xoff[:-1]) + (yoff[1:] - yoff[:-1])).max().item()) if B > 0 else 0
    loss = torch.zeros(max(B, 1), dtype=torch.float64, device=dev)
    wxy, wxd, wyd = torch.zeros_like(loss), torch.zeros_like(loss), torch.zeros_like(loss)
    ax = torch.full((max(nx, 1),), -1, dtype=torch.int32, device=dev)
    ay = torch.full((max(ny, 1),), -1, dtype=torch.int32, device=dev)
    grad = torch.zeros((max(nx, 1), 2), dtype=torch.float64, device=dev) if want_grad else None
    status = torch.zeros(max(B, 1), dtype=torch.uint8, device=dev)
    rc = _lib.lib().tlc_w2_inference_matching(C.c_int32(B), _lib.ptr(xoff), _lib.ptr(X) if nx else None, _lib.ptr(yoff),
                                              _lib.ptr(Y) if ny else None, C.c_int(order), C.c_int32(max_points), _lib.ptr(loss),
                                              _lib.ptr(wxy), _lib.ptr(wxd), _lib.ptr(wyd), _lib.ptr(ax), _lib.ptr(ay), _lib.ptr(grad),
                                              _lib.ptr(status), _lib.stream_ptr())
    _lib.check(rc, "tlc_w2_inference_matching")
    if large == "device" and max_points > _lib.W2_LDS_NMAX:
        w2_large_matching(xoff, X, yoff, Y, order=order, infer=True, min_rows=_lib.W2_LDS_NMAX, want_grad=want_grad,
                          _out=dict(loss=loss, wxy=wxy, wxd=wxd, wyd=wyd, assign_x=ax, assign_y=ay, grad=grad, status=status))
    return dict(loss=loss[:B], wxy=wxy[:B], wxd=wxd[:B], wyd=wyd[:B], assign_x=ax[:nx], assign_y=ay[:ny],
                grad=None if grad is None else grad[:nx], status=status[:B])


W2_LARGE_MAX_WORK_BYTES, W2_LARGE_MAX_SLOTS = 2 << 30, 256          # the most workspace w2_large_matching allocates, and slots in it


def check_w2_large(large):
    if large not in ("refuse", "device"):
        raise ValueError("large / w2_large should be 'refuse' or 'device', not %r" % (large,))


def w2_large_rows(xoff, yoff, infer, min_rows=0):
    """(rows of the largest problem `tlc_w2_large_matching` would solve, number of problems it would take) from the offsets: one host
    read.  It takes the problems of more than min_rows rows and solves those of them up to W2_LARGE_NMAX (training form: with n >= m)."""
    n = (xoff[1:] - xoff[:-1]).to("cpu")
    m = (yoff[1:] - yoff[:-1]).to("cpu")
    N = n + m if infer else n
    taken = N > min_rows
    solved = taken & (N <= _lib.W2_LARGE_NMAX) & ((n >= m) if not infer else (N >= 0))
    return (int(N[solved].max()) if bool(solved.any()) else 0), int(taken.sum())


@_lib.on_device_of
def w2_large_matching(xoff, X, yoff, Y, order=2, infer=False, min_rows=0, want_grad=True, work=None, _out=None):
    """The matching loss of `w2_partial_matching` (infer=False) / `w2_inference_matching` (infer=True) for problems of up to 65 536 rows
    (predicted points; with infer, predicted + target points): `tlc_w2_large_matching`, the workspace tier of csrc/w2_large.hip.
    A problem of at most min_rows rows is left alone (0: every problem that has a row is solved; -1: those without rows too).
    work: a uint8 CUDA tensor (256-byte aligned) of at least `tlc_w2_large_work_bytes(largest problem, 1)` bytes; by default one slot
    per problem taken, up to W2_LARGE_MAX_SLOTS slots and W2_LARGE_MAX_WORK_BYTES.  The result does not depend on it.
    -> dict(loss[B], wxy[B], wxd[B], wyd[B] or None, assign_x[sum n], assign_y[sum m] or None, grad or None, status[B], work)."""
    torch = _lib.require_gpu()
    B = xoff.numel() - 1
    dev = X.device
    X = X.to(torch.float64).contiguous()
    Y = Y.to(torch.float64).contiguous()
    xoff = xoff.to(torch.int64).contiguous()
    yoff = yoff.to(torch.int64).contiguous()
    nx, ny = int(X.shape[0]), int(Y.shape[0])
    rows = taken = 0
    if B > 0:
        ends = torch.stack([xoff[-1], yoff[-1]]).tolist()
        if ends[0] > nx or ends[1] > ny:
            raise ValueError("w2_large_matching: offsets end at (%d, %d) but X / Y hold (%d, %d) points" % (ends[0], ends[1], nx, ny))
        rows, taken = w2_large_rows(xoff, yoff, infer, min_rows)
    if _out is None:
        loss = torch.zeros(max(B, 1), dtype=torch.float64, device=dev)
        _out = dict(loss=loss, wxy=torch.zeros_like(loss), wxd=torch.zeros_like(loss), wyd=torch.zeros_like(loss) if infer else None,
                    assign_x=torch.full((max(nx, 1),), -1, dtype=torch.int32, device=dev),
                    assign_y=torch.full((max(ny, 1),), -1, dtype=torch.int32, device=dev) if infer else None,
                    grad=torch.zeros((max(nx, 1), 2), dtype=torch.float64, device=dev) if want_grad else None,
                    status=torch.zeros(max(B, 1), dtype=torch.uint8, device=dev))
    o = _out
    if work is None:
        slot = int(_lib.lib().tlc_w2_large_work_bytes(C.c_int64(rows), C.c_int32(1)))
        slots = max(1, min(taken, W2_LARGE_MAX_SLOTS, W2_LARGE_MAX_WORK_BYTES // slot))
        work = torch.empty(slot * slots, dtype=torch.uint8, device=dev)
    rc = _lib.lib().tlc_w2_large_matching(C.c_int32(B), _lib.ptr(xoff), _lib.ptr(X) if nx else None, _lib.ptr(yoff), _lib.ptr(Y) if ny else None,
                                          C.c_int(order), C.c_int(1 if infer else 0), C.c_int32(min_rows), _lib.ptr(o["loss"]), _lib.ptr(o["wxy"]),
                                          _lib.ptr(o["wxd"]), _lib.ptr(o["wyd"]), _lib.ptr(o["assign_x"]), _lib.ptr(o["assign_y"]),
                                          _lib.ptr(o["grad"]), _lib.ptr(o["status"]), _lib.ptr(work), C.c_int64(work.numel()), _lib.stream_ptr())
    _lib.check(rc, "tlc_w2_large_matching")
    return dict(loss=o["loss"][:B], wxy=o["wxy"][:B], wxd=o["wxd"][:B], wyd=None if o["wyd"] is None else o["wyd"][:B],
                assign_x=o["assign_x"][:nx], assign_y=None if o["assign_y"] is None else o["assign_y"][:ny],
                grad=None if o["grad"] is None else o["grad"][:nx], status=o["status"][:B], work=work)


_BN_STATUS = "2 = more than %d points in one pair (TLC_BN_NMAX, the cap of tlc_bottleneck_matching), 3 = NaN / Inf coordinates" % _lib.BN_NMAX


@_lib.on_device_of
def bottleneck_matching(xoff, X, yoff, Y, want_grad=False, grad_target=False, check=True):
    """The bottleneck distance d_B (both diagrams may use the diagonal; include/tlcgnn.h defines it) for a batch of (predicted, target)
    diagram pairs: xoff / yoff int64[B+1] offsets, X / Y float64[., 2] CUDA tensors; a pair holds at most _lib.BN_NMAX = 4 096 points.
    -> dict(dist[B], arg int32[B, 2] (the pair that attains it, -1 = diagonal), assign_x[sum n], assign_y[sum m] (a matching that attains
    it), grad[sum n, 2] or None (want_grad), grad_target[sum m, 2] or None (grad_target), status[B]).
    A pair above the cap (status 2) or with a NaN / Inf coordinate (status 3) raises RuntimeError; check=False returns the statuses
    instead (one host read less)."""
    torch = _lib.require_gpu()
    B = xoff.numel() - 1
    dev = X.device
    X = X.to(torch.float64).contiguous()
    Y = Y.to(torch.float64).contiguous()
    xoff = xoff.to(torch.int64).contiguous()
    yoff = yoff.to(torch.int64).contiguous()
    if yoff.numel() != xoff.numel():
        raise ValueError("bottleneck_matching: xoff and yoff describe %d and %d problems" % (B, yoff.numel() - 1))
    nx, ny = int(X.shape[0]), int(Y.shape[0])
    max_points = 0
    if B > 0:
        # (offsets beyond the arrays would be read out of bounds on the device; one host read, with max_points)
        ends = torch.stack([xoff[-1], yoff[-1], ((xoff[1:] - xoff[:-1]) + (yoff[1:] - yoff[:-1])).max()]).tolist()
        if ends[0] > nx or ends[1] > ny:
            raise ValueError("bottleneck_matching: offsets end at (%d, %d) but X / Y hold (%d, %d) points" % (ends[0], ends[1], nx, ny))
        max_points = min(max(int(ends[2]), 0), 0x7fffffff)
    dist = torch.zeros(max(B, 1), dtype=torch.float64, device=dev)
    arg = torch.full((max(B, 1), 2), -1, dtype=torch.int32, device=dev)
    ax = torch.full((max(nx, 1),), -1, dtype=torch.int32, device=dev)
    ay = torch.full((max(ny, 1),), -1, dtype=torch.int32, device=dev)
    gx = torch.zeros((max(nx, 1), 2), dtype=torch.float64, device=dev) if want_grad else None
    gy = torch.zeros((max(ny, 1), 2), dtype=torch.float64, device=dev) if grad_target else None
    status = torch.zeros(max(B, 1), dtype=torch.uint8, device=dev)
    rc = _lib.lib().tlc_bottleneck_matching(C.c_int32(B), _lib.ptr(xoff), _lib.ptr(X) if nx else None, _lib.ptr(yoff), _lib.ptr(Y) if ny else None,
                                            C.c_int32(max_points), _lib.ptr(dist), _lib.ptr(arg), _lib.ptr(ax), _lib.ptr(ay), _lib.ptr(gx),
                                            _lib.ptr(gy), _lib.ptr(status), _lib.stream_ptr())
    _lib.check(rc, "tlc_bottleneck_matching")
    if check and B > 0 and bool((status[:B] != 0).any()):
        bad = torch.nonzero(status[:B]).flatten()
        raise RuntimeError("bottleneck_matching: problem %d has status %d (%s)" % (int(bad[0]), int(status[bad[0]]), _BN_STATUS))
    return dict(dist=dist[:B], arg=arg[:B], assign_x=ax[:nx], assign_y=ay[:ny], grad=None if gx is None else gx[:nx],
                grad_target=None if gy is None else gy[:ny], status=status[:B])


def sliced_directions(M=50):
    """The directions and the step of the reference's sliced loss, exactly as Knowledge_Distillation/Teacher_model.py:117-124 makes
    them: theta starts at 0.5 and accumulates step = 1.0 / M; direction i is (float32(cos(theta pi)), float32(sin(theta pi))) -- the
    FloatTensor of :120 -- widened to float64.  -> (float64[M, 2] numpy array, scale = step)."""
    import numpy as np
    M = int(M)
    if M < 1:
        raise ValueError("sliced_directions: M should be at least 1, not %d" % M)
    dirs = np.empty((M, 2), dtype=np.float64)
    theta = 0.5
    step = 1.0 / M
    for i in range(M):
        dirs[i, 0] = np.float32(np.cos(theta * np.pi))
        dirs[i, 1] = np.float32(np.sin(theta * np.pi))
        theta += step
    return dirs, step


SLICED_W_WORK_CAP = 1 << 30     # what sliced_wasserstein allocates at most by default (unless one direction alone needs more)


def sliced_w_work_bytes(n_problems, total_points, max_points, n_dirs):
    """Bytes of workspace that run all n_dirs directions of the largest problem at once (tlc_sliced_w_work_bytes: host arithmetic);
    0 when no problem has more than _lib.SW_LDS_NMAX points."""
    need = _lib.lib().tlc_sliced_w_work_bytes(C.c_int32(int(n_problems)), C.c_int64(int(total_points)), C.c_int64(int(max_points)),
                                              C.c_int32(int(n_dirs)))
    if need < 0:
        _lib.check(1, "tlc_sliced_w_work_bytes")                 # TLC_ERR_INVALID_ARG: the message is the library's
    return int(need)


@_lib.on_device_of
def sliced_wasserstein(xoff, X, yoff, Y, dirs=None, scale=None, M=50, want_grad=("x",), work_bytes=None):
    """The sliced Wasserstein distance (Teacher_model.py:110-124 `compute_PD_loss(kernel='sliced')`; include/tlcgnn.h defines it)
    for a batch of diagram pairs of any size: xoff / yoff int64[B+1] offsets, X / Y float64[., 2] CUDA tensors.  dirs float64[M, 2]
    and scale default to `sliced_directions(M)`.  want_grad: which of 'x', 'y' get a gradient.  work_bytes: the size of the workspace
    of the problems above _lib.SW_LDS_NMAX points, allocated per call from torch's caching allocator (a training loop gets the same
    block back): about 66 B x directions x points of the largest problem to sort all directions at once (290 MB for 88 650 points at
    M = 50), at least the size of one direction; any size in between gives the same bits, in more launches.  None: all directions at
    once up to SLICED_W_WORK_CAP bytes, beyond it the cap (or one direction, where that is larger).
    -> dict(loss[B], grad_x[sum n, 2] or None, grad_y[sum m, 2] or None, status[B]: 0 ok, 3 = NaN / Inf coordinates)."""
    import torch
    B = xoff.numel() - 1
    dev = X.device
    xoff = xoff.to(torch.int64).contiguous()
    yoff = yoff.to(torch.int64).contiguous()
    if yoff.numel() != xoff.numel():
        raise ValueError("sliced_wasserstein: xoff and yoff describe %d and %d problems" % (B, yoff.numel() - 1))
    nx, ny = int(X.shape[0]), int(Y.shape[0])
    max_points = total = 0
    if B > 0:
        # (offsets beyond the arrays would be read out of bounds on the device; one host read, with the sizes the entry wants)
        cnt = (xoff[1:] - xoff[:-1]) + (yoff[1:] - yoff[:-1])
        ends = torch.stack([xoff[-1], yoff[-1], cnt.max(), cnt.sum()]).tolist()
        if ends[0] > nx or ends[1] > ny:
            raise ValueError("sliced_wasserstein: offsets end at (%d, %d) but X / Y hold (%d, %d) points" % (ends[0], ends[1], nx, ny))
        max_points, total = max(int(ends[2]), 0), max(int(ends[3]), 0)
    _lib.require_gpu()
    X = X.to(torch.float64).contiguous()
    Y = Y.to(torch.float64).contiguous()
    if dirs is None:
        d_np, step = sliced_directions(M)
        dirs = torch.from_numpy(d_np)
        if scale is None:
            scale = step
    elif scale is None:
        raise ValueError("sliced_wasserstein: dirs without a scale")
    dirs = torch.as_tensor(dirs, dtype=torch.float64).to(dev).contiguous()
    if dirs.dim() != 2 or dirs.shape[1] != 2:
        raise ValueError("sliced_wasserstein: dirs should be [M, 2], not %s" % (tuple(dirs.shape),))
    n_dirs = int(dirs.shape[0])
    want = set(want_grad or ())
    if not want <= {"x", "y"}:
        raise ValueError("sliced_wasserstein: want_grad holds 'x' and / or 'y', not %r" % (want_grad,))
    loss = torch.zeros(max(B, 1), dtype=torch.float64, device=dev)
    gx = torch.zeros((max(nx, 1), 2), dtype=torch.float64, device=dev) if "x" in want else None
    gy = torch.zeros((max(ny, 1), 2), dtype=torch.float64, device=dev) if "y" in want else None
    status = torch.zeros(max(B, 1), dtype=torch.uint8, device=dev)
    L = _lib.lib()
    if work_bytes is None:
        work_bytes = L.tlc_sliced_w_work_bytes(C.c_int32(B), C.c_int64(total), C.c_int64(max_points), C.c_int32(n_dirs))
        work_bytes = max(int(work_bytes), 0)                    # (a refused n_dirs is reported by the call below)
        if work_bytes > SLICED_W_WORK_CAP:
            work_bytes = max(SLICED_W_WORK_CAP, int(L.tlc_sliced_w_work_bytes(C.c_int32(B), C.c_int64(total), C.c_int64(max_points), C.c_int32(1))))
    work = torch.empty(int(work_bytes), dtype=torch.uint8, device=dev) if work_bytes > 0 else None
    rc = L.tlc_sliced_wasserstein(C.c_int32(B), _lib.ptr(xoff), _lib.ptr(X) if nx else None, _lib.ptr(yoff), _lib.ptr(Y) if ny else None,
                                  C.c_int32(n_dirs), _lib.ptr(dirs), C.c_double(float(scale)), C.c_int64(max_points), _lib.ptr(loss),
                                  _lib.ptr(gx), _lib.ptr(gy), _lib.ptr(status), _lib.ptr(work), C.c_int64(int(work_bytes)), _lib.stream_ptr())
    _lib.check(rc, "tlc_sliced_wasserstein")
    return dict(loss=loss[:B], grad_x=None if gx is None else gx[:nx], grad_y=None if gy is None else gy[:ny], status=status[:B])


def landscape(pts, offs, ts, K=5, winners=True, work=None, check=True):
    """Persistence landscapes [B, K, T] of packed diagrams (include/tlcgnn.h defines them; `engine.landscape`): pts [sum n, 2] of any
    float dtype, offs int64[B + 1] (None: one diagram), ts [T] sample values, on one CUDA device; computed in float64.
    -> dict(out float64[B, K, T], winner int32[B, K, T] or None, status uint8[B]).  A diagram with a NaN / Inf coordinate (status 3)
    raises RuntimeError naming it unless check=False."""
    import torch
    from . import engine
    if not torch.is_tensor(ts) or ts.dim() != 1:
        raise ValueError("landscape: ts should be a 1-D tensor, not %s" % (tuple(ts.shape) if torch.is_tensor(ts) else type(ts).__name__,))
    if offs is None:
        offs = torch.tensor([0, pts.shape[0]], dtype=torch.int64, device=pts.device)
    out, win, status = engine.landscape(pts.detach().to(torch.float64).reshape(-1, 2), offs.to(torch.int64), ts.detach().to(torch.float64), K,
                                        winners=winners, work=work)
    if check and status.numel() and bool((status != 0).any()):
        bad = torch.nonzero(status).flatten()
        raise RuntimeError("landscape: diagram %d has status %d (3 = a NaN / Inf coordinate)" % (int(bad[0]), int(status[bad[0]])))
    return dict(out=out, winner=win, status=status)


DGM_KERNELS = ("pss", "gauss")


def dgm_kernel_params(kernel, sigma):
    """-> (gamma, scale, mirror) of include/tlcgnn.h's function for a named kernel between diagrams: 'pss', the persistence scale-space
    kernel with bandwidth sigma (gamma = 1 / (8 sigma), scale = 1 / (8 pi sigma), the mirror term); 'gauss', the plain Gaussian of the
    persistence weighted Gaussian kernel (gamma = 1 / (2 sigma^2), scale = 1, no mirror; its weights are `pwg_weights`)."""
    import math
    sigma = float(sigma)
    if not (math.isfinite(sigma) and sigma > 0.0):
        raise ValueError("diagram kernel: sigma should be finite and > 0, not %r" % (sigma,))
    if kernel == "pss":
        return 1.0 / (8.0 * sigma), 1.0 / (8.0 * math.pi * sigma), True
    if kernel == "gauss":
        return 1.0 / (2.0 * sigma * sigma), 1.0, False
    raise ValueError("diagram kernel: kernel should be one of %s, not %r" % (DGM_KERNELS, kernel))


def pwg_weights(pts, C=1.0, p=1.0):
    """arctan(C * persistence^p) per point of pts [n, 2], the weights of the persistence weighted Gaussian kernel (Kusano et al. 2016):
    plain torch ops, so C and p may be tensors that require grad."""
    import torch
    return torch.atan(C * (pts[:, 1] - pts[:, 0]) ** p)


def dgm_raise_on_status(what, status_x, status_y):
    """RuntimeError naming the first diagram whose status is not 0 (3 = a NaN / Inf coordinate or weight)."""
    import torch
    for name, st in (("x", status_x), ("y", status_y)):
        if st is not None and st.numel() and bool((st != 0).any()):
            bad = int(torch.nonzero(st).flatten()[0])
            raise RuntimeError("%s: diagram %d of %s has status %d (3 = a NaN / Inf coordinate or weight)" % (what, bad, name, int(st[bad])))


def diagram_gram(x, xoff, y=None, yoff=None, wx=None, wy=None, kernel="pss", sigma=1.0, paired=False, work=None, check=True):
    """The Gram matrix of a kernel between packed persistence diagrams (`engine.dgm_gram`; include/tlcgnn.h defines the function):
    x [sum n, 2] of any float dtype with xoff int64[Bx + 1] (None: one diagram) against y / yoff, every pair ([Bx, By]) or, with
    paired=True, diagram i against diagram i ([B]); computed in float64.  y=None: X against itself -- symmetric, only j >= i computed
    (paired: k(X_i, X_i)).  kernel / sigma: `dgm_kernel_params`; wx / wy: optional weights per point (`pwg_weights`).
    -> dict(out, status_x, status_y).  A diagram with a NaN / Inf coordinate or weight (status 3) raises RuntimeError naming it unless
    check=False (its row / column is NaN then)."""
    import torch
    from . import engine
    gamma, scale, mirror = dgm_kernel_params(kernel, sigma)
    if y is None and (yoff is not None or wy is not None):
        raise ValueError("diagram_gram: yoff / wy without y")

    def side(pts, offs, w):
        pts = pts.detach().to(torch.float64).reshape(-1, 2).contiguous()
        if offs is None:
            offs = torch.tensor([0, pts.shape[0]], dtype=torch.int64, device=pts.device)
        return pts, offs.to(torch.int64).contiguous(), None if w is None else w.detach().to(torch.float64).reshape(-1).contiguous()

    X = side(x, xoff, wx)
    Y = X if y is None else side(y, yoff, wy)
    out, sx, sy = engine.dgm_gram(*X, *Y, gamma, scale, mirror, paired=paired, symmetric=(y is None and not paired), work=work)
    if check:
        dgm_raise_on_status("diagram_gram", sx, None if y is None else sy)
    return dict(out=out, status_x=sx, status_y=sy)


def capture(fn, warmup=2):
    """HIP graph of a forward closure: `fn` (C-ABI launches on the current stream, outputs in caller-held or graph-pool buffers,
    no host synchronisation inside) is warmed up on a side stream, captured once, and replayed with `.replay()`.
    torch.cuda.CUDAGraph is hipStreamBeginCapture / hipGraphLaunch plumbing.  Every LP-forward entry point of the C ABI is
    capturable (tests/test_gpu_lp_forward.py).  Measured on the PubMed forward (five kernels, 70 us of kernel time): replay
    86 us vs 78 us launched kernel by kernel from Python -- ROCm's graph launch costs more than the launch gaps it removes, so
    bench.py does not use it."""
    torch = _lib.require_gpu()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(warmup):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph

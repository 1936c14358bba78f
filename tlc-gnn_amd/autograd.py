"""Autograd glue for PDGNN training: `loss.backward()` of the reference's training loop
(Knowledge_Distillation/train_Teacher_Model.py:55-62) through the HIP kernels; and for the TLCGNN link-prediction step
(pipelines.py:10-18): GcnLayer and LpDecode, used by pipelines.train through Net's private training forward; and for the node
classifier of Knowledge_Distillation/ConvCurv_GIN.py: CurvConv and NcLinear (nc_curv.hip).

torch.autograd only carries the graph: every forward and every backward below is one C-ABI call (`tlc_gat_layer_fwd/_bwd`,
`tlc_msg_layer_fwd/_bwd`, `tlc_edge_head_fwd/_bwd`, `tlc_w2_partial_matching`, `tlc_sliced_wasserstein`, `tlc_bottleneck_matching`, `tlc_pi_raster` / `tlc_pi_raster_wgrad`, `tlc_pi_image` / `tlc_pi_image_vjp`, `tlc_landscape` / `tlc_landscape_vjp`, `tlc_dgm_gram` / `tlc_dgm_gram_vjp`, `tlc_hks_batch_dt` + `tlc_hks_large_batch_dt`) or a few (`tlc_gemm_f32` /
`tlc_spmm_csr_f32` / `tlc_gemm_tn_f32`, `tlc_lp_decode_fused_f32` / `tlc_lp_decode_bwd_f32` / `tlc_lp_decode_bwd_pi_f32`, `tlc_segment_sum_f64`); nothing is recomputed with torch ops
and there is no CPU path.
"""
import torch

from . import _lib, ops, engine


class GatLayer(torch.autograd.Function):
    """One PDGNN layer (gat_conv.py:113-216) with the PReLU that follows it in Base_Model.forward (Teacher_model.py:218-219)."""

    @staticmethod
    def forward(ctx, x, wl, att, wij, bias, rowptr, src, prelu_slope):
        out = ops.gat_layer(rowptr, src, x, wl, att, wij, bias, prelu_slope=prelu_slope)
        ctx.save_for_backward(x, wl, att, wij, out, rowptr, src)
        ctx.prelu_slope = prelu_slope
        ctx.att_shape = att.shape
        return out

    @staticmethod
    def backward(ctx, gout):
        x, wl, att, wij, out, rowptr, src = ctx.saved_tensors
        gx, gwl, gatt, gwij, gbias = ops.gat_layer_bwd(rowptr, src, x, wl, att, wij, ctx.prelu_slope, out, gout.contiguous(),
                                                       need_gx=ctx.needs_input_grad[0])
        return gx, gwl, gatt.reshape(ctx.att_shape), gwij, gbias, None, None, None


class EdgeHead(torch.autograd.Function):
    """lin6(prelu(lin5([x_s || x_t]))) per edge (Teacher_model.py:54-59)."""

    @staticmethod
    def forward(ctx, x, w5, b5, w6, b6, src, dst, prelu_slope):
        pd = ops.edge_head(src, dst, x, w5, b5, prelu_slope, w6, b6)
        ctx.save_for_backward(x, w5, b5, w6, src, dst)
        ctx.prelu_slope = prelu_slope
        return pd

    @staticmethod
    def backward(ctx, gpd):
        x, w5, b5, w6, src, dst = ctx.saved_tensors
        gx, gw5, gb5, gw6, gb6 = ops.edge_head_bwd(src, dst, x, w5, b5, ctx.prelu_slope, w6, gpd.contiguous())
        return gx, gw5, gb5, gw6, gb6, None, None, None


class GnnLayer(torch.autograd.Function):
    """One layer of the teacher's GIN / GCN / SAGE baselines (Teacher_model.py:148-175,202-208) with the activation that follows it:
    `tlc_gnn_layer_fwd`, and `tlc_gnn_layer_bwd` on the structure's transpose (no atomics).  `batch`: a gnn_layers.GnnBatch."""

    @staticmethod
    def forward(ctx, x, wa, ws, bias, batch, act, slope):
        out, agg = ops.gnn_layer(batch.rowptr, batch.src, batch.coef, batch.self_scale, x, wa, ws, bias, act, slope, want_agg=True)
        ctx.save_for_backward(x, agg, out, wa, ws)
        ctx.batch, ctx.act, ctx.slope, ctx.has_bias = batch, act, slope, bias is not None
        return out

    @staticmethod
    def backward(ctx, gout):
        x, agg, out, wa, ws = ctx.saved_tensors
        b = ctx.batch
        rowptr_t, col_t, coef_t = b.transpose() if ctx.needs_input_grad[0] else (None, None, None)
        gx, gwa, gws, gb = ops.gnn_layer_bwd(rowptr_t, col_t, coef_t, b.self_scale, x, agg, out, gout.contiguous(), wa, ws, ctx.has_bias,
                                             ctx.act, ctx.slope, need_gx=ctx.needs_input_grad[0])
        return gx, gwa, gws, gb, None, None, None


class MsgLayer(torch.autograd.Function):
    """One layer of the PDGNN family (GATConv's ablations, PDConv) with the PReLU that follows it: `tlc_msg_layer_fwd`, and
    `tlc_msg_layer_bwd` (no floating-point atomics) on the structure and its transpose.  `batch`: a gat_conv.GraphBatch.  att / wij may
    be None when their switch is off; their gradient is then None."""

    @staticmethod
    def forward(ctx, x, wl, att, wij, bias, batch, mode, agg, prelu_slope):
        out = ops.msg_layer(batch.rowptr, batch.col, x, wl, att, wij, bias, mode, agg, prelu_slope)
        ctx.save_for_backward(x, wl, att, wij, out)
        ctx.batch, ctx.mode, ctx.agg, ctx.prelu_slope = batch, mode, agg, prelu_slope
        return out

    @staticmethod
    def backward(ctx, gout):
        x, wl, att, wij, out = ctx.saved_tensors
        b = ctx.batch
        rowptr_t, col_t, pos_t = b.transpose()
        gx, gwl, gatt, gwij, gbias = ops.msg_layer_bwd(b.rowptr, b.col, rowptr_t, col_t, pos_t, x, wl, att, wij, ctx.mode, ctx.agg, ctx.prelu_slope,
                                                       out, gout.contiguous(), need_gx=ctx.needs_input_grad[0])
        # (ops.msg_layer_bwd returns None for gatt / gwij exactly when att / wij were None: their switch is off)
        return gx, gwl, (None if gatt is None else gatt.reshape(att.shape)), gwij, gbias, None, None, None, None


_W2_STATUS = "1 = fewer predicted than target points, 2 = too many points for one problem (%s), 3 = NaN / Inf coordinates"
_W2_CAP = {"refuse": "4096; large='device' takes up to 65536", "device": "65536"}


class DiagramLoss(torch.autograd.Function):
    """`wasserstein_distance(PD_hat, PD, order=p, enable_autodiff=True, num_models=1)` (wasserstein.py:198-379) of one or more
    (predicted, target) pairs: -> (loss [B], wxy [B], wxd [B]); only `loss` carries a gradient, like the reference's
    (wxy / wxd are the logged parts).

    infer=True: `wasserstein_distance_inference` (wasserstein.py:93-195, both diagrams may use the diagonal)
    -> (loss, wxy, wxd, wyd)."""

    @staticmethod
    def forward(ctx, pd_hat, xoff, target, yoff, order, infer, large="refuse"):
        if infer:
            r = ops.w2_inference_matching(xoff, pd_hat.detach(), yoff, target, order=order, want_grad=True, large=large)
        else:
            r = ops.w2_partial_matching(xoff, pd_hat.detach(), yoff, target, order=order, want_grad=True, large=large)
        bad = r["status"] != 0
        if bool(bad.any()):
            raise ValueError("diagram loss: status %s (%s)" % (r["status"].tolist(), _W2_STATUS % _W2_CAP[large]))
        ctx.save_for_backward(r["grad"], xoff)
        dt = pd_hat.dtype
        ctx.dtype = dt
        # (the tensors RETURNED are marked: a cast makes new ones, and a mark on the float64 originals would be lost)
        parts = [r[k].to(dt) for k in (("wxy", "wxd", "wyd") if infer else ("wxy", "wxd"))]
        ctx.mark_non_differentiable(*parts)
        return (r["loss"].to(dt),) + tuple(parts)

    @staticmethod
    def backward(ctx, gloss, *_unused):
        grad, xoff = ctx.saved_tensors
        cnt = xoff[1:] - xoff[:-1]
        per_point = torch.repeat_interleave(gloss.to(torch.float64), cnt)          # d total / d loss[b] for each predicted point
        return (grad * per_point.unsqueeze(1)).to(ctx.dtype), None, None, None, None, None, None


class SlicedDiagramLoss(torch.autograd.Function):
    """The sliced Wasserstein distance of one or more (predicted, target) diagram pairs (`compute_PD_loss(kernel='sliced')`,
    Teacher_model.py:110-124; include/tlcgnn.h defines it) -> loss [B] in pd_hat's dtype.  One `tlc_sliced_wasserstein` call computes
    the loss and the gradients of both diagrams; the reference's graph reaches the target too (through its projections), so `target`
    gets its gradient when it requires one."""

    @staticmethod
    def forward(ctx, pd_hat, xoff, target, yoff, dirs, scale):
        want = (("x",) if ctx.needs_input_grad[0] else ()) + (("y",) if ctx.needs_input_grad[2] else ())
        r = ops.sliced_wasserstein(xoff, pd_hat.detach(), yoff, target.detach(), dirs=dirs, scale=scale, want_grad=want)
        if bool((r["status"] != 0).any()):
            raise ValueError("sliced diagram loss: status %s (3 = NaN / Inf coordinates)" % r["status"].tolist())
        ctx.save_for_backward(xoff, yoff, r["grad_x"], r["grad_y"])
        ctx.dtypes = (pd_hat.dtype, target.dtype)
        return r["loss"].to(pd_hat.dtype)

    @staticmethod
    def backward(ctx, gloss):
        xoff, yoff, gx, gy = ctx.saved_tensors
        g64 = gloss.to(torch.float64)
        out = [None, None]
        for k, (offs, g) in enumerate(((xoff, gx), (yoff, gy))):
            if g is not None:
                per_point = torch.repeat_interleave(g64, offs[1:] - offs[:-1])   # d total / d loss[b] for each point of problem b
                out[k] = (g * per_point.unsqueeze(1)).to(ctx.dtypes[k])
        return out[0], None, out[1], None, None, None


class BottleneckLoss(torch.autograd.Function):
    """The bottleneck distance of one or more (predicted, target) diagram pairs (include/tlcgnn.h defines it) -> d_B [B] in pd_hat's
    dtype.  One `tlc_bottleneck_matching` call computes the distance and the gradients of both diagrams: +-1 or +-1/2 on the one point
    of each diagram that the attaining pair names (`ops.bottleneck_matching`), a convention where the maximum is tied."""

    @staticmethod
    def forward(ctx, pd_hat, xoff, target, yoff):
        r = ops.bottleneck_matching(xoff, pd_hat.detach(), yoff, target.detach(), want_grad=ctx.needs_input_grad[0],
                                    grad_target=ctx.needs_input_grad[2])
        ctx.save_for_backward(xoff, yoff, r["grad"], r["grad_target"])
        ctx.dtypes = (pd_hat.dtype, target.dtype)
        return r["dist"].to(pd_hat.dtype)

    @staticmethod
    def backward(ctx, gloss):
        xoff, yoff, gx, gy = ctx.saved_tensors
        g64 = gloss.to(torch.float64)
        out = [None, None]
        for k, (offs, g) in enumerate(((xoff, gx), (yoff, gy))):
            if g is not None:
                per_point = torch.repeat_interleave(g64, offs[1:] - offs[:-1])   # d total / d d_B[b] for each point of problem b
                out[k] = (g * per_point.unsqueeze(1)).to(ctx.dtypes[k])
        return out[0], None, out[1], None


class DiagramImage(torch.autograd.Function):
    """The differentiable imager of Teacher_Model.forward(grad_PI=True) (Teacher_model.py:80-81 -> pimg.py:354-400): images of one
    or more predicted diagrams, [B, res*res] in the diagrams' dtype.  The reference detaches the coordinates inside the two
    normal-CDF factors (:392,395), so the gradient reaches a point through its weight only (`tlc_pi_raster_wgrad`)."""

    @staticmethod
    def forward(ctx, pd_hat, offs, res):
        pts = pd_hat.detach().to(torch.float64).contiguous()
        ctx.save_for_backward(pts, offs)
        ctx.res, ctx.dtype = res, pd_hat.dtype
        return engine.pi_raster(offs, pts, res).to(pd_hat.dtype)

    @staticmethod
    def backward(ctx, gimg):
        pts, offs = ctx.saved_tensors
        g = engine.pi_raster_wgrad(offs, pts, gimg.to(torch.float64), ctx.res)
        return g.to(ctx.dtype), None, None


class GeneralDiagramImage(torch.autograd.Function):
    """Images of one or more diagrams under any imager specification (`engine.PiSpec`), [B, Rb * Rp] row-major [birth_bin, pers_bin]
    in the diagrams' dtype: `tlc_pi_image` forward, `tlc_pi_image_vjp` backward.  mode 'weight' is the reference's gradient
    (DiagramImage's, generalised to the ramp's slope), 'full' the true derivative, which also moves a point's position."""

    @staticmethod
    def forward(ctx, pd_hat, offs, spec, mode):
        pts = pd_hat.detach().to(torch.float64).contiguous()
        ctx.save_for_backward(pts, offs)
        ctx.spec, ctx.mode, ctx.dtype = spec, mode, pd_hat.dtype
        return engine.pi_image(offs, pts, spec).to(pd_hat.dtype)

    @staticmethod
    def backward(ctx, gimg):
        pts, offs = ctx.saved_tensors
        g = engine.pi_image_vjp(offs, pts, gimg.to(torch.float64), ctx.spec, ctx.mode)
        return g.to(ctx.dtype), None, None, None


class DiagramLandscape(torch.autograd.Function):
    """Persistence landscapes of one or more diagrams (include/tlcgnn.h defines them), [B, K, T] in the diagrams' dtype:
    `tlc_landscape` forward, `tlc_landscape_vjp` backward over the forward's winners -- a +-1 selection, so the gradient of a cell
    reaches one coordinate of one point.  The points are computed in float64 whatever their dtype; the samples get no gradient."""

    @staticmethod
    def forward(ctx, pd_hat, offs, ts, K):
        pts = pd_hat.detach().to(torch.float64).contiguous()
        r = ops.landscape(pts, offs, ts, K=K, winners=True)
        ctx.save_for_backward(pts, offs, r["winner"])
        ctx.ts, ctx.K, ctx.dtype = ts.detach().to(torch.float64).contiguous(), K, pd_hat.dtype
        return r["out"].to(pd_hat.dtype)

    @staticmethod
    def backward(ctx, gout):
        pts, offs, winner = ctx.saved_tensors
        g = engine.landscape_vjp(pts, offs, ctx.ts, ctx.K, winner, gout.to(torch.float64).contiguous())
        return g.to(ctx.dtype), None, None, None


class DiagramGram(torch.autograd.Function):
    """The Gram matrix of a diagram kernel (include/tlcgnn.h defines it): `tlc_dgm_gram` forward, `tlc_dgm_gram_vjp` backward -- once
    per side that needs a gradient, the second side with the roles swapped and the upstream transposed; y None (X against itself): one
    call with G + G^T (paired: 2 G).  Computed in float64 whatever the dtypes."""

    @staticmethod
    def forward(ctx, x, xoff, wx, y, yoff, wy, gamma, scale, mirror, paired):
        def side(pts, offs, w):
            return (pts.detach().to(torch.float64).reshape(-1, 2).contiguous(), offs.to(torch.int64).contiguous(),
                    None if w is None else w.detach().to(torch.float64).reshape(-1).contiguous())
        same = y is None
        X = side(x, xoff, wx)
        Y = X if same else side(y, yoff, wy)
        out, sx, sy = engine.dgm_gram(*X, *Y, gamma, scale, mirror, paired=paired, symmetric=same and not paired)
        ops.dgm_raise_on_status("diagram_gram", sx, None if same else sy)
        ctx.save_for_backward(*X, *Y, sx, sy)
        ctx.params = (gamma, scale, mirror, paired, same)
        ctx.dtypes = tuple(None if t is None else t.dtype for t in (x, wx, y, wy))
        return out.to(x.dtype)

    @staticmethod
    def backward(ctx, gout):
        xp, xo, xw, yp, yo, yw, sx, sy = ctx.saved_tensors
        gamma, scale, mirror, paired, same = ctx.params
        g = gout.to(torch.float64).contiguous()
        need = ctx.needs_input_grad
        gx = gwx = gy = gwy = None
        if same:
            if need[0] or need[2]:
                gx, gwx = engine.dgm_gram_vjp(xp, xo, xw, xp, xo, xw, gamma, scale, mirror, sx, sx, 2.0 * g if paired else g + g.t(), paired=paired)
        else:
            if need[0] or need[2]:
                gx, gwx = engine.dgm_gram_vjp(xp, xo, xw, yp, yo, yw, gamma, scale, mirror, sx, sy, g, paired=paired)
            if need[3] or need[5]:
                gy, gwy = engine.dgm_gram_vjp(yp, yo, yw, xp, xo, xw, gamma, scale, mirror, sy, sx, g if paired else g.t().contiguous(),
                                              paired=paired)
        cast = lambda t, k, on: t.to(ctx.dtypes[k]) if (t is not None and on) else None        # noqa: E731
        return (cast(gx, 0, need[0]), None, cast(gwx, 1, need[2]), cast(gy, 2, need[3]), None, cast(gwy, 3, need[5]), None, None, None, None)


class ExtendedPersistence(torch.autograd.Function):
    """The exact extended persistence as a differentiable function of the filtration values: (up, down, one, ext0, counts) in the slot
    layout of `engine.pd_from_filtration`, the same values bit for bit.  Every coordinate is a copy of one f[v], so the backward is a
    selection: `engine.pd_point_vertices` finds the vertex of every coordinate after the forward (the lowest id with f[v] == c --
    the critical vertex where a graph's values are distinct, a fixed convention under ties, where the diagram is not differentiable:
    DESIGN.md 6.6), and one `tlc_pd_filtration_grad` sums the point gradients into grad f in a fixed order.  f may be float32 or
    float64: the diagrams are computed in float64 and returned in f's dtype, and so is the gradient."""

    @staticmethod
    def forward(ctx, f, node_offs, edge_offs, edges, flags, pd_large):
        f64 = f.detach().to(torch.float64).contiguous()
        pd = engine.pd_from_filtration(node_offs, edge_offs, edges, f64, flags=flags, want_rank=False, pd_large=pd_large)
        verts = engine.pd_point_vertices(node_offs, edge_offs, f64, pd)
        bad = verts["status"].nonzero().flatten().tolist()
        if bad:
            raise RuntimeError("extended_persistence: graph(s) %s are not computed: status %s (%d = ST_TOO_LARGE: above the cap of "
                               "pd_large='host'; %d = ST_BAD_INPUT)" % (bad, verts["status"][bad].tolist(), _lib.ST_TOO_LARGE, _lib.ST_BAD_INPUT))
        ctx.save_for_backward(node_offs, edge_offs, pd["counts"], verts["up"], verts["down"], verts["one"], verts["ext0"], verts["status"])
        ctx.dtype, ctx.n = f.dtype, f.numel()
        ctx.mark_non_differentiable(pd["counts"])
        return tuple(pd[k].to(f.dtype) for k in engine.VERTEX_KEYS) + (pd["counts"],)

    @staticmethod
    def backward(ctx, g_up, g_down, g_one, g_ext0, _g_counts):
        node_offs, edge_offs, counts, v_up, v_down, v_one, v_ext0, status = ctx.saved_tensors
        verts = dict(up=v_up, down=v_down, one=v_one, ext0=v_ext0, status=status)
        g = engine.pd_filtration_grad(node_offs, edge_offs, counts, verts, g_up, g_down, g_one, g_ext0)
        return g[:ctx.n].to(ctx.dtype), None, None, None, None, None


def extended_persistence(f, node_offs, edge_offs, edges, flags=_lib.KEEP_ZERO_PERS, pd_large="host"):
    """-> (up, down, one, ext0, counts): the diagrams of `engine.pd_from_filtration` in slot layout, differentiable in f (counts is
    not).  A graph that is not computed raises RuntimeError naming it."""
    engine.check_pd_large(pd_large)
    return ExtendedPersistence.apply(f, node_offs, edge_offs, edges, int(flags), pd_large)


class HksSignature(torch.autograd.Function):
    """Heat-kernel signatures of a packed batch as a differentiable function of the diffusion times: float64[T, sum n], the values of
    `engine.hks_batch` / `engine.hks_large_batch` bit for bit, with d / d t from the same kernels (tlc_hks_batch_dt, then
    tlc_hks_large_batch_dt for the graphs above HKS_NMAX nodes, then with hks_sparse='device' tlc_hks_sparse_batch_dt
    (`engine.hks_sparse_batch`) for what is still ST_TOO_LARGE).  The gradient is in `times` only:
    grad_times[k] = sum(grad[k] * d out[k] / d t)."""

    @staticmethod
    def forward(ctx, times, node_ptr, edge_ptr, edges, normalise, hks_sparse='host'):
        host = [float(t) for t in times.detach().to(torch.float64).cpu().tolist()]    # the one read of the times
        B = node_ptr.numel() - 1
        tot_n = int(node_ptr[-1]) if B > 0 else 0
        out, dout, st = engine.hks_batch(node_ptr, edge_ptr, edges, host, normalise=normalise, total_nodes=tot_n, dt=True)
        st_h = st.cpu()
        rest = torch.nonzero(st_h != _lib.ST_OK).flatten()
        if rest.numel():
            sizes = (node_ptr[1:] - node_ptr[:-1]).cpu()[rest]
            take = (st_h[rest] == _lib.ST_TOO_LARGE) & (sizes <= _lib.HKS_LARGE_NMAX)
            if bool(take.any()):
                bad_t = [t for t in host if not 0.0 <= t <= _lib.HKS_LARGE_TIME_MAX]     # (a NaN fails both comparisons)
                if bad_t:
                    raise RuntimeError("hks_signature: graph(s) %s have more than %d nodes (status %d = ST_TOO_LARGE) and their tier takes "
                                       "times inside [0, %g], not %s" % (rest[take].tolist(), _lib.HKS_NMAX, _lib.ST_TOO_LARGE,
                                                                         _lib.HKS_LARGE_TIME_MAX, bad_t))
                engine.hks_large_batch(node_ptr, edge_ptr, edges, rest[take].tolist(), sizes[take].tolist(), host, normalise=normalise,
                                       total_nodes=tot_n, out=out, status=st, dout=dout)
                st_h = st.cpu()
            wide = torch.nonzero(st_h == _lib.ST_TOO_LARGE).flatten()
            if hks_sparse == 'device' and wide.numel():        # what the large tier does not take: tlc_hks_sparse_batch_dt, any node count
                bad_t = [t for t in host if not 0.0 <= t <= _lib.HKS_SPARSE_TIME_MAX]
                if bad_t:
                    raise RuntimeError("hks_signature: graph(s) %s are still too large after the other tiers (status %d = ST_TOO_LARGE) and the "
                                       "sparse tier takes times inside [0, %g], not %s"
                                       % (wide.tolist(), _lib.ST_TOO_LARGE, _lib.HKS_SPARSE_TIME_MAX, bad_t))
                engine.hks_sparse_batch(node_ptr, edge_ptr, edges, wide.tolist(), (node_ptr[1:] - node_ptr[:-1]).cpu()[wide].tolist(),
                                        (edge_ptr[1:] - edge_ptr[:-1]).cpu()[wide].tolist(), host, normalise=normalise, total_nodes=tot_n,
                                        out=out, status=st, dout=dout)
                st_h = st.cpu()
            bad = torch.nonzero(st_h != _lib.ST_OK).flatten().tolist()
            if bad:
                raise RuntimeError("hks_signature: graph(s) %s are not computed: status %s (%d = ST_TOO_LARGE: more than %d nodes; %d = "
                                   "ST_NOT_CONVERGED; %d = ST_BAD_INPUT: offsets out of order, an edge id out of range, a self loop or a "
                                   "repeated edge); there is no host route with a derivative"
                                   % (bad, st_h[bad].tolist(), _lib.ST_TOO_LARGE, _lib.HKS_LARGE_NMAX, _lib.ST_NOT_CONVERGED, _lib.ST_BAD_INPUT))
        ctx.save_for_backward(dout)
        ctx.dtype, ctx.device = times.dtype, times.device
        return out

    @staticmethod
    def backward(ctx, grad):
        dout, = ctx.saved_tensors
        g = (grad.to(torch.float64) * dout).sum(dim=1)
        return g.to(device=ctx.device, dtype=ctx.dtype), None, None, None, None, None


def hks_signature(times, node_ptr, edge_ptr, edges, normalise=True, hks_sparse='host'):
    """-> float64[T, sum n]: row k is the heat-kernel signature at times[k] of every graph of the packed batch (node_ptr / edge_ptr
    int64[B + 1], edges int32[sum m, 2] local ids, CUDA tensors; simple graphs, each undirected edge once), normalised per graph by
    (max + 1e-10) unless normalise=False; differentiable in `times`, a 1-D tensor of 1 .. HKS_TMAX entries of any float dtype, on any
    device.  The forward READS THE TIMES TO THE HOST once: both kernels take them as launch arguments, and the number of squarings of
    the large tier depends on them.  Graphs up to HKS_NMAX nodes take the Jacobi tiers, larger ones up to HKS_LARGE_NMAX the large
    tier (times inside [0, HKS_LARGE_TIME_MAX] then); anything else raises RuntimeError naming graph and status -- there is no host
    fallback, because the host route has no derivative.  hks_sparse='device': the graphs above HKS_LARGE_NMAX nodes take the sparse
    tier (tlc_hks_sparse_batch_dt; no node cap, times inside [0, HKS_SPARSE_TIME_MAX]) instead of raising; 'host' (the default) raises."""
    if hks_sparse not in ("host", "device"):
        raise ValueError("hks_sparse should be one of ('host', 'device'), not %r" % (hks_sparse,))
    if not torch.is_tensor(times) or times.dim() != 1 or not times.is_floating_point() or not 1 <= times.numel() <= _lib.HKS_TMAX:
        raise ValueError("hks_signature: times should be a 1-D float tensor of 1 .. %d entries" % _lib.HKS_TMAX)
    return HksSignature.apply(times, node_ptr, edge_ptr, edges, bool(normalise), hks_sparse)


class DistanceFiltration(torch.autograd.Function):
    """The distance filtration of a packed batch as a differentiable function of the edge weights: the values of
    `engine.dist_filtration` bit for bit, the gradient of `engine.dist_filtration_vjp` (tlc_dist_filtration_vjp: along the
    shortest-path tree of each root, through the descriptor and the division by the maximum).  w may be float32 or
    float64: the filtration is computed in float64 and returned in w's dtype, and so is the gradient."""

    @staticmethod
    def forward(ctx, w, node_offs, edge_offs, edges, roots, descriptor, norm, include_roots, unreachable_100):
        w64 = w.detach().to(torch.float64).contiguous()
        f, _, parent = engine.dist_filtration(node_offs, edge_offs, edges, w64, roots, descriptor=descriptor, norm=norm,
                                              include_roots=include_roots, unreachable_100=unreachable_100)
        ctx.save_for_backward(w64, node_offs, edge_offs, edges, roots, parent)
        ctx.opts, ctx.dtype = (descriptor, norm, include_roots, unreachable_100), w.dtype
        return f.to(w.dtype)

    @staticmethod
    def backward(ctx, grad):
        w64, node_offs, edge_offs, edges, roots, parent = ctx.saved_tensors
        descriptor, norm, include_roots, unreachable_100 = ctx.opts
        gw, _ = engine.dist_filtration_vjp(node_offs, edge_offs, edges, w64, roots, parent, grad.to(torch.float64).contiguous(),
                                           descriptor=descriptor, norm=norm, include_roots=include_roots, unreachable_100=unreachable_100)
        return gw.to(ctx.dtype), None, None, None, None, None, None, None, None


def distance_filtration(w, node_offs, edge_offs, edges, roots, descriptor="sum", norm="max", include_roots=False, unreachable_100=False):
    """-> [sum n]: the distance filtration of every graph of the packed batch (node_offs / edge_offs int64[B + 1], edges int32[sum m, 2]
    local ids, each undirected edge once; roots int32[B, 2] local ids, column 1 == -1 for one root), differentiable in the edge weights
    w [sum m] (> 0) only.  A graph that is not computed raises RuntimeError naming it and its status."""
    return DistanceFiltration.apply(w, node_offs, edge_offs, edges, roots, descriptor, norm, bool(include_roots), bool(unreachable_100))


class GatherEdgeValues(torch.autograd.Function):
    """w[eid]: the value of its graph edge for every packed vicinity edge (0 where eid < 0: an edge of a refused vicinity).  Backward:
    every graph edge gets the sum of the gradients of its copies, by `engine.segment_sum` (tlc_segment_sum_f64) over the segment index
    of eid -- fp64, in an order that depends on the number of copies alone, no atomics (torch's index_add_ has neither property)."""

    @staticmethod
    def forward(ctx, w, eid, seg_ptr, seg_pos):
        ctx.save_for_backward(seg_ptr, seg_pos)
        ctx.dtype = w.dtype
        idx = eid.to(torch.int64)
        return torch.where(idx >= 0, w.detach()[idx.clamp(min=0)], torch.zeros((), dtype=w.dtype, device=w.device))

    @staticmethod
    def backward(ctx, grad):
        seg_ptr, seg_pos = ctx.saved_tensors
        g = engine.segment_sum(grad.to(torch.float64).contiguous(), seg_ptr, seg_pos)
        return g.to(ctx.dtype), None, None, None


def gather_edge_values(w, eid, seg_ptr, seg_pos):
    """-> w[eid] [len(eid)], differentiable in w [M]: eid int32 from `engine.packed_edge_lookup`, (seg_ptr, seg_pos) =
    `engine.segment_index(eid, M)`, built once per pair list."""
    if seg_ptr.numel() != w.numel() + 1 or seg_pos.numel() != eid.numel():
        raise ValueError("gather_edge_values: the segment index is not the one of these %d values and %d positions" % (w.numel(), eid.numel()))
    return GatherEdgeValues.apply(w, eid, seg_ptr, seg_pos)


def packed_points(points, slot_offs, n_points):
    """The first n_points[g] rows of every slot of `points` [sum slots, 2] (slot g starts at slot_offs[g]), packed:
    -> (pts [K, 2], offs int64[B + 1]) -- what `diagram_image` and `diagram_loss` take.  Index ops on the device, no loop over graphs;
    every row is read once, so the backward (an index_put without duplicates) is deterministic."""
    return pack_rows(points, slot_offs[:-1], n_points)


def pack_rows(points, starts, n_points):
    """`packed_points` for slots given by their first rows `starts` [S] (any order, not overlapping)."""
    cnt = n_points.to(torch.int64)
    offs = torch.zeros(cnt.numel() + 1, dtype=torch.int64, device=points.device)
    offs[1:] = torch.cumsum(cnt, 0)
    K = int(offs[-1])
    owner = torch.repeat_interleave(torch.arange(cnt.numel(), device=points.device), cnt, output_size=K)
    rows = torch.arange(K, device=points.device) - offs[:-1][owner] + starts.to(torch.int64)[owner]
    return points[rows], offs


def diagram_image(pd_hat, offs=None, res=5, imager=None, grad='weight'):
    """Images [B, Rb * Rp] of one or more diagrams, differentiable in the points.  imager=None, grad='weight': the reference's
    configuration at resolution `res` on `tlc_pi_raster` / `tlc_pi_raster_wgrad` (DiagramImage).  An imager -- a
    `Knowledge_Distillation.pimg.PersistenceImager` or an `engine.PiSpec` -- or grad='full' routes through the general entries
    (GeneralDiagramImage); with imager=None the specification is the default one at `res`, itself a valid imager."""
    if grad not in ("weight", "full"):
        raise ValueError("diagram_image: grad is %r, not 'weight' or 'full'" % (grad,))
    if offs is None:
        offs = torch.tensor([0, pd_hat.shape[0]], dtype=torch.int64, device=pd_hat.device)
    if imager is None and grad == "weight":
        return DiagramImage.apply(pd_hat, offs, int(res))
    if imager is None:
        spec = engine.PiSpec.default(int(res))
    elif isinstance(imager, engine.PiSpec):
        spec = imager
    else:
        if not imager.weight_is_ramp():
            raise ValueError("diagram_image: the imager's weight is a host callable; its images are forward only "
                             "(use imager.transform_batch on detached points)")
        spec = imager.spec(skew=True)
    return GeneralDiagramImage.apply(pd_hat, offs, spec, grad)


def diagram_landscape(pd_hat, offs=None, ts=None, K=5):
    """Persistence landscapes [B, K, T] of one or more diagrams (pd_hat [sum n, 2] float32 or float64, offs int64[B + 1] or None for
    one diagram), differentiable in the points: out[b, k, j] is the (k + 1)-th largest tent value min(t_j - birth, death - t_j) > 0
    of diagram b, +0.0 where fewer points are present.  ts: a 1-D tensor of sample values without grad (the caller's linspace);
    1 <= K <= _lib.LS_KMAX, 1 <= T <= _lib.LS_TMAX; any diagram size.  A NaN / Inf coordinate raises RuntimeError naming the diagram."""
    if not torch.is_tensor(ts) or ts.dim() != 1:
        raise ValueError("diagram_landscape: ts should be a 1-D tensor of sample values")
    if ts.requires_grad:
        raise ValueError("diagram_landscape: ts requires grad, but the samples get no gradient (detach them)")
    K = int(K)
    if not 1 <= K <= _lib.LS_KMAX:
        raise ValueError("diagram_landscape: K = %d, outside 1 .. %d" % (K, _lib.LS_KMAX))
    if not 1 <= ts.numel() <= _lib.LS_TMAX:
        raise ValueError("diagram_landscape: %d samples, outside 1 .. %d" % (ts.numel(), _lib.LS_TMAX))
    if offs is None:
        offs = torch.tensor([0, pd_hat.shape[0]], dtype=torch.int64, device=pd_hat.device)
    return DiagramLandscape.apply(pd_hat, offs, ts, K)


def diagram_gram(x, xoff=None, y=None, yoff=None, wx=None, wy=None, kernel="pss", sigma=1.0, paired=False):
    """The Gram matrix of a kernel between packed persistence diagrams (`ops.diagram_gram`), [Bx, By] or with paired=True [B], in x's
    dtype; differentiable in both point sets and both weight vectors.  y=None: X against itself (the symmetric call).  kernel 'pss' /
    'gauss' and sigma: `ops.dgm_kernel_params`; sigma is a Python number and gets no gradient.  A NaN / Inf coordinate or weight
    raises RuntimeError naming the diagram."""
    gamma, scale, mirror = ops.dgm_kernel_params(kernel, sigma)
    if y is None and (yoff is not None or wy is not None):
        raise ValueError("diagram_gram: yoff / wy without y")
    if xoff is None:
        xoff = torch.tensor([0, x.shape[0]], dtype=torch.int64, device=x.device)
    if y is not None and yoff is None:
        yoff = torch.tensor([0, y.shape[0]], dtype=torch.int64, device=y.device)
    return DiagramGram.apply(x, xoff, wx, y, yoff, wy, gamma, scale, mirror, bool(paired))


def diagram_kernel_distance(x, xoff, y, yoff, wx=None, wy=None, kernel="pss", sigma=1.0):
    """[B]: the SQUARED kernel distance k(X_i, X_i) + k(Y_i, Y_i) - 2 k(X_i, Y_i) between the diagrams of two packed batches, from three
    paired `diagram_gram` calls; differentiable like them.  Squared because the root has no gradient at 0.  Smooth everywhere, no
    assignment, no sort and no cap on the points -- the cheap sibling of `diagram_loss` and `sliced_diagram_loss`.  The three terms
    are formed and subtracted in float64 (they cancel where the diagrams agree); the result is cast to x's dtype."""
    x64, y64 = x.to(torch.float64), y.to(torch.float64)
    kxx = diagram_gram(x64, xoff, wx=wx, kernel=kernel, sigma=sigma, paired=True)
    kyy = diagram_gram(y64, yoff, wx=wy, kernel=kernel, sigma=sigma, paired=True)
    kxy = diagram_gram(x64, xoff, y64, yoff, wx=wx, wy=wy, kernel=kernel, sigma=sigma, paired=True)
    return (kxx + kyy - 2.0 * kxy).to(x.dtype)


def gat_layer(x, wl, att, wij, bias, rowptr, src, prelu_slope=-1.0):
    return GatLayer.apply(x, wl, att, wij, bias, rowptr, src, float(prelu_slope))


def gnn_layer(x, wa, ws, bias, batch, act=None, slope=0.0):
    return GnnLayer.apply(x, wa, ws, bias, batch, act, slope)


def msg_layer(x, wl, att, wij, bias, batch, mode, agg="sum_minmax", prelu_slope=-1.0):
    return MsgLayer.apply(x, wl, att, wij, bias, batch, int(mode), agg, float(prelu_slope))


def edge_head(x, w5, b5, w6, b6, src, dst, prelu_slope):
    return EdgeHead.apply(x, w5, b5, w6, b6, src, dst, float(prelu_slope))


def diagram_loss(pd_hat, target, order=2, xoff=None, yoff=None, infer=False, large="refuse"):
    """-> (loss, wxy, wxd) per problem; infer=True: (loss, wxy, wxd, wyd) of the evaluation distance.
    large: 'refuse' raises for a problem of more than 4 096 rows (predicted points; with infer, predicted + target points), 'device'
    solves those of up to 65 536 in the workspace tier (`ops.w2_large_matching`)."""
    ops.check_w2_large(large)
    dev = pd_hat.device
    if xoff is None:
        xoff = torch.tensor([0, pd_hat.shape[0]], dtype=torch.int64, device=dev)
    if yoff is None:
        yoff = torch.tensor([0, target.shape[0]], dtype=torch.int64, device=dev)
    return DiagramLoss.apply(pd_hat, xoff, target, yoff, int(order), bool(infer), large)


def sliced_diagram_loss(pd_hat, target, M=50, xoff=None, yoff=None, dirs=None, scale=None):
    """-> loss [B]: the sliced Wasserstein distance between the diagrams pd_hat and target of every problem, over the reference's M
    directions (`ops.sliced_directions`) or over dirs float64[M, 2] with `scale`.  Differentiable in pd_hat and, when it requires
    grad, in target; any diagram size.  A NaN / Inf coordinate raises ValueError."""
    dev = pd_hat.device
    if xoff is None:
        xoff = torch.tensor([0, pd_hat.shape[0]], dtype=torch.int64, device=dev)
    if yoff is None:
        yoff = torch.tensor([0, target.shape[0]], dtype=torch.int64, device=dev)
    if dirs is None:
        d_np, step = ops.sliced_directions(M)
        dirs = torch.from_numpy(d_np).to(dev)
        if scale is None:
            scale = step
    elif scale is None:
        raise ValueError("sliced_diagram_loss: dirs without a scale")
    return SlicedDiagramLoss.apply(pd_hat, xoff, target, yoff, dirs, float(scale))


def bottleneck_loss(pd_hat, target, xoff=None, yoff=None):
    """-> d_B [B]: the bottleneck distance between the diagrams pd_hat and target of every problem (both may use the diagonal; at most
    4 096 points per pair).  Differentiable in pd_hat and, when it requires grad, in target: the gradient sits on the one pair that
    attains the distance.  A pair above the cap or with a NaN / Inf coordinate raises RuntimeError."""
    dev = pd_hat.device
    if xoff is None:
        xoff = torch.tensor([0, pd_hat.shape[0]], dtype=torch.int64, device=dev)
    if yoff is None:
        yoff = torch.tensor([0, target.shape[0]], dtype=torch.int64, device=dev)
    return BottleneckLoss.apply(pd_hat, xoff, target, yoff)


class GcnLayer(torch.autograd.Function):
    """GCNConv.forward of the training path (PD_conv.py:179-188): act(A (X W) + b) with tlc_gemm_f32 / tlc_spmm_csr_f32, the
    same calls as baselines/TLCGNN.GCNConv.forward.  Backward, G = d loss / d(pre-activation):
    db = colsum(G), d(XW) = A^T G (tlc_spmm_csr_f32 on the transposed operator), dW = X^T d(XW) (tlc_gemm_tn_f32),
    dX = d(XW) W^T (tlc_gemm_f32) only when X needs it."""

    @staticmethod
    def forward(ctx, x, weight, bias, op, op_t, relu):
        rowptr, col, val = op
        xd = x.detach()
        xw = ops.gemm(xd, weight.detach())
        out = ops.spmm(rowptr, col, val, xw, bias=bias.detach(), relu=relu)
        ctx.save_for_backward(xd, weight, out if relu else None)
        ctx.op_t, ctx.relu = op_t, relu
        return out

    @staticmethod
    def backward(ctx, gout):
        x, weight, out = ctx.saved_tensors
        g = gout.contiguous()
        if ctx.relu:
            g = g.masked_fill(out <= 0, 0.0)                          # ReLU's backward (threshold on the result)
        rowptr_t, col_t, val_t = ctx.op_t
        gb = ops.colsum(g)
        gxw = ops.spmm(rowptr_t, col_t, val_t, g)
        gw = ops.gemm_tn(x, gxw)
        gx = ops.gemm(gxw, weight.detach().t().contiguous()) if ctx.needs_input_grad[0] else None
        return gx, gw, gb, None, None, None


class LpDecode(torch.autograd.Function):
    """Net.decode after the pair selection (TLCGNN.py:48-61) on the PRE-renorm embedding: emb.renorm_(2, 0, 1) (on a copy: the
    caller's tensor is left alone, autograd saw it) and the fused decode -- the same two calls as Net.decode, so the same
    probabilities.  Backward: tlc_lp_decode_bwd_f32 -> d emb (through the renorm), dW1, db1, dW, db; and, only when pi requires grad,
    tlc_lp_decode_bwd_pi_f32 -> d pi."""

    @staticmethod
    def forward(ctx, emb, pairs, pi, w1, b1, w2, b2):
        pre = emb.detach().contiguous()
        post = ops.renorm_rows_(pre.clone())
        prob = ops.lp_decode(pairs, post, pi, w1.detach(), b1.detach(), w2.detach(), b2.detach())
        ctx.save_for_backward(pre, post, pairs, pi, w1, b1, w2, b2)
        return prob

    @staticmethod
    def backward(ctx, gprob):
        pre, post, pairs, pi, w1, b1, w2, b2 = ctx.saved_tensors
        pi32 = pi if pi.dtype == torch.float32 else pi.to(torch.float32)   # (the forward's cast on load: same rounding)
        gemb, gw1, gb1, gw2, gb2 = ops.lp_decode_bwd(pairs, pre, post, pi32, w1.detach(), b1.detach(), w2.detach(), b2.detach(),
                                                     gprob.contiguous())
        if not ctx.needs_input_grad[2]:
            return gemb, None, None, gw1, gb1, gw2, gb2
        # a learned image table (topo.VicinityImages): d loss / d PI from tlc_lp_decode_bwd_pi_f32, in pi's dtype
        gpi = engine.lp_decode_bwd_pi(pairs, pre, post, pi32, w1.detach(), b1.detach(), w2.detach(), b2.detach(), gprob.contiguous())
        return gemb, None, gpi.to(pi.dtype), gw1, gb1, gw2, gb2


def gcn_layer(x, weight, bias, op, op_t, relu=False):
    return GcnLayer.apply(x, weight, bias, op, op_t, bool(relu))


def lp_decode(emb, pairs, pi, w1, b1, w2, b2):
    return LpDecode.apply(emb, pairs, pi, w1, b1, w2, b2)


class CurvConv(torch.autograd.Function):
    """curvGN.forward (Knowledge_Distillation/ConvCurv_GIN.py:159-170) without the skip branch: xl = lin(x) (tlc_nc_linear_f32), the
    edge MLP, the softmax grouped by source and the aggregation at the target (tlc_nc_curv_fwd_f32).  Backward: tlc_nc_curv_bwd_f32
    -> d xl and the edge MLP's gradients, then tlc_nc_linear_bwd_f32 -> dx, d lin.weight, d lin.bias.  w_mul gets no gradient (the
    reference computes it under no_grad from a frozen teacher)."""

    @staticmethod
    def forward(ctx, x, lin_w, lin_b, w1, prelu, w2, b2, w_mul, groups):
        xd = x.detach().contiguous()
        xl = ops.nc_linear(xd, lin_w.detach(), lin_b.detach())
        out, alpha = ops.nc_curv_fwd(groups, xl, w_mul, w1.detach(), prelu.detach(), w2.detach(), b2.detach())
        ctx.save_for_backward(xd, lin_w, xl, w_mul, w1, prelu, w2, alpha, groups)
        return out

    @staticmethod
    def backward(ctx, gout):
        xd, lin_w, xl, w_mul, w1, prelu, w2, alpha, groups = ctx.saved_tensors
        gxl, gw1, gp, gw2, gb2 = ops.nc_curv_bwd(groups, xl, w_mul, w1.detach(), prelu.detach(), w2.detach(), alpha, gout.contiguous())
        gx, gw, gb = ops.nc_linear_bwd(xd, lin_w.detach(), gxl, need_gx=ctx.needs_input_grad[0])
        return gx, gw, gb, gw1, gp, gw2, gb2, None, None


class NcLinear(torch.autograd.Function):
    """torch.nn.Linear on tlc_nc_linear_f32 / tlc_nc_linear_bwd_f32 (curvGN's lin1 of the skip branches, ConvCurv_GIN.py:161)."""

    @staticmethod
    def forward(ctx, x, w, b):
        xd = x.detach().contiguous()
        ctx.save_for_backward(xd, w)
        return ops.nc_linear(xd, w.detach(), b.detach())

    @staticmethod
    def backward(ctx, gy):
        xd, w = ctx.saved_tensors
        gx, gw, gb = ops.nc_linear_bwd(xd, w.detach(), gy.contiguous(), need_gx=ctx.needs_input_grad[0])
        return gx, gw, gb


def curv_conv(x, lin_w, lin_b, w1, prelu, w2, b2, w_mul, groups):
    return CurvConv.apply(x, lin_w, lin_b, w1, prelu, w2, b2, w_mul, groups)


def nc_linear(x, w, b):
    return NcLinear.apply(x, w, b)

"""Device-side entry points of the PD/PI path: thin, typed wrappers over the C ABI (include/tlcgnn.h).

Everything here takes/returns torch CUDA tensors (device memory + stream plumbing only) and calls
libtlcgnn_hip.so through ctypes.  The reference-named drop-ins (sg2dgm/, baselines/, Knowledge_Distillation/)
are built on these.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import KEEP_ZERO_PERS, INCLUDE_ROOTS, NORM_EPS, PI_ORD0_EXT1, NO_EXT1, UNREACHABLE_100  # noqa: F401


class DeviceGraph:
    """graph2pi.__init__ (sg2dgm/riccidist2dgm.py:216-226): weighted graph resident on one GPU.

    rowptr/col/w: symmetric CSR (numpy), w = kappa + 1 > 0.
    """

    def __init__(self, rowptr, col, w, device=None):
        torch = _lib.require_gpu()
        self.device = torch.cuda.current_device() if device is None else int(device)
        rowptr = np.ascontiguousarray(rowptr, dtype=np.int32)
        col = np.ascontiguousarray(col, dtype=np.int32)
        w = np.ascontiguousarray(w, dtype=np.float64)
        self.n_nodes = len(rowptr) - 1
        self.nnz = int(rowptr[-1])
        h = C.c_void_p()
        rc = _lib.lib().tlc_graph_create(C.c_int32(self.n_nodes), rowptr.ctypes.data_as(C.c_void_p),
                                         col.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p),
                                         C.c_int(self.device), C.byref(h))
        _lib.check(rc, "tlc_graph_create")
        self._h = h
        self._inflight = []

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().tlc_graph_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- P2-P9 -------------------------------------------------------------------------------------------
    def pd_pi_batch(self, pairs, hop, flags=0, res=5, out=None, status=None, async_=False):
        """pairs: int32 CUDA tensor [E,2] -> (pi float64[E,res*res], status uint8[E]) on the current stream.
        async_: submit without making the current stream wait (tlc_pd_pi_batch_async): batches submitted back to back overlap;
        the outputs are complete for work that follows join() on its stream."""
        import torch
        assert pairs.is_cuda and pairs.dtype == torch.int32 and pairs.dim() == 2 and pairs.shape[1] == 2
        assert pairs.device.index == self.device, "pairs live on cuda:%s, the graph on cuda:%d" % (pairs.device.index, self.device)
        pairs = pairs.contiguous()
        E = pairs.shape[0]
        if out is None:
            out = torch.empty((E, res * res), dtype=torch.float64, device=pairs.device)
        if status is None:
            status = torch.empty((E,), dtype=torch.uint8, device=pairs.device)
        fn = _lib.lib().tlc_pd_pi_batch_async if async_ else _lib.lib().tlc_pd_pi_batch
        rc = fn(self._h, _lib.ptr(pairs), C.c_int64(E), C.c_int(hop), C.c_uint32(flags),
                C.c_int(res), _lib.ptr(out), _lib.ptr(status), _lib.stream_ptr(self.device))
        _lib.check(rc, "tlc_pd_pi_batch")
        if async_:
            self._inflight.append((pairs, out, status))          # (the buffers of a batch in flight must stay alive)
            del self._inflight[:-6]
        return out, status

    def join(self):
        """The current stream waits for every batch submitted with async_=True (nothing is waited for on the host)."""
        _lib.check(_lib.lib().tlc_pd_pi_batch_join(self._h, _lib.stream_ptr(self.device)), "tlc_pd_pi_batch_join")

    def stats(self):
        out = (C.c_int64 * 10)()
        rc = _lib.lib().tlc_pd_pi_batch_stats(self._h, C.cast(out, C.c_void_p), _lib.stream_ptr(self.device))
        _lib.check(rc, "tlc_pd_pi_batch_stats")
        v = list(out)
        return {"tier_small": v[0], "tier_medium": v[1], "tier_large": v[2], "tier_huge": v[3],
                "tier_mid": v[7], "tier_tiny": v[8], "tier_medium_many_pos": v[9],
                "induced_entries": v[4], "tie_fallback_sources": v[5], "chunks": v[6]}

    # ---- diagnostics (tests, A/B timing) --------------------------------------------------------------------------
    def set_option(self, name, value):
        """'extract' (ball-list extraction) / 'heavy' (its hub-row skipping) / 'tiny' (lane-per-subgraph kernel):
        1 on (default), 0 off.  Results do not depend on them (tests/test_gpu_extract.py)."""
        _lib.check(_lib.lib().tlc_debug_set_option(self._h, name.encode(), C.c_int(int(value))), "tlc_debug_set_option")

    def dc_stats(self):
        """(subgraphs whose cycle swap ran as the divide and conquer, subgraphs it gave back to the serial walk) since the last
        pd_pi_batch call began."""
        out = (C.c_longlong * 2)()
        _lib.check(_lib.lib().tlc_debug_dc_stats(self._h, C.cast(out, C.c_void_p), _lib.stream_ptr(self.device)), "tlc_debug_dc_stats")
        return int(out[0]), int(out[1])

    def tier_counts(self):
        """The tier lists of the last pd_pi_batch call as the device cut them (tlc_debug_tier_counts)."""
        out = (C.c_longlong * 8)()
        _lib.check(_lib.lib().tlc_debug_tier_counts(self._h, C.cast(out, C.c_void_p), _lib.stream_ptr(self.device)), "tlc_debug_tier_counts")
        return dict(zip(("small", "medium", "large", "huge", "mid", "tiny", "medium_many_pos", "medium_wide"), (int(v) for v in out)))

    CHUNK_COUNTERS = ("front_list_last_call", "front_list", "pipelined_chunks", "early_chunks", "beyond_spec_slots", "poisoned_chunks",
                      "poison_bytes", "poison_arena_bytes", "poison_early_bytes", "poison_small_bytes", "deferred_second_halves",
                      "max_busy_workspaces")

    def chunk_counters(self):
        """Scheduling counters of the handle (tlc_debug_chunk_counters): the front-list vicinities of the last pd_pi_batch call
        ('front_list_last_call'), then totals since the handle was created, and the bytes of each region the last poisoned chunk filled
        (option 'poison'); 'deferred_second_halves' / 'max_busy_workspaces' show how far chunks overlapped (a hop change drains
        every workspace)."""
        out = (C.c_longlong * len(self.CHUNK_COUNTERS))()
        _lib.check(_lib.lib().tlc_debug_chunk_counters(self._h, C.cast(out, C.c_void_p), C.c_int32(len(out)), _lib.stream_ptr(self.device)),
                   "tlc_debug_chunk_counters")
        return dict(zip(self.CHUNK_COUNTERS, (int(v) for v in out)))

    def front_list_count(self):
        """MEDIUM vicinities the last pd_pi_batch call's pipelined chunks put in front of their list (option mh_front_pos)."""
        return self.chunk_counters()["front_list_last_call"]

    # ---- measurement helpers (bench.py) -----------------------------------------------------------------------
    KERNELS = ["vicinity_count", "scan_bin", "vicinity_fill", "pd_tier_small", "pd_tier_medium", "pd_tier_large", "pd_tier_huge",
               "pd_tier_mid"]

    def set_timing(self, on=True, only=None):
        """on: bracket every kernel of later batches with HIP events; only=[names of KERNELS]: just those (the event records
        cost time themselves: 48 us of the 1.06 ms PubMed batch for all eight)."""
        mask = (1 if on else 0) if only is None else sum(1 << (self.KERNELS.index(k) + 1) for k in only)
        _lib.check(_lib.lib().tlc_pd_pi_batch_set_timing(self._h, C.c_int(mask)), "set_timing")

    def timings(self):
        """ms per kernel of the last batch (HIP events on the stream each kernel ran on); -1 = not launched."""
        out = (C.c_double * 8)()
        _lib.check(_lib.lib().tlc_pd_pi_batch_timings(self._h, C.cast(out, C.c_void_p), _lib.stream_ptr(self.device)), "timings")
        return dict(zip(self.KERNELS, list(out)[:8]))

    def timing_history(self, kernel, cap=64):
        """ms of `kernel` (a name of KERNELS) over the most recent chunks, oldest first -- read once after a run of batches
        that were enqueued without synchronising (the library keeps the events of the last 64 chunks)."""
        out = (C.c_double * cap)()
        n = C.c_int32(0)
        _lib.check(_lib.lib().tlc_pd_pi_batch_timing_history(self._h, C.c_int(self.KERNELS.index(kernel)), C.cast(out, C.c_void_p),
                                                             C.c_int32(cap), C.byref(n), _lib.stream_ptr(self.device)), "timing_history")
        return list(out)[:n.value]

    def sizes(self, n_pairs):
        n = np.zeros(n_pairs, dtype=np.int32)
        m2 = np.zeros(n_pairs, dtype=np.int32)
        _lib.check(_lib.lib().tlc_pd_pi_batch_sizes(self._h, n.ctypes.data_as(C.c_void_p), m2.ctypes.data_as(C.c_void_p),
                                                    C.c_int64(n_pairs), _lib.stream_ptr(self.device)), "sizes")
        return n, m2

    def _capacity_offsets(self, E, cap, dev):
        """arange(E + 1) * cap, kept for the last few (E, cap): a loop over equally sized chunks asks for the same two tensors every time
        (read-only: callers get the cached tensor itself)."""
        cache = self.__dict__.setdefault("_cap_offs", {})
        key = (E, cap, str(dev))
        t = cache.get(key)
        if t is None:
            import torch
            if len(cache) >= 8:
                cache.clear()
            t = cache[key] = torch.arange(E + 1, dtype=torch.int64, device=dev) * cap
        return t

    def vicinity_sizes(self, pairs, hop, flags=0):
        """-> (n int32[E], m int32[E]) CUDA tensors: |S| and the induced edge count of every pair's vicinity (tlc_vicinity_sizes)."""
        import torch
        assert pairs.device.index == self.device, "pairs live on cuda:%s, the graph on cuda:%d" % (pairs.device.index, self.device)
        pairs = pairs.contiguous()
        E = pairs.shape[0]
        n = torch.zeros(max(E, 1), dtype=torch.int32, device=pairs.device)
        m = torch.zeros(max(E, 1), dtype=torch.int32, device=pairs.device)
        rc = _lib.lib().tlc_vicinity_sizes(self._h, _lib.ptr(pairs), C.c_int64(E), C.c_int(hop), C.c_uint32(flags), _lib.ptr(n), _lib.ptr(m),
                                           _lib.stream_ptr(self.device))
        _lib.check(rc, "tlc_vicinity_sizes")
        return n[:E], m[:E]

    def vicinity_filtration(self, pairs, hop, flags=0, cap=None, edge_cap=None, zero=True, offsets=None):
        """-> (node_offs int64[E+1], ids int32[E*cap], f float64[E*cap], n int32[E], status uint8[E])
        with edge_cap: additionally (edge_offs int64[E+1], edges int32[E*edge_cap,2] local ids, m int32[E]).
        zero=False: the capacity buffers are not zero-filled (what lies beyond a pair's n / m entries is never read by a caller
        that slices by n / m: 290 MB of fill per 4 096 pairs at node_cap 512 / edge_cap 8 192).
        offsets=(node_offs, edge_offs, total_nodes, total_edges): the caller's own offsets (e.g. exact ones from vicinity_sizes +
        pack_offsets) instead of a capacity per pair; the outputs then have total_nodes / total_edges rows."""
        import torch
        assert pairs.device.index == self.device, "pairs live on cuda:%s, the graph on cuda:%d" % (pairs.device.index, self.device)
        pairs = pairs.contiguous()
        E = pairs.shape[0]
        dev = pairs.device
        mk = torch.zeros if zero else torch.empty
        if offsets is not None:
            offs, eoffs_x, tot_n, tot_m = offsets
            ids = mk(max(int(tot_n), 1), dtype=torch.int32, device=dev)
            f = mk(max(int(tot_n), 1), dtype=torch.float64, device=dev)
            n = torch.zeros(max(E, 1), dtype=torch.int32, device=dev)
            st = torch.zeros(max(E, 1), dtype=torch.uint8, device=dev)
            edges = mk((max(int(tot_m), 1), 2), dtype=torch.int32, device=dev)
            m = torch.zeros(max(E, 1), dtype=torch.int32, device=dev)
            rc = _lib.lib().tlc_vicinity_filtration(self._h, _lib.ptr(pairs), C.c_int64(E), C.c_int(hop), C.c_uint32(flags),
                                                    _lib.ptr(offs), _lib.ptr(ids), _lib.ptr(f), _lib.ptr(n), _lib.ptr(st),
                                                    _lib.ptr(eoffs_x), _lib.ptr(edges), _lib.ptr(m), _lib.stream_ptr(self.device))
            _lib.check(rc, "tlc_vicinity_filtration")
            return offs, ids, f, n[:E], st[:E], eoffs_x, edges, m[:E]
        cap = self.n_nodes if cap is None else int(cap)
        offs = self._capacity_offsets(E, cap, dev)
        ids = mk(max(E * cap, 1), dtype=torch.int32, device=dev)
        f = mk(max(E * cap, 1), dtype=torch.float64, device=dev)
        n = torch.zeros(max(E, 1), dtype=torch.int32, device=dev)
        st = torch.zeros(max(E, 1), dtype=torch.uint8, device=dev)
        eoffs = edges = m = None
        if edge_cap is not None:
            eoffs = self._capacity_offsets(E, int(edge_cap), dev)
            edges = mk((max(E * int(edge_cap), 1), 2), dtype=torch.int32, device=dev)
            m = torch.zeros(max(E, 1), dtype=torch.int32, device=dev)
        rc = _lib.lib().tlc_vicinity_filtration(self._h, _lib.ptr(pairs), C.c_int64(E), C.c_int(hop), C.c_uint32(flags),
                                                _lib.ptr(offs), _lib.ptr(ids), _lib.ptr(f), _lib.ptr(n), _lib.ptr(st),
                                                _lib.ptr(eoffs), _lib.ptr(edges), _lib.ptr(m), _lib.stream_ptr(self.device))
        _lib.check(rc, "tlc_vicinity_filtration")
        if edge_cap is not None:
            return offs, ids, f, n[:E], st[:E], eoffs, edges, m[:E]
        return offs, ids, f, n[:E], st[:E]


@_lib.on_device_of
def pack_vicinities(node_offs, ids, f, edge_offs, edges, node_ptr, edge_ptr, tot_n, tot_m, label=None, owners=True):
    """The capacity layout of vicinity_filtration -> packed (ids int64 [tot_n], f [tot_n], edges int32 [tot_m, 2], pair_of_node,
    pair_of_edge) at node_ptr / edge_ptr (tlc_pack_vicinities: one kernel, no host synchronisation)."""
    torch = _lib.require_gpu()
    dev = f.device
    E = node_ptr.numel() - 1
    out_ids = torch.empty(max(tot_n, 1), dtype=torch.int64, device=dev)
    out_f = torch.empty(max(tot_n, 1), dtype=torch.float64, device=dev)
    out_e = torch.empty((max(tot_m, 1), 2), dtype=torch.int32, device=dev)
    pn = torch.empty(max(tot_n, 1), dtype=torch.int64, device=dev) if owners else None
    pe = torch.empty(max(tot_m, 1), dtype=torch.int64, device=dev) if owners else None
    rc = _lib.lib().tlc_pack_vicinities(C.c_int64(E), _lib.ptr(node_offs), _lib.ptr(ids), _lib.ptr(f), _lib.ptr(edge_offs),
                                        _lib.ptr(edges), _lib.ptr(node_ptr), _lib.ptr(edge_ptr), _lib.ptr(label), _lib.ptr(out_ids),
                                        _lib.ptr(out_f), _lib.ptr(out_e), _lib.ptr(pn), _lib.ptr(pe), _lib.stream_ptr())
    _lib.check(rc, "tlc_pack_vicinities")
    return out_ids[:tot_n], out_f[:tot_n], out_e[:tot_m], (pn[:tot_n] if owners else None), (pe[:tot_m] if owners else None)


@_lib.on_device_of
def stack_batch(node_ptr, edge_ptr, edges, f=None):
    """A packed batch (node_ptr / edge_ptr int64[B+1], edges int32 [m,2] local ids, f float64 [n]) -> (edge_index int64 [2, m+n] with
    global ids and the n self loops last, x float32 [n,1] or None): the operands of Teacher_Model.forward, one launch
    (tlc_stack_batch); the sizes are the tensors' own, nothing is read back."""
    torch = _lib.require_gpu()
    B, m = node_ptr.numel() - 1, int(edges.shape[0])
    if f is None:
        raise ValueError("stack_batch: f (its length is the node count) is needed")
    n = int(f.numel())
    ei = torch.empty((2, m + n), dtype=torch.int64, device=edges.device)
    x = torch.empty((n, 1), dtype=torch.float32, device=edges.device)
    rc = _lib.lib().tlc_stack_batch(C.c_int64(B), _lib.ptr(node_ptr), _lib.ptr(edge_ptr), _lib.ptr(edges.contiguous()),
                                    _lib.ptr(f.contiguous()), C.c_int64(n), C.c_int64(m), _lib.ptr(ei), _lib.ptr(x), _lib.stream_ptr())
    _lib.check(rc, "tlc_stack_batch")
    return ei, x


@_lib.on_device_of
def pack_offsets(n, m):
    """Per-pair counts of vicinity_filtration (int32[E], negative = did not fit) -> (node_ptr int64[E+1], edge_ptr int64[E+1],
    totals int64[4] = min n, min m, sum n, sum m): tlc_pack_offsets, one launch; vicinities without an edge are left out."""
    torch = _lib.require_gpu()
    E = n.numel()
    dev = n.device
    node_ptr = torch.empty(E + 1, dtype=torch.int64, device=dev)
    edge_ptr = torch.empty(E + 1, dtype=torch.int64, device=dev)
    totals = torch.empty(4, dtype=torch.int64, device=dev)
    rc = _lib.lib().tlc_pack_offsets(C.c_int64(E), _lib.ptr(n.contiguous()), _lib.ptr(m.contiguous()), _lib.ptr(node_ptr), _lib.ptr(edge_ptr),
                                     _lib.ptr(totals), _lib.stream_ptr())
    _lib.check(rc, "tlc_pack_offsets")
    return node_ptr, edge_ptr, totals


@_lib.on_device_of
def hks_batch(node_ptr, edge_ptr, edges, times, normalise=True, total_nodes=None, dt=False):
    """Heat-kernel signatures of a packed batch of simple graphs on the device (tlc_hks_batch; `hks_signature` of the reference's
    data_utils_LP/NC/GC, one Jacobi eigen-decomposition per graph shared by all `times`).

    node_ptr / edge_ptr int64[B+1], edges int32[sum m, 2] local ids: CUDA tensors, the layout of `Vicinities.batch`.  times: a
    float or up to 8 floats.  normalise: each graph's values / (max + 1e-10).  Returns (f float64[T, sum n], status uint8[B]); a
    graph whose status is not ST_OK (ST_TOO_LARGE: more than HKS_NMAX nodes; ST_NOT_CONVERGED; ST_BAD_INPUT: offsets out of order or
    beyond the totals, an id outside 0 .. n-1, a self loop, or an unordered pair listed twice, in the same or in both directions --
    each undirected edge once is the contract, a multigraph is refused and never computed differently from the host route) has NaN in
    its slice.
    total_nodes: sum n if the caller has it already (`Vicinities.batch` does); else node_ptr[-1] is read, the call's only host read.
    dt=True: tlc_hks_batch_dt, returns (f, df, status) with df float64[T, sum n] = d f / d t of exactly what f holds (normalised when f
    is: the quotient rule at the lowest index of the maximum); f and status are the same bits, df is NaN where f is."""
    torch = _lib.require_gpu()
    dev = node_ptr.device
    times = [float(t) for t in (times if hasattr(times, "__len__") else [times])]
    T, B = len(times), node_ptr.numel() - 1
    if not 1 <= T <= _lib.HKS_TMAX:
        raise ValueError("hks_batch: 1 .. %d times per call" % _lib.HKS_TMAX)
    tot_m = int(edges.shape[0])
    tot_n = int(total_nodes) if total_nodes is not None else (int(node_ptr[-1]) if B > 0 else 0)
    out = torch.full((T, tot_n), float("nan"), dtype=torch.float64, device=dev)
    status = torch.zeros(max(B, 1), dtype=torch.uint8, device=dev)
    if B > 0:
        need = C.c_int64(0)
        _lib.check(_lib.lib().tlc_hks_batch_work_bytes(C.c_int64(B), C.c_int64(tot_n), C.c_int64(tot_m), C.c_int32(T), C.byref(need)),
                   "tlc_hks_batch_work_bytes")
        work = torch.empty(need.value, dtype=torch.uint8, device=dev)
        if dt:
            dout = torch.full((T, tot_n), float("nan"), dtype=torch.float64, device=dev)
            rc = _lib.lib().tlc_hks_batch_dt(_lib.ptr(node_ptr.contiguous()), _lib.ptr(edge_ptr.contiguous()), _lib.ptr(edges.contiguous()),
                                             C.c_int64(B), C.c_int64(tot_n), C.c_int64(tot_m), (C.c_double * T)(*times), C.c_int32(T),
                                             C.c_uint32(_lib.HKS_NORMALISE if normalise else 0), _lib.ptr(out), _lib.ptr(dout), _lib.ptr(status),
                                             _lib.ptr(work), C.c_int64(need.value), _lib.stream_ptr())
            _lib.check(rc, "tlc_hks_batch_dt")
            return out, dout, status[:B]
        rc = _lib.lib().tlc_hks_batch(_lib.ptr(node_ptr.contiguous()), _lib.ptr(edge_ptr.contiguous()), _lib.ptr(edges.contiguous()),
                                      C.c_int64(B), C.c_int64(tot_n), C.c_int64(tot_m), (C.c_double * T)(*times), C.c_int32(T),
                                      C.c_uint32(_lib.HKS_NORMALISE if normalise else 0), _lib.ptr(out), _lib.ptr(status), _lib.ptr(work),
                                      C.c_int64(need.value), _lib.stream_ptr())
        _lib.check(rc, "tlc_hks_batch")
    if dt:
        return out, torch.full((T, tot_n), float("nan"), dtype=torch.float64, device=dev), status[:B]
    return out, status[:B]


HKS_LARGE_WORK_CAP = 2 << 30      # hks_large_batch(work_bytes=None): the workspace it allocates at most (never below min_bytes)


def hks_large_work_bytes(sel_nodes, n_times=1):
    """(min_bytes, all_bytes) of tlc_hks_large_work_bytes for the node counts of a selection: host arithmetic, no device needed."""
    nodes = [int(v) for v in sel_nodes]
    lo, hi = C.c_int64(0), C.c_int64(0)
    arr = (C.c_int64 * max(len(nodes), 1))(*nodes)
    _lib.check(_lib.lib().tlc_hks_large_work_bytes(arr, C.c_int64(len(nodes)), C.c_int32(n_times), C.byref(lo), C.byref(hi)),
               "tlc_hks_large_work_bytes")
    return lo.value, hi.value


@_lib.on_device_of
def hks_large_batch(node_ptr, edge_ptr, edges, sel, sel_nodes, times, normalise=True, total_nodes=None, out=None, status=None, work_bytes=None,
                    dout=None):
    """Heat-kernel signatures of SELECTED graphs of a packed batch on the device without eigenpairs (tlc_hks_large_batch: exp(-tL) by
    scaling, a degree-14 Taylor series and squarings, fp64 products on the matrix cores) -- the tier for graphs above HKS_NMAX nodes,
    up to HKS_LARGE_NMAX; times inside [0, HKS_LARGE_TIME_MAX].

    node_ptr / edge_ptr / edges, times, normalise, total_nodes: as `hks_batch`.  sel: the indices of the graphs to compute, strictly
    ascending; sel_nodes: their node counts (HOST sequences: the library sizes its workspace from them without a read-back; a count
    that is not the device's is ST_BAD_INPUT, one above HKS_LARGE_NMAX ST_TOO_LARGE).  out float64[T, sum n] / status uint8[B]: written
    for the selected graphs only (given: e.g. what `hks_batch` returned; not given: NaN-filled / zero-filled).  work_bytes: the
    workspace to allocate, at least min_bytes of `hks_large_work_bytes` (the selection then runs in groups that fit, same bits);
    None: all_bytes, bounded by HKS_LARGE_WORK_CAP.  Returns (out, status).
    dout: True or a contiguous float64[T, sum n] (e.g. the df of `hks_batch(dt=True)`): tlc_hks_large_batch_dt writes the selected graphs'
    d out / d t into it, out and status the same bits; returns (out, dout, status)."""
    torch = _lib.require_gpu()
    dev = node_ptr.device
    times = [float(t) for t in (times if hasattr(times, "__len__") else [times])]
    T, B = len(times), node_ptr.numel() - 1
    if not 1 <= T <= _lib.HKS_TMAX:
        raise ValueError("hks_large_batch: 1 .. %d times per call" % _lib.HKS_TMAX)
    sel, sel_nodes = [int(v) for v in sel], [int(v) for v in sel_nodes]
    if len(sel) != len(sel_nodes):
        raise ValueError("hks_large_batch: sel and sel_nodes differ in length")
    tot_m = int(edges.shape[0])
    tot_n = int(total_nodes) if total_nodes is not None else (int(node_ptr[-1]) if B > 0 else 0)
    if out is None:
        out = torch.full((T, tot_n), float("nan"), dtype=torch.float64, device=dev)
    if status is None:
        status = torch.zeros(max(B, 1), dtype=torch.uint8, device=dev)[:B]
    if tuple(out.shape) != (T, tot_n) or out.dtype != torch.float64 or not out.is_contiguous() or status.numel() != B or status.dtype != torch.uint8 \
            or not status.is_contiguous():
        raise ValueError("hks_large_batch: out should be contiguous float64[%d, %d] and status contiguous uint8[%d]" % (T, tot_n, B))
    want_dt = dout is not None and dout is not False
    if want_dt:
        if dout is True:
            dout = torch.full((T, tot_n), float("nan"), dtype=torch.float64, device=dev)
        if tuple(dout.shape) != (T, tot_n) or dout.dtype != torch.float64 or not dout.is_contiguous():
            raise ValueError("hks_large_batch: dout should be contiguous float64[%d, %d]" % (T, tot_n))
    S = len(sel)
    if S > 0:
        lo, hi = hks_large_work_bytes(sel_nodes, T)
        need = max(lo, min(hi, HKS_LARGE_WORK_CAP)) if work_bytes is None else int(work_bytes)
        work = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
        if want_dt:
            rc = _lib.lib().tlc_hks_large_batch_dt(_lib.ptr(node_ptr.contiguous()), _lib.ptr(edge_ptr.contiguous()), _lib.ptr(edges.contiguous()),
                                                   C.c_int64(B), C.c_int64(tot_n), C.c_int64(tot_m), (C.c_int64 * S)(*sel), (C.c_int64 * S)(*sel_nodes),
                                                   C.c_int64(S), (C.c_double * T)(*times), C.c_int32(T),
                                                   C.c_uint32(_lib.HKS_NORMALISE if normalise else 0), _lib.ptr(out), _lib.ptr(dout), _lib.ptr(status),
                                                   _lib.ptr(work), C.c_int64(need), _lib.stream_ptr())
            _lib.check(rc, "tlc_hks_large_batch_dt")
            return out, dout, status
        rc = _lib.lib().tlc_hks_large_batch(_lib.ptr(node_ptr.contiguous()), _lib.ptr(edge_ptr.contiguous()), _lib.ptr(edges.contiguous()),
                                            C.c_int64(B), C.c_int64(tot_n), C.c_int64(tot_m), (C.c_int64 * S)(*sel), (C.c_int64 * S)(*sel_nodes),
                                            C.c_int64(S), (C.c_double * T)(*times), C.c_int32(T),
                                            C.c_uint32(_lib.HKS_NORMALISE if normalise else 0), _lib.ptr(out), _lib.ptr(status), _lib.ptr(work),
                                            C.c_int64(need), _lib.stream_ptr())
        _lib.check(rc, "tlc_hks_large_batch")
    if want_dt:
        return out, dout, status
    return out, status


HKS_SPARSE_WORK_CAP = 2 << 30     # hks_sparse_batch(work_bytes=None): the workspace it allocates at most (never below min_bytes)


def hks_sparse_work_bytes(sel_nodes, sel_edges, n_times=1):
    """(min_bytes, all_bytes) of tlc_hks_sparse_work_bytes for the node and edge counts of a selection: host arithmetic, no device needed."""
    nodes, edges = [int(v) for v in sel_nodes], [int(v) for v in sel_edges]
    if len(nodes) != len(edges):
        raise ValueError("hks_sparse_work_bytes: sel_nodes and sel_edges differ in length")
    lo, hi = C.c_int64(0), C.c_int64(0)
    _lib.check(_lib.lib().tlc_hks_sparse_work_bytes((C.c_int64 * max(len(nodes), 1))(*nodes), (C.c_int64 * max(len(edges), 1))(*edges),
                                                    C.c_int64(len(nodes)), C.c_int32(n_times), C.byref(lo), C.byref(hi)),
               "tlc_hks_sparse_work_bytes")
    return lo.value, hi.value


@_lib.on_device_of
def hks_sparse_batch(node_ptr, edge_ptr, edges, sel, sel_nodes, sel_edges, times, normalise=True, total_nodes=None, out=None, status=None,
                     work_bytes=None, dout=None):
    """Heat-kernel signatures of SELECTED graphs of a packed batch on the device without eigenpairs and without a dense matrix
    (tlc_hks_sparse_batch: the columns of exp(-t/2 L) by a Taylor chain of sparse products, 64 columns per wavefront) -- the tier for
    sparse graphs of any size; times inside [0, HKS_SPARSE_TIME_MAX].

    The arguments of `hks_large_batch`, and sel_edges: the selected graphs' edge counts (a HOST sequence like sel_nodes; a count that
    is not the device's is ST_BAD_INPUT).  work_bytes: at least min_bytes of `hks_sparse_work_bytes` (the panels then run in groups
    that fit, same bits); None: all_bytes, bounded by HKS_SPARSE_WORK_CAP.  Returns (out, status), with dout (out, dout, status)."""
    torch = _lib.require_gpu()
    dev = node_ptr.device
    times = [float(t) for t in (times if hasattr(times, "__len__") else [times])]
    T, B = len(times), node_ptr.numel() - 1
    if not 1 <= T <= _lib.HKS_TMAX:
        raise ValueError("hks_sparse_batch: 1 .. %d times per call" % _lib.HKS_TMAX)
    sel, sel_nodes, sel_edges = [int(v) for v in sel], [int(v) for v in sel_nodes], [int(v) for v in sel_edges]
    if len(sel) != len(sel_nodes) or len(sel) != len(sel_edges):
        raise ValueError("hks_sparse_batch: sel, sel_nodes and sel_edges differ in length")
    tot_m = int(edges.shape[0])
    tot_n = int(total_nodes) if total_nodes is not None else (int(node_ptr[-1]) if B > 0 else 0)
    if out is None:
        out = torch.full((T, tot_n), float("nan"), dtype=torch.float64, device=dev)
    if status is None:
        status = torch.zeros(max(B, 1), dtype=torch.uint8, device=dev)[:B]
    if tuple(out.shape) != (T, tot_n) or out.dtype != torch.float64 or not out.is_contiguous() or status.numel() != B or status.dtype != torch.uint8 \
            or not status.is_contiguous():
        raise ValueError("hks_sparse_batch: out should be contiguous float64[%d, %d] and status contiguous uint8[%d]" % (T, tot_n, B))
    want_dt = dout is not None and dout is not False
    if want_dt:
        if dout is True:
            dout = torch.full((T, tot_n), float("nan"), dtype=torch.float64, device=dev)
        if tuple(dout.shape) != (T, tot_n) or dout.dtype != torch.float64 or not dout.is_contiguous():
            raise ValueError("hks_sparse_batch: dout should be contiguous float64[%d, %d]" % (T, tot_n))
    S = len(sel)
    if S > 0:
        lo, hi = hks_sparse_work_bytes(sel_nodes, sel_edges, T)
        need = max(lo, min(hi, HKS_SPARSE_WORK_CAP)) if work_bytes is None else int(work_bytes)
        work = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
        head = (_lib.ptr(node_ptr.contiguous()), _lib.ptr(edge_ptr.contiguous()), _lib.ptr(edges.contiguous()), C.c_int64(B), C.c_int64(tot_n),
                C.c_int64(tot_m), (C.c_int64 * S)(*sel), (C.c_int64 * S)(*sel_nodes), (C.c_int64 * S)(*sel_edges), C.c_int64(S),
                (C.c_double * T)(*times), C.c_int32(T), C.c_uint32(_lib.HKS_NORMALISE if normalise else 0), _lib.ptr(out))
        tail = (_lib.ptr(status), _lib.ptr(work), C.c_int64(need), _lib.stream_ptr())
        if want_dt:
            _lib.check(_lib.lib().tlc_hks_sparse_batch_dt(*head, _lib.ptr(dout), *tail), "tlc_hks_sparse_batch_dt")
        else:
            _lib.check(_lib.lib().tlc_hks_sparse_batch(*head, *tail), "tlc_hks_sparse_batch")
    if want_dt:
        return out, dout, status
    return out, status


def struct_kinds(kinds):
    """A name or a sequence of names of _lib.STRUCT_KINDS -> (bit mask, the names in output-row order: degree, centrality, clustering)."""
    names = [kinds] if isinstance(kinds, str) else list(kinds)
    if not names or any(k not in _lib.STRUCT_KINDS for k in names) or len(set(names)) != len(names):
        raise ValueError("struct_batch: kinds should be one or more of %s, each once, not %r" % (tuple(_lib.STRUCT_KINDS), kinds))
    return sum(_lib.STRUCT_KINDS[k] for k in names), [k for k in _lib.STRUCT_KINDS if k in names]


@_lib.on_device_of
def struct_batch(node_ptr, edge_ptr, edges, kinds, normalise=True, total_nodes=None):
    """The degree / centrality / clustering node functions of a packed batch of simple graphs on the device (tlc_struct_batch; the
    values of `data_utils_LP.structural_filtration`, bit for bit).

    node_ptr / edge_ptr int64[B+1], edges int32[sum m, 2] local ids: CUDA tensors, the layout of `Vicinities.batch`.  kinds: a name or
    a sequence of names out of 'degree', 'centrality', 'clustering'.  normalise: each graph's values / (max + 1e-10).  Returns
    (f float64[K, sum n], status uint8[B]): the rows of f in the order degree, centrality, clustering of the kinds asked for (whatever
    order they were named in); a graph whose status is ST_BAD_INPUT (offsets out of order or beyond the totals, an id outside
    0 .. n-1, a self loop, an unordered pair listed twice in either orientation) has NaN in its slice.  No size cap, no host fallback.
    total_nodes: sum n if the caller has it already (`Vicinities.batch` does); else node_ptr[-1] is read, the call's only host read."""
    torch = _lib.require_gpu()
    dev = node_ptr.device
    mask, names = struct_kinds(kinds)
    K, B = len(names), node_ptr.numel() - 1
    tot_m = int(edges.shape[0])
    tot_n = int(total_nodes) if total_nodes is not None else (int(node_ptr[-1]) if B > 0 else 0)
    out = torch.full((K, tot_n), float("nan"), dtype=torch.float64, device=dev)
    status = torch.zeros(max(B, 1), dtype=torch.uint8, device=dev)
    if B > 0:
        need = C.c_int64(0)
        _lib.check(_lib.lib().tlc_struct_batch_work_bytes(C.c_int64(B), C.c_int64(tot_n), C.c_int64(tot_m), C.c_uint32(mask), C.byref(need)),
                   "tlc_struct_batch_work_bytes")
        work = torch.empty(need.value, dtype=torch.uint8, device=dev)
        rc = _lib.lib().tlc_struct_batch(_lib.ptr(node_ptr.contiguous()), _lib.ptr(edge_ptr.contiguous()), _lib.ptr(edges.contiguous()),
                                         C.c_int64(B), C.c_int64(tot_n), C.c_int64(tot_m), C.c_uint32(mask),
                                         C.c_uint32(_lib.STRUCT_NORMALISE if normalise else 0), _lib.ptr(out), _lib.ptr(status), _lib.ptr(work),
                                         C.c_int64(need.value), _lib.stream_ptr())
        _lib.check(rc, "tlc_struct_batch")
    return out, status[:B]


def graph_components_work_bytes(n_graphs, total_nodes, total_edges):
    """Bytes of workspace tlc_graph_components needs for a batch of these totals: host arithmetic, no device."""
    need = C.c_int64(0)
    _lib.check(_lib.lib().tlc_graph_components_work_bytes(C.c_int64(int(n_graphs)), C.c_int64(int(total_nodes)), C.c_int64(int(total_edges)),
                                                          C.byref(need)), "tlc_graph_components_work_bytes")
    return need.value


@_lib.on_device_of
def graph_components(node_ptr, edge_ptr, edges, work=None, total_nodes=None, max_nodes=None):
    """Connected components of a packed batch of RAW edge lists on the device, the largest component of every graph extracted,
    renumbered and deduplicated (tlc_graph_components; `data_utils_GC.largest_component`, integer for integer).

    node_ptr / edge_ptr int64[B+1], edges int32[sum m, 2] local ids: CUDA tensors; both orientations, repeated pairs and self loops are
    allowed and dropped.  Returns dict(info int32[B, 4] = (k, m, c, s) per graph -- nodes and distinct edges of the chosen component,
    components and distinct pairs of the whole graph --, new_id int32[sum n] (-1: dropped), out_edges int32[sum m, 2] (slot layout: the
    first m rows of graph g's input slot, (lo, hi) ascending), status uint8[B] (ST_OK / ST_BAD_INPUT; a refused graph's slots and info row
    keep what they held: -1 where the tensors are allocated here)).
    work: a 16-byte aligned uint8 CUDA tensor of at least `graph_components_work_bytes` (None: allocated).  total_nodes: sum n if the
    caller has it; else node_ptr[-1] is read.  max_nodes: an upper bound on one graph's nodes if the caller has it (a graph above it is
    refused): up to _lib.CC_WAVE_NMAX, or with total_nodes up to there, the call reads nothing back."""
    torch = _lib.require_gpu()
    dev = node_ptr.device
    B = node_ptr.numel() - 1
    tot_m = int(edges.shape[0])
    tot_n = int(total_nodes) if total_nodes is not None else (int(node_ptr[-1]) if B > 0 else 0)
    out = dict(info=torch.full((max(B, 1), 4), -1, dtype=torch.int32, device=dev),
               new_id=torch.full((max(tot_n, 1),), -1, dtype=torch.int32, device=dev),
               out_edges=torch.full((max(tot_m, 1), 2), -1, dtype=torch.int32, device=dev),
               status=torch.zeros(max(B, 1), dtype=torch.uint8, device=dev))
    if B > 0:
        if work is None:
            work = torch.empty(max(graph_components_work_bytes(B, tot_n, tot_m), 16), dtype=torch.uint8, device=dev)
        rc = _lib.lib().tlc_graph_components(_lib.ptr(node_ptr.contiguous()), _lib.ptr(edge_ptr.contiguous()), _lib.ptr(edges.contiguous()),
                                             C.c_int64(B), C.c_int64(tot_n), C.c_int64(tot_m), C.c_int64(-1 if max_nodes is None else int(max_nodes)),
                                             _lib.ptr(out["info"]), _lib.ptr(out["new_id"]), _lib.ptr(out["out_edges"]), _lib.ptr(out["status"]),
                                             _lib.ptr(work), C.c_int64(work.numel()), _lib.stream_ptr())
        _lib.check(rc, "tlc_graph_components")
    return dict(info=out["info"][:B], new_id=out["new_id"][:tot_n], out_edges=out["out_edges"][:tot_m], status=out["status"][:B])


def check_pd_large(pd_large):
    """'host' (tlc_pd_from_filtration alone: the one-workgroup HUGE tier, and no answer above its cap) or 'device' (the HUGE class and
    everything above it through tlc_pd_wide)."""
    if pd_large not in ("host", "device"):
        raise ValueError("pd_large should be 'host' or 'device', not %r" % (pd_large,))
    return pd_large


def pd_wide_work_bytes(sel_nodes, sel_edges):
    """Bytes of workspace tlc_pd_wide needs for graphs of these node / edge counts (the largest one's): host arithmetic, no device."""
    nodes, edges = [int(v) for v in sel_nodes], [int(v) for v in sel_edges]
    if len(nodes) != len(edges):
        raise ValueError("pd_wide_work_bytes: sel_nodes and sel_edges differ in length")
    need = C.c_int64(0)
    S = len(nodes)
    _lib.check(_lib.lib().tlc_pd_wide_work_bytes((C.c_int64 * max(S, 1))(*nodes), (C.c_int64 * max(S, 1))(*edges), C.c_int64(S), C.byref(need)),
               "tlc_pd_wide_work_bytes")
    return need.value


def _pd_outputs(torch, dev, B, sn, sm, want_rank):
    up = torch.zeros((max(sn, 1), 2), dtype=torch.float64, device=dev)
    down = torch.zeros((max(sn, 1), 2), dtype=torch.float64, device=dev)
    one = torch.zeros((max(sm, 1), 2), dtype=torch.float64, device=dev)
    ext0 = torch.zeros((max(B, 1), 2), dtype=torch.float64, device=dev)
    counts = torch.zeros((max(B, 1), 4), dtype=torch.int32, device=dev)
    rank = torch.zeros(max(sm, 1), dtype=torch.int32, device=dev) if want_rank else None
    return dict(up=up, down=down, one=one, ext0=ext0, counts=counts, edge_rank=rank)


def _pd_wide_into(out, node_offs, edge_offs, edges, f, flags, sel, work=None):
    """tlc_pd_wide on the graphs `sel` (host ints) into the full-size tensors of `out`; returns the stats of the last one.  A graph the
    entry refuses (TLC_ST_BAD_INPUT) raises RuntimeError after every selected graph has run."""
    torch = _lib.require_gpu()
    B = node_offs.numel() - 1
    sel = [int(g) for g in sel]
    stats = (C.c_int64 * _lib.PD_WIDE_N_STATS)()
    if not sel:
        return [0] * _lib.PD_WIDE_N_STATS
    if any(g < 0 or g >= B for g in sel):
        raise ValueError("pd_wide: sel outside 0 .. %d" % (B - 1))
    idx = torch.tensor(sel, dtype=torch.int64, device=f.device)
    sizes = torch.stack([node_offs[idx + 1] - node_offs[idx], edge_offs[idx + 1] - edge_offs[idx]]).cpu().clamp_(min=0)
    need = pd_wide_work_bytes(sizes[0].tolist(), sizes[1].tolist())
    if work is None:
        work = torch.empty(max(need, 16), dtype=torch.uint8, device=f.device)
    rc = _lib.lib().tlc_pd_wide(C.c_int64(B), _lib.ptr(node_offs), _lib.ptr(edge_offs), _lib.ptr(edges), _lib.ptr(f), C.c_uint32(flags),
                                (C.c_int64 * len(sel))(*sel), C.c_int64(len(sel)), _lib.ptr(out["up"]), _lib.ptr(out["down"]),
                                _lib.ptr(out["one"]), _lib.ptr(out["ext0"]), _lib.ptr(out["counts"]), _lib.ptr(out["edge_rank"]),
                                _lib.ptr(work), C.c_int64(work.numel()), stats, _lib.stream_ptr())
    _lib.check(rc, "tlc_pd_wide")
    bad = (out["counts"][idx, 0] == _lib.PD_WIDE_BAD_INPUT_ROW).nonzero().flatten().tolist()
    if bad:
        raise RuntimeError("pd_wide: graph(s) %s: ST_BAD_INPUT (offsets out of order, an id outside 0 .. n-1 or a self loop); their rows "
                           "hold %d, every other selected graph is computed" % ([sel[i] for i in bad], _lib.PD_WIDE_BAD_INPUT_ROW))
    return list(stats)


@_lib.on_device_of
def pd_wide(node_offs, edge_offs, edges, f, flags=0, sel=None, want_rank=False, work=None, out=None):
    """Extended persistence of big graphs on the whole device (tlc_pd_wide): no node cap, 32-bit ids, n + m up to
    _lib.PD_WIDE_MAX_ITEMS.  Arguments and the returned dict as `pd_from_filtration`, plus `stats` = [divide-and-conquer levels, Boruvka
    rounds, kernel launches, fallback ran, status] of the last selected graph.

    sel: the graphs to compute (host ints, any order; None: all); rows and slots of the others keep what `out` held (None: zeros).
    work: a uint8 CUDA tensor of at least `pd_wide_work_bytes` of the largest selected graph (None: allocated).  edge_rank is in this
    tier's own descending order: under equal keys a valid permutation, not the reference's.  A refused graph raises RuntimeError."""
    torch = _lib.require_gpu()
    B = node_offs.numel() - 1
    sn, sm = int(f.numel()), int(edges.shape[0])
    if out is None:
        out = _pd_outputs(torch, f.device, B, sn, sm, want_rank)
    node_offs, edge_offs, edges, f = node_offs.contiguous(), edge_offs.contiguous(), edges.contiguous(), f.contiguous()
    try:
        stats = _pd_wide_into(out, node_offs, edge_offs, edges, f, flags, range(B) if sel is None else sel, work)
    except RuntimeError as err:
        err.partial = out
        raise
    rank = out["edge_rank"]
    return dict(up=out["up"], down=out["down"], one=out["one"], ext0=out["ext0"][:B], counts=out["counts"][:B],
                edge_rank=None if rank is None else rank[:sm], stats=stats)


@_lib.on_device_of
def pd_from_filtration(node_offs, edge_offs, edges, f, flags=0, want_rank=True, pd_large="host"):
    """Batched perturb_filter_function + Union_find + Accelerate_PD (sg2dgm/accelerated_PD.py:6-178).

    All arguments CUDA tensors: node_offs/edge_offs int64[B+1], edges int32[sum m,2], f float64[sum n].
    Returns dict(up, down, one, ext0, counts, edge_rank) of CUDA tensors (layout: include/tlcgnn.h).

    pd_large='host' (default): tlc_pd_from_filtration alone -- a graph above PD_L_NMAX nodes or PD_L_MMAX edges runs in one workgroup, one
    above 65 535 nodes or 2^24 - 2 edges is not computed (counts row -1).  'device': those graphs (picked from the offsets on the
    device) go through `pd_wide` instead, the rest through the same launch as before; edge_rank of the rerouted graphs is then in
    pd_wide's order.
    """
    check_pd_large(pd_large)
    torch = _lib.require_gpu()
    dev = f.device
    B = node_offs.numel() - 1
    sn, sm = int(f.numel()), int(edges.shape[0])
    out = _pd_outputs(torch, dev, B, sn, sm, want_rank)
    up, down, one, ext0, counts, rank = out["up"], out["down"], out["one"], out["ext0"], out["counts"], out["edge_rank"]
    edges = edges.contiguous()
    node_offs, edge_offs, f = node_offs.contiguous(), edge_offs.contiguous(), f.contiguous()
    wide = []
    if pd_large == "device" and B > 0:
        n_g, m_g = node_offs[1:] - node_offs[:-1], edge_offs[1:] - edge_offs[:-1]
        wide = ((n_g > _lib.PD_L_NMAX) | (m_g > _lib.PD_L_MMAX)).nonzero().flatten().tolist()
    if wide:
        # the entry takes consecutive offsets only, so the graphs that stay are gathered into a packed batch of their own, computed
        # by the same entry, and their slots scattered back (`_pd_from_filtration_subset`); the rerouted ones go through tlc_pd_wide
        keep = torch.ones(B, dtype=torch.bool, device=dev)
        keep[torch.tensor(wide, dtype=torch.int64, device=dev)] = False
        sub = keep.nonzero().flatten()
        _pd_from_filtration_subset(node_offs, edge_offs, edges, f, flags, sub, out)
        _pd_wide_into(out, node_offs, edge_offs, edges, f, flags, wide)
    else:
        rc = _lib.lib().tlc_pd_from_filtration(C.c_int32(B), _lib.ptr(node_offs), _lib.ptr(edge_offs),
                                               _lib.ptr(edges), _lib.ptr(f), C.c_uint32(flags), _lib.ptr(up),
                                               _lib.ptr(down), _lib.ptr(one), _lib.ptr(ext0), _lib.ptr(counts),
                                               _lib.ptr(rank), _lib.stream_ptr())
        _lib.check(rc, "tlc_pd_from_filtration")
    return dict(up=up, down=down, one=one, ext0=ext0[:B], counts=counts[:B], edge_rank=None if rank is None else rank[:sm])


def _pd_from_filtration_subset(node_offs, edge_offs, edges, f, flags, sub, out):
    """tlc_pd_from_filtration on the graphs `sub` (int64 CUDA tensor, ascending) of a packed batch, into the full-size tensors of `out`.
    The entry takes per-graph START offsets only through consecutive arrays, so the kept graphs are gathered into a packed batch of
    their own with torch ops on the device, computed, and their slots scattered back."""
    torch = _lib.require_gpu()
    S = int(sub.numel())
    if S == 0:
        return None
    dev = f.device
    n_g, m_g = (node_offs[1:] - node_offs[:-1])[sub], (edge_offs[1:] - edge_offs[:-1])[sub]
    zero = torch.zeros(1, dtype=torch.int64, device=dev)
    no2, eo2 = torch.cat([zero, n_g.cumsum(0)]), torch.cat([zero, m_g.cumsum(0)])
    sn2, sm2 = int(no2[-1]), int(eo2[-1])
    # position i of the gathered batch <- position src[i] of the full one
    gn = torch.repeat_interleave(torch.arange(S, device=dev), n_g)
    src_n = torch.arange(sn2, device=dev) - no2[:-1][gn] + node_offs[:-1][sub][gn]
    ge = torch.repeat_interleave(torch.arange(S, device=dev), m_g)
    src_e = torch.arange(sm2, device=dev) - eo2[:-1][ge] + edge_offs[:-1][sub][ge]
    f2 = f[src_n].contiguous()
    e2 = edges[src_e].contiguous() if sm2 else torch.zeros((1, 2), dtype=torch.int32, device=dev)
    o2 = _pd_outputs(torch, dev, S, sn2, sm2, out["edge_rank"] is not None)
    rc = _lib.lib().tlc_pd_from_filtration(C.c_int32(S), _lib.ptr(no2), _lib.ptr(eo2), _lib.ptr(e2), _lib.ptr(f2), C.c_uint32(flags),
                                           _lib.ptr(o2["up"]), _lib.ptr(o2["down"]), _lib.ptr(o2["one"]), _lib.ptr(o2["ext0"]),
                                           _lib.ptr(o2["counts"]), _lib.ptr(o2["edge_rank"]), _lib.stream_ptr())
    _lib.check(rc, "tlc_pd_from_filtration")
    if sn2:
        out["up"][src_n] = o2["up"][:sn2]
        out["down"][src_n] = o2["down"][:sn2]
    if sm2:
        out["one"][src_e] = o2["one"][:sm2]
        if out["edge_rank"] is not None:
            out["edge_rank"][src_e] = o2["edge_rank"][:sm2]
    out["ext0"][sub] = o2["ext0"][:S]
    out["counts"][sub] = o2["counts"][:S]
    return o2


def pd_grad_work_bytes(max_nodes, max_edges):
    """Bytes of workspace `pd_point_vertices` / `pd_filtration_grad` need for a batch whose largest graph has this many nodes and its
    largest edge list this many edges (tlc_pd_grad_work_bytes): host arithmetic, no device; 0 up to _lib.PD_VERT_LDS_NMAX nodes."""
    need = C.c_int64(0)
    _lib.check(_lib.lib().tlc_pd_grad_work_bytes(C.c_int64(int(max_nodes)), C.c_int64(int(max_edges)), C.byref(need)), "tlc_pd_grad_work_bytes")
    return need.value


def _pd_grad_work(torch, node_offs, edge_offs, work):
    """(workspace tensor or None, its bytes) for the batch: allocated from the largest node / edge count unless the caller's is given."""
    if work is not None:
        return work, int(work.numel())
    if node_offs.numel() < 2:
        return None, 0
    top = torch.stack([(node_offs[1:] - node_offs[:-1]).max(), (edge_offs[1:] - edge_offs[:-1]).max()]).clamp_(min=0).tolist()
    need = pd_grad_work_bytes(top[0], top[1])
    return (torch.empty(need, dtype=torch.uint8, device=node_offs.device) if need else None), need


VERTEX_KEYS = ("up", "down", "one", "ext0")


@_lib.on_device_of
def pd_point_vertices(node_offs, edge_offs, f, pd, work=None):
    """The vertex behind every coordinate of the diagrams `pd` (the dict `pd_from_filtration` or `pd_wide` returned for this f):
    the lowest local id v with f[v] == c (tlc_pd_point_vertices).  Returns dict(up, down int32[sum n, 2], one
    int32[sum m, 2], ext0 int32[B, 2], status uint8[B]); -1 behind a slot's points.  status: ST_OK, ST_TOO_LARGE (a counts row of -1),
    ST_BAD_INPUT (a refused graph, or a coordinate no vertex holds: that entry is -1).  work: a uint8 CUDA tensor of
    `pd_grad_work_bytes` (None: allocated; none is needed up to _lib.PD_VERT_LDS_NMAX nodes)."""
    torch = _lib.require_gpu()
    dev = f.device
    B = node_offs.numel() - 1
    node_offs, edge_offs, f = node_offs.contiguous(), edge_offs.contiguous(), f.contiguous()
    up, down, one = pd["up"].contiguous(), pd["down"].contiguous(), pd["one"].contiguous()
    ext0, counts = pd["ext0"].contiguous(), pd["counts"].contiguous()
    out = dict(up=torch.full((up.shape[0], 2), -1, dtype=torch.int32, device=dev),
               down=torch.full((down.shape[0], 2), -1, dtype=torch.int32, device=dev),
               one=torch.full((one.shape[0], 2), -1, dtype=torch.int32, device=dev),
               ext0=torch.full((max(B, 1), 2), -1, dtype=torch.int32, device=dev),
               status=torch.zeros(max(B, 1), dtype=torch.uint8, device=dev))
    work, nbytes = _pd_grad_work(torch, node_offs, edge_offs, work)
    rc = _lib.lib().tlc_pd_point_vertices(C.c_int64(B), _lib.ptr(node_offs), _lib.ptr(edge_offs), _lib.ptr(f), _lib.ptr(up), _lib.ptr(down),
                                          _lib.ptr(one), _lib.ptr(ext0), _lib.ptr(counts), _lib.ptr(out["up"]), _lib.ptr(out["down"]),
                                          _lib.ptr(out["one"]), _lib.ptr(out["ext0"]), _lib.ptr(out["status"]), _lib.ptr(work),
                                          C.c_int64(nbytes), _lib.stream_ptr())
    _lib.check(rc, "tlc_pd_point_vertices")
    out["ext0"], out["status"] = out["ext0"][:B], out["status"][:B]
    return out


@_lib.on_device_of
def pd_filtration_grad(node_offs, edge_offs, counts, verts, g_up=None, g_down=None, g_one=None, g_ext0=None, work=None, out=None):
    """grad_f float64[sum n]: per vertex, the sum of the gradients g_* (float64, each in the layout of its slot; None: zeros) of the
    coordinates `verts` (the dict of `pd_point_vertices`) assigns to it, in the fixed order of tlc_pd_filtration_grad -- no atomics, the
    same bits every run.  Slices of graphs whose status is not ST_OK keep what `out` held (None: zeros)."""
    torch = _lib.require_gpu()
    dev = node_offs.device
    B = node_offs.numel() - 1
    node_offs, edge_offs, counts = node_offs.contiguous(), edge_offs.contiguous(), counts.contiguous()
    sn = int(verts["up"].shape[0])
    if out is None:
        out = torch.zeros(sn, dtype=torch.float64, device=dev)
    grads = []
    for key, g in zip(VERTEX_KEYS, (g_up, g_down, g_one, g_ext0)):
        if g is not None:
            g = g.to(torch.float64).contiguous()
            if g.shape[0] < (B if key == "ext0" else verts[key].shape[0]) or g.shape[-1] != 2:
                raise ValueError("pd_filtration_grad: g_%s has shape %s, its slot %s" % (key, tuple(g.shape), tuple(verts[key].shape)))
        grads.append(g)
    work, nbytes = _pd_grad_work(torch, node_offs, edge_offs, work)
    status = verts["status"].contiguous()
    rc = _lib.lib().tlc_pd_filtration_grad(C.c_int64(B), _lib.ptr(node_offs), _lib.ptr(edge_offs), _lib.ptr(counts),
                                           _lib.ptr(verts["up"]), _lib.ptr(verts["down"]), _lib.ptr(verts["one"]), _lib.ptr(verts["ext0"]),
                                           _lib.ptr(grads[0]), _lib.ptr(grads[1]), _lib.ptr(grads[2]), _lib.ptr(grads[3]),
                                           _lib.ptr(status) if B > 0 else None, _lib.ptr(out), _lib.ptr(work), C.c_int64(nbytes),
                                           _lib.stream_ptr())
    _lib.check(rc, "tlc_pd_filtration_grad")
    return out


@_lib.on_device_of
def pi_raster(offs, pts, res=5):
    """Batched PersistenceImager(resolution=res).transform (sg2dgm/PersistenceImager.pyx:352-388).

    offs int64[B+1], pts float64[sum k, 2] (birth, death) CUDA tensors -> float64[B, res*res].
    """
    torch = _lib.require_gpu()
    B = offs.numel() - 1
    out = torch.empty((max(B, 1), res * res), dtype=torch.float64, device=offs.device)
    pts = pts.contiguous()
    rc = _lib.lib().tlc_pi_raster(C.c_int32(B), _lib.ptr(offs.contiguous()), _lib.ptr(pts) if pts.numel() else None,
                                  C.c_int(res), _lib.ptr(out), _lib.stream_ptr())
    _lib.check(rc, "tlc_pi_raster")
    return out[:B]


@_lib.on_device_of
def pi_raster_wgrad(offs, pts, grad_img, res=5):
    """d images / d points of the reference's differentiable imager (pimg.py:354-400: through the weights only) contracted with
    grad_img float64[B, res*res] -> float64[N, 2] (tlc_pi_raster_wgrad)."""
    torch = _lib.require_gpu()
    B = offs.numel() - 1
    pts = pts.contiguous()
    grad_img = grad_img.contiguous()
    out = torch.zeros((max(pts.shape[0], 1), 2), dtype=torch.float64, device=offs.device)
    rc = _lib.lib().tlc_pi_raster_wgrad(C.c_int32(B), C.c_int64(pts.shape[0]), _lib.ptr(offs.contiguous()), _lib.ptr(pts) if pts.numel() else None,
                                        C.c_int(res), _lib.ptr(grad_img), _lib.ptr(out), _lib.stream_ptr())
    _lib.check(rc, "tlc_pi_raster_wgrad")
    return out[:pts.shape[0]]


class PiSpec:
    """One specification of the general imager (tlc_pi_image, include/tlcgnn.h): the grid lines as the imager object holds them
    (bpnts [Rb + 1], ppnts [Rp + 1]), the ramp (low, high, start, end), the covariance (var_b, var_p, cov) and the skew flag.
    Host data only; the library checks it (a refusal is a TlcError that says why)."""

    def __init__(self, bpnts, ppnts, ramp=(0.0, 1.0, 0.0, 1.0), sigma=(1.0, 1.0, 0.0), skew=True):
        self.bpnts = np.ascontiguousarray(np.asarray(bpnts, dtype=np.float64).reshape(-1))
        self.ppnts = np.ascontiguousarray(np.asarray(ppnts, dtype=np.float64).reshape(-1))
        self.ramp = np.ascontiguousarray(np.asarray(ramp, dtype=np.float64).reshape(4))
        self.sigma = np.ascontiguousarray(np.asarray(sigma, dtype=np.float64).reshape(3))
        self.skew = bool(skew)

    @property
    def resolution(self):
        return (self.bpnts.size - 1, self.ppnts.size - 1)

    @classmethod
    def default(cls, res=5):
        """PersistenceImager(resolution=res) of the reference: unit ranges, sigma = I, the default ramp -- what `pi_raster` computes."""
        lines = np.linspace(0.0, 1.0 + 1.0 / res, res + 1, endpoint=False, dtype=np.float64)
        return cls(lines, lines.copy())

    def _c_args(self):
        p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        rb, rp = self.resolution
        return (C.c_int32(rb), C.c_int32(rp), p(self.bpnts), p(self.ppnts), p(self.ramp), p(self.sigma), C.c_int32(int(self.skew)))


def pi_image_work_bytes(n_dgms, max_points, spec):
    """(full, least) bytes of `pi_image`'s workspace (tlc_pi_image_work_bytes): 0 unless a diagram has more than _lib.PI_SLICE points;
    any size from `least` up gives the same bits."""
    rb, rp = spec.resolution
    least = C.c_int64(0)
    full = _lib.lib().tlc_pi_image_work_bytes(C.c_int32(n_dgms), C.c_int64(max_points), C.c_int32(rb), C.c_int32(rp), C.byref(least))
    if full < 0:
        _lib.check(1, "tlc_pi_image_work_bytes")
    return int(full), int(least.value)


_PI_WORK_CAP = 1 << 28          # a workspace pi_image allocates itself stays below this unless one diagram needs more


@_lib.on_device_of
def pi_image(offs, pts, spec, weights=None, work=None):
    """Batched persistence images of any imager specification (tlc_pi_image; csrc/pi_general.hip).

    offs int64[B+1], pts float64[K, 2] CUDA tensors, spec a PiSpec, weights float64[K] (optional: overrides the ramp), work an optional
    uint8 CUDA workspace -> float64[B, Rb * Rp], row-major [birth_bin, pers_bin].  The offsets are copied to the host once."""
    torch = _lib.require_gpu()
    B = offs.numel() - 1
    rb, rp = spec.resolution
    out = torch.empty((max(B, 1), rb * rp), dtype=torch.float64, device=offs.device)
    offs = offs.contiguous()
    pts = pts.contiguous()
    assert pts.dtype == torch.float64 and offs.dtype == torch.int64
    if weights is not None:
        weights = weights.contiguous()
        assert weights.dtype == torch.float64 and weights.numel() == pts.shape[0]
    h_offs = np.ascontiguousarray(offs.cpu().numpy())
    max_points = int(np.diff(h_offs).max()) if B > 0 else 0
    nbytes = 0
    if max_points > _lib.PI_SLICE:
        if work is None:
            full, least = pi_image_work_bytes(B, max_points, spec)
            work = torch.empty(max(least, min(full, _PI_WORK_CAP)), dtype=torch.uint8, device=offs.device)
        nbytes = work.numel()
    rc = _lib.lib().tlc_pi_image(C.c_int32(B), C.c_int64(pts.shape[0]), _lib.ptr(offs), h_offs.ctypes.data_as(C.c_void_p),
                                 _lib.ptr(pts) if pts.numel() else None, _lib.ptr(weights) if weights is not None and weights.numel() else None,
                                 *spec._c_args(), _lib.ptr(out), _lib.ptr(work) if nbytes else None, C.c_int64(nbytes), _lib.stream_ptr())
    _lib.check(rc, "tlc_pi_image")
    return out[:B]


@_lib.on_device_of
def pi_image_vjp(offs, pts, grad_img, spec, mode="weight"):
    """d (sum grad_img * pi_image) / d pts -> float64[K, 2] (tlc_pi_image_vjp).  mode 'weight': the reference's gradient, through a
    point's weight only; 'full': the true derivative (separable sigma only)."""
    if mode not in ("weight", "full"):
        raise ValueError("pi_image_vjp: mode is %r, not 'weight' or 'full'" % (mode,))
    torch = _lib.require_gpu()
    B = offs.numel() - 1
    pts = pts.contiguous()
    grad_img = grad_img.contiguous()
    rb, rp = spec.resolution
    assert pts.dtype == torch.float64 and grad_img.dtype == torch.float64 and grad_img.numel() == B * rb * rp
    out = torch.zeros((max(pts.shape[0], 1), 2), dtype=torch.float64, device=offs.device)
    rc = _lib.lib().tlc_pi_image_vjp(C.c_int32(B), C.c_int64(pts.shape[0]), _lib.ptr(offs.contiguous()), _lib.ptr(pts) if pts.numel() else None,
                                     *spec._c_args(), C.c_int32(_lib.PI_GRAD_FULL if mode == "full" else _lib.PI_GRAD_WEIGHT),
                                     _lib.ptr(grad_img) if grad_img.numel() else None, _lib.ptr(out), _lib.stream_ptr())
    _lib.check(rc, "tlc_pi_image_vjp")
    return out[:pts.shape[0]]


def landscape_work_bytes(n_dgms, max_points, K, T):
    """(full, least) bytes of `landscape`'s workspace (tlc_landscape_work_bytes): 0 unless a diagram has more than _lib.LS_LDS_NMAX
    points; any size from `least` up gives the same bits."""
    least = C.c_int64(0)
    full = _lib.lib().tlc_landscape_work_bytes(C.c_int32(int(n_dgms)), C.c_int64(int(max_points)), C.c_int32(int(K)), C.c_int32(int(T)),
                                               C.byref(least))
    if full < 0:
        _lib.check(1, "tlc_landscape_work_bytes")
    return int(full), int(least.value)


def _landscape_sizes(what, pts, offs, ts, K):
    """The checks `landscape` and `landscape_vjp` share -> (B, T, max_points); the offsets are read once (offsets beyond the points
    would be read out of bounds on the device)."""
    import torch
    if ts.dim() != 1:
        raise ValueError("%s: ts should be 1-D, not %s" % (what, tuple(ts.shape)))
    T, K = int(ts.numel()), int(K)
    if not 1 <= T <= _lib.LS_TMAX:
        raise ValueError("%s: %d samples, outside 1 .. %d" % (what, T, _lib.LS_TMAX))
    if not 1 <= K <= _lib.LS_KMAX:
        raise ValueError("%s: K = %d, outside 1 .. %d" % (what, K, _lib.LS_KMAX))
    B = offs.numel() - 1
    max_points = 0
    if B > 0:
        cnt = offs[1:] - offs[:-1]
        end, max_points = torch.stack([offs[-1], cnt.max()]).tolist()
        if end > pts.shape[0]:
            raise ValueError("%s: the offsets end at %d but there are %d points" % (what, end, pts.shape[0]))
    return B, T, max(int(max_points), 0)


@_lib.on_device_of
def landscape(pts, offs, ts, K, winners=True, work=None):
    """Persistence landscapes of packed diagrams (tlc_landscape; csrc/landscape.hip; include/tlcgnn.h defines them).

    pts float64[sum n, 2] (birth, death), offs int64[B + 1], ts float64[T] sample values (CUDA tensors), K levels, work an optional
    uint8 CUDA workspace (only diagrams above _lib.LS_LDS_NMAX points use one) -> (out float64[B, K, T], winner int32[B, K, T] or
    None, status uint8[B]: 0 ok, 3 = a NaN / Inf coordinate).  The offsets and the samples are read back once."""
    B, T, max_points = _landscape_sizes("landscape", pts, offs, ts, K)
    torch = _lib.require_gpu()
    dev = offs.device
    pts, offs, ts = pts.contiguous(), offs.contiguous(), ts.contiguous()
    assert pts.dtype == torch.float64 and offs.dtype == torch.int64 and ts.dtype == torch.float64
    out = torch.empty((max(B, 1), int(K), T), dtype=torch.float64, device=dev)
    win = torch.empty((max(B, 1), int(K), T), dtype=torch.int32, device=dev) if winners else None
    status = torch.zeros(max(B, 1), dtype=torch.uint8, device=dev)
    nbytes = 0
    if max_points > _lib.LS_LDS_NMAX:
        if work is None:
            work = torch.empty(landscape_work_bytes(B, max_points, K, T)[0], dtype=torch.uint8, device=dev)
        nbytes = work.numel()
    rc = _lib.lib().tlc_landscape(C.c_int32(B), _lib.ptr(offs), _lib.ptr(pts) if pts.numel() else None, C.c_int32(T), _lib.ptr(ts),
                                  C.c_int32(int(K)), C.c_int64(max_points), _lib.ptr(out), _lib.ptr(win), _lib.ptr(status),
                                  _lib.ptr(work) if nbytes else None, C.c_int64(nbytes), _lib.stream_ptr())
    _lib.check(rc, "tlc_landscape")
    return out[:B], (win[:B] if winners else None), status[:B]


@_lib.on_device_of
def landscape_vjp(pts, offs, ts, K, winner, grad_out):
    """d (sum grad_out * landscape) / d pts -> float64[sum n, 2] (tlc_landscape_vjp): winner int32[B, K, T] is `landscape`'s output,
    grad_out float64[B, K, T].  A +-1 selection summed in one fixed order by one owner per point."""
    B, T, max_points = _landscape_sizes("landscape_vjp", pts, offs, ts, K)
    torch = _lib.require_gpu()
    pts, offs, ts = pts.contiguous(), offs.contiguous(), ts.contiguous()
    winner, grad_out = winner.contiguous(), grad_out.contiguous()
    assert pts.dtype == torch.float64 and offs.dtype == torch.int64 and ts.dtype == torch.float64
    assert winner.dtype == torch.int32 and grad_out.dtype == torch.float64
    assert winner.numel() == B * int(K) * T and grad_out.numel() == B * int(K) * T
    out = torch.zeros((max(pts.shape[0], 1), 2), dtype=torch.float64, device=offs.device)
    rc = _lib.lib().tlc_landscape_vjp(C.c_int32(B), _lib.ptr(offs), _lib.ptr(pts) if pts.numel() else None, C.c_int32(T), _lib.ptr(ts),
                                      C.c_int32(int(K)), C.c_int64(max_points), _lib.ptr(winner), _lib.ptr(grad_out), _lib.ptr(out),
                                      _lib.stream_ptr())
    _lib.check(rc, "tlc_landscape_vjp")
    return out[:pts.shape[0]]


def dgm_gram_flags(mirror, paired, symmetric=False):
    """The TLC_DG_* flag word of `dgm_gram` / `dgm_gram_vjp`."""
    return ((_lib.DG_PAIRED if paired else _lib.DG_ALL) | (_lib.DG_SYMMETRIC if symmetric else 0) | (_lib.DG_MIRROR if mirror else 0))


def dgm_gram_work_bytes(nx, ny, max_nx_points, max_ny_points, flags):
    """(full, least) bytes of the workspace of `dgm_gram` and `dgm_gram_vjp` (tlc_dgm_gram_work_bytes): 0 while no diagram of X has more
    than 64 points and none of Y more than _lib.DG_GROUP; any size from `least` up gives the same bits."""
    least = C.c_int64(0)
    full = _lib.lib().tlc_dgm_gram_work_bytes(C.c_int32(int(nx)), C.c_int32(int(ny)), C.c_int64(int(max_nx_points)), C.c_int64(int(max_ny_points)),
                                              C.c_uint32(int(flags)), C.byref(least))
    if full < 0:
        _lib.check(1, "tlc_dgm_gram_work_bytes")
    return int(full), int(least.value)


def _dgm_gram_side(what, name, pts, offs, w):
    """The checks of one side -> (B, max_points); the offsets are read once (offsets beyond the points would be read out of bounds)."""
    import torch
    assert pts.dtype == torch.float64 and offs.dtype == torch.int64 and pts.dim() == 2 and pts.shape[1] == 2
    assert pts.is_contiguous() and offs.is_contiguous() and (w is None or (w.dtype == torch.float64 and w.is_contiguous()))
    B = offs.numel() - 1
    if B < 0:
        raise ValueError("%s: %soff is empty" % (what, name))
    if w is not None and w.shape != (pts.shape[0],):
        raise ValueError("%s: w%s should hold one weight per point (%d), not shape %s" % (what, name, pts.shape[0], tuple(w.shape)))
    max_points = 0
    if B > 0:
        end, max_points = torch.stack([offs[-1], (offs[1:] - offs[:-1]).max()]).tolist()
        if end > pts.shape[0]:
            raise ValueError("%s: the offsets of %s end at %d but there are %d points" % (what, name, end, pts.shape[0]))
    return B, max(int(max_points), 0)


def _dgm_gram_call(what, x, xoff, wx, y, yoff, wy, flags, work):
    torch = _lib.require_gpu()
    nx, max_nx = _dgm_gram_side(what, "x", x, xoff, wx)
    if flags & _lib.DG_SYMMETRIC:
        ny, max_ny = nx, max_nx
    else:
        ny, max_ny = _dgm_gram_side(what, "y", y, yoff, wy)
    if (flags & _lib.DG_PAIRED) and nx != ny:
        raise ValueError("%s: paired, but x holds %d diagrams and y %d" % (what, nx, ny))
    nbytes = 0
    full, _ = dgm_gram_work_bytes(nx, ny, max_nx, max_ny, flags)
    if full > 0:
        if work is None:
            work = torch.empty(full, dtype=torch.uint8, device=xoff.device)
        nbytes = work.numel()
    sizes = (C.c_int64(max_nx), C.c_int64(max_ny))
    # (the workspace travels with its pointer: it has to outlive the call that is made with it)
    return nx, ny, sizes, work, (_lib.ptr(work) if nbytes else None, C.c_int64(nbytes), _lib.stream_ptr())


def _dgm_gram_operands(x, xoff, wx, y, yoff, wy, nx, ny):
    p = lambda t: _lib.ptr(t) if t is not None and t.numel() else None                    # noqa: E731
    return (C.c_int32(nx), _lib.ptr(xoff), p(x), p(wx), C.c_int32(ny), _lib.ptr(yoff), p(y), p(wy))


@_lib.on_device_of
def dgm_gram(x, xoff, wx, y, yoff, wy, gamma, scale, mirror, paired=False, symmetric=False, work=None):
    """k(X_i, Y_j) = scale * sum_p sum_q w_p w_q (e1 - mirror * e2) between packed diagrams (tlc_dgm_gram; csrc/dgm_gram.hip;
    include/tlcgnn.h defines it and its summation order).

    x float64[sum n, 2], xoff int64[Bx + 1], wx float64[sum n] or None (every weight 1), y / yoff / wy likewise (CUDA tensors);
    symmetric=True: y, yoff and wy are not read, Y is X and only j >= i is computed.  work: an optional uint8 CUDA workspace.
    -> (out float64[Bx, By], or [B] with paired=True; status_x uint8[Bx], status_y uint8[By]: 3 = a NaN / Inf coordinate or weight, the
    diagram's row / column of out is NaN).  The offsets are read back once."""
    torch = _lib.require_gpu()
    if symmetric:
        y, yoff, wy = x, xoff, wx
    flags = dgm_gram_flags(mirror, paired, symmetric)
    nx, ny, sizes, work, tail = _dgm_gram_call("dgm_gram", x, xoff, wx, y, yoff, wy, flags, work)
    dev = xoff.device
    out = torch.empty((max(nx, 1),) if paired else (max(nx, 1), max(ny, 1)), dtype=torch.float64, device=dev)
    sx = torch.zeros(max(nx, 1), dtype=torch.uint8, device=dev)
    sy = torch.zeros(max(ny, 1), dtype=torch.uint8, device=dev)
    rc = _lib.lib().tlc_dgm_gram(*_dgm_gram_operands(x, xoff, wx, y, yoff, wy, nx, ny), C.c_double(float(gamma)), C.c_double(float(scale)),
                                 C.c_uint32(flags), *sizes, _lib.ptr(out), _lib.ptr(sx), _lib.ptr(sy), *tail)
    _lib.check(rc, "tlc_dgm_gram")
    return (out[:nx] if paired else out[:nx, :ny]), sx[:nx], sy[:ny]


@_lib.on_device_of
def dgm_gram_vjp(x, xoff, wx, y, yoff, wy, gamma, scale, mirror, status_x, status_y, grad_out, paired=False, work=None):
    """d (sum grad_out * gram) / d (x, wx) with Y held fixed (tlc_dgm_gram_vjp) -> (float64[sum n, 2], float64[sum n] or None without wx).
    status_x / status_y: `dgm_gram`'s; grad_out float64[Bx, By] or [B].  The gradient in (y, wy) is this call with the roles swapped and
    grad_out transposed."""
    torch = _lib.require_gpu()
    flags = dgm_gram_flags(mirror, paired, False)
    nx, ny, sizes, work, tail = _dgm_gram_call("dgm_gram_vjp", x, xoff, wx, y, yoff, wy, flags, work)
    grad_out, status_x, status_y = grad_out.contiguous(), status_x.contiguous(), status_y.contiguous()
    assert grad_out.dtype == torch.float64 and grad_out.numel() == (nx if paired else nx * ny)
    assert status_x.dtype == torch.uint8 and status_x.numel() == nx and status_y.dtype == torch.uint8 and status_y.numel() == ny
    rows = x.shape[0]
    gx = torch.zeros((max(rows, 1), 2), dtype=torch.float64, device=xoff.device)
    gw = None if wx is None else torch.zeros(max(rows, 1), dtype=torch.float64, device=xoff.device)
    if rows == 0:
        return gx[:0], (None if gw is None else gw[:0])
    p = lambda t: _lib.ptr(t) if t.numel() else None                                      # noqa: E731
    rc = _lib.lib().tlc_dgm_gram_vjp(*_dgm_gram_operands(x, xoff, wx, y, yoff, wy, nx, ny), C.c_double(float(gamma)), C.c_double(float(scale)),
                                     C.c_uint32(flags), *sizes, p(status_x), p(status_y), p(grad_out), _lib.ptr(gx), _lib.ptr(gw), *tail)
    _lib.check(rc, "tlc_dgm_gram_vjp")
    return gx[:rows], (None if gw is None else gw[:rows])


# size tiers of the PD kernel (csrc/tlc_kernels.h) and what the library's timing slots bracket
TIER_LIMITS = [("pd_tier_small", 64, 128), ("pd_tier_mid", 128, 256), ("pd_tier_medium", 512, 1024), ("pd_tier_large", 2048, 4096)]
TINY_LIMITS = (16, 24)          # TLC_T_NMAX / TLC_T_MMAX: lane-per-subgraph kernel (plain image batches at resolution 5)
MEDIUM_MANY_POS = 120           # TLC_MH_MIN_POS: MEDIUM-sized vicinities with at least this many Pos edges (m - n + 1)
MEDIUM_COMPACT = (384, 512)     # TLC_C_NMAX / TLC_C_MMAX: the compact configuration of the MEDIUM-sized tiers (beyond it: MEDWIDE)


def tier_of(n, m2, tiny=True):
    """Which kernel's TIMING SLOT covers each pair, from (|S|, induced directed entries), mirroring tlc_scan_bin and run_chunk:
    'pd_tier_small' = the wavefront-per-subgraph SMALL kernel only -- the pairs of the lane-per-subgraph kernel are
    'pd_tier_tiny' (no slot of its own); 'pd_tier_medium' = the MEDIUM-sized vicinities with many Pos edges or beyond the compact
    kernel configuration (the launch that slot brackets), the rest of the MEDIUM tier is 'pd_tier_medium_rest' (not bracketed);
    '' for pairs finished early.
    So bytes summed over the pairs of a name and the time of that name's slot cover the same work."""
    n = np.asarray(n)
    m = np.asarray(m2) // 2
    out = np.full(n.shape, "pd_tier_huge", dtype=object)
    for name, nm, mm in reversed(TIER_LIMITS):
        out[(n <= nm) & (m <= mm)] = name
    med = out == "pd_tier_medium"
    out[med & (m - n + 1 < MEDIUM_MANY_POS) & (n <= MEDIUM_COMPACT[0]) & (m <= MEDIUM_COMPACT[1])] = "pd_tier_medium_rest"
    if tiny:
        out[(n <= TINY_LIMITS[0]) & (m <= TINY_LIMITS[1])] = "pd_tier_tiny"
    out[n <= 0] = ""
    return out


def algorithmic_bytes(rowptr, col, pairs, hop, res=5):
    """SURVEY.md 8(d) byte model per pair (host-side accounting through the C ABI; no GPU needed)."""
    rowptr = np.ascontiguousarray(rowptr, dtype=np.int32)
    col = np.ascontiguousarray(col, dtype=np.int32)
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    out = np.zeros(len(pairs), dtype=np.float64)
    rc = _lib.lib().tlc_pd_pi_algorithmic_bytes(C.c_int32(len(rowptr) - 1), rowptr.ctypes.data_as(C.c_void_p),
                                                col.ctypes.data_as(C.c_void_p), pairs.ctypes.data_as(C.c_void_p),
                                                C.c_int64(len(pairs)), C.c_int(hop), C.c_int(res),
                                                out.ctypes.data_as(C.c_void_p))
    _lib.check(rc, "tlc_pd_pi_algorithmic_bytes")
    return out


# ---- the negative list of loaddatas.py:44-45 and the sparse image store ----------------------------
class ComplementIndex:
    """Non-edges of a symmetric 0/1 adjacency in the order of `sp.triu(sp.csr_matrix(1. - adj.toarray())).nonzero()`
    (loaddatas.py:44), addressed by list number on the device -- no N x N matrix, no [n_neg, 2] array.

    rowptr/col: numpy CSR of the symmetric adjacency, columns ascending and unique inside a row (checked here)."""

    def __init__(self, rowptr, col, device=None):
        torch = _lib.require_gpu()
        rowptr = np.ascontiguousarray(rowptr, dtype=np.int32)
        col = np.ascontiguousarray(col, dtype=np.int32)
        n = len(rowptr) - 1
        if len(col):
            inner = np.ones(len(col), dtype=bool)
            inner[rowptr[:-1][rowptr[:-1] < len(col)]] = False          # first entry of every non-empty row
            if not np.all(np.diff(col.astype(np.int64))[inner[1:]] > 0):
                raise ValueError("ComplementIndex: CSR columns must be ascending and unique inside every row")
        dev = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
        self.n_nodes = n
        self.rowptr = torch.from_numpy(rowptr).to(dev)
        self.col = torch.from_numpy(col).to(dev) if len(col) else torch.zeros(1, dtype=torch.int32, device=dev)
        self.row_start = torch.empty(n + 1, dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            rc = _lib.lib().tlc_complement_rows(C.c_int32(n), _lib.ptr(self.rowptr), _lib.ptr(self.col),
                                                _lib.ptr(self.row_start), _lib.stream_ptr())
        _lib.check(rc, "tlc_complement_rows")
        self.n_neg = int(self.row_start[-1].item())

    def __len__(self):
        return self.n_neg

    def pairs(self, ranks=None, first=0, count=None, out=None):
        """int32 CUDA [count, 2]: the pairs numbered ranks[...] (int64 CUDA tensor) or first .. first+count-1."""
        import torch
        if ranks is not None:
            assert ranks.is_cuda and ranks.dtype == torch.int64
            ranks = ranks.contiguous()
            count = ranks.numel()
        elif count is None:
            count = self.n_neg - first
        if out is None:
            out = torch.empty((count, 2), dtype=torch.int32, device=self.rowptr.device)
        with torch.cuda.device(self.rowptr.device):
            rc = _lib.lib().tlc_complement_pairs(C.c_int32(self.n_nodes), _lib.ptr(self.rowptr), _lib.ptr(self.col),
                                                 _lib.ptr(self.row_start), _lib.ptr(ranks), C.c_int64(first), C.c_int64(count),
                                                 _lib.ptr(out), _lib.stream_ptr())
        _lib.check(rc, "tlc_complement_pairs")
        return out


def near_pairs(index, hop, cap=None):
    """Non-adjacent pairs u <= v with d(u,v) <= hop (tlc_near_pairs) of a ComplementIndex: (pairs int32 CUDA [k,2], ranks int64
    CUDA [k]) with ranks = their numbers in the complement list.  Unordered."""
    import torch
    dev = index.rowptr.device
    cap = max(1 << 16, 64 * index.n_nodes) if cap is None else int(cap)
    with torch.cuda.device(dev):
        count = torch.zeros(1, dtype=torch.int64, device=dev)
        while True:
            ranks = torch.empty(cap, dtype=torch.int64, device=dev)
            pairs = torch.empty((cap, 2), dtype=torch.int32, device=dev)
            count.zero_()
            rc = _lib.lib().tlc_near_pairs(C.c_int32(index.n_nodes), _lib.ptr(index.rowptr), _lib.ptr(index.col),
                                           _lib.ptr(index.row_start), C.c_int(hop), C.c_int64(cap), _lib.ptr(count), _lib.ptr(ranks),
                                           _lib.ptr(pairs), _lib.stream_ptr())
            _lib.check(rc, "tlc_near_pairs")
            k = int(count.item())
            if k <= cap:
                return pairs[:k], ranks[:k]
            del ranks, pairs
            cap = k + 1024


@_lib.on_device_of
def select_rows(pi, status, index_base, count, out_idx, out_status, out_rows, hist=None, keep_failed=False):
    """Append the non-zero rows of an image block (keep_failed: and the zero rows with status != 0) to a sparse store and add
    the block's status bytes to `hist` (int64 CUDA [8]) -- tlc_select_rows.  count: int64 CUDA scalar tensor the caller zeroed
    (read it after synchronising; it may exceed the capacity)."""
    rc = _lib.lib().tlc_select_rows(C.c_int64(pi.shape[0]), C.c_int32(pi.shape[1]), _lib.ptr(pi), _lib.ptr(status),
                                    C.c_int64(index_base), C.c_int64(out_idx.shape[0]), C.c_uint32(1 if keep_failed else 0),
                                    _lib.ptr(count), _lib.ptr(hist), _lib.ptr(out_idx), _lib.ptr(out_status), _lib.ptr(out_rows),
                                    _lib.stream_ptr())
    _lib.check(rc, "tlc_select_rows")


def ollivier_ricci_sinkhorn(rowptr, col, edges, alpha=0.5, reg=0.1, max_iter=1000, stop_thr=1e-9, device=None, want_iters=False):
    """Ollivier-Ricci curvature of the given edges with the Sinkhorn transport distance -- GraphRicciCurvature's
    OllivierRicci(G, alpha, method="Sinkhorn") as loaddatas.py:105-123 calls it (tlc_ollivier_ricci_sinkhorn).

    rowptr/col: numpy CSR of the symmetric, loop-free, unit-weight graph (columns ascending); edges: int [E,2] adjacent pairs.
    Returns float64 numpy [E] (and the iteration counts)."""
    torch = _lib.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
    rowptr = np.ascontiguousarray(rowptr, dtype=np.int32)
    col = np.ascontiguousarray(col, dtype=np.int32)
    edges = np.ascontiguousarray(edges, dtype=np.int32).reshape(-1, 2)
    E, n = len(edges), len(rowptr) - 1
    if E == 0:
        return (np.zeros(0), np.zeros(0, dtype=np.int32)) if want_iters else np.zeros(0)
    deg = np.diff(rowptr).astype(np.int64)
    ok = (edges >= 0).all(1) & (edges < n).all(1)
    if not ok.all():
        raise ValueError("ollivier_ricci_sinkhorn: edge endpoint out of range")
    # the 0/1/2/3 hop-distance rule of the kernel holds for ADJACENT pairs only: every edge must be in the CSR (self pairs get 0)
    keys = np.repeat(np.arange(n, dtype=np.int64), deg) * n + col.astype(np.int64)
    want = edges[:, 0].astype(np.int64) * n + edges[:, 1].astype(np.int64)
    loops = edges[:, 0] == edges[:, 1]
    pos = np.searchsorted(keys, want)
    found = (pos < len(keys)) & (keys[np.minimum(pos, max(len(keys) - 1, 0))] == want) if len(keys) else np.zeros(E, dtype=bool)
    if not (found | loops).all():
        raise ValueError("ollivier_ricci_sinkhorn: every pair must be an edge of the CSR (columns ascending)")
    na = np.where(ok, deg[np.clip(edges[:, 0], 0, n - 1)] + 1, 1)
    nb = np.where(ok, deg[np.clip(edges[:, 1], 0, n - 1)] + 1, 1)
    prod = na * nb
    big = (prod > 8192) | (na + nb > 256)                         # what the wavefront kernel leaves to the workgroup kernel
    max_support = int(max(2, (na + nb).max()))
    max_product = int(prod[big].max()) if big.any() else 16
    slots = int(min(max(int(big.sum()), 1), 512))
    work_bytes = 16 + ((4 * E + 15) // 16) * 16 + slots * ((((max_product + 3) // 4 + 15) // 16) * 16)
    with torch.cuda.device(dev):
        d_rowptr, d_col = torch.from_numpy(rowptr).to(dev), torch.from_numpy(col).to(dev)
        d_edges = torch.from_numpy(edges).to(dev)
        kappa = torch.empty(E, dtype=torch.float64, device=dev)
        iters = torch.empty(E, dtype=torch.int32, device=dev)
        work = torch.empty(work_bytes, dtype=torch.uint8, device=dev)
        rc = _lib.lib().tlc_ollivier_ricci_sinkhorn(C.c_int32(n), _lib.ptr(d_rowptr), _lib.ptr(d_col), C.c_int64(E), _lib.ptr(d_edges),
                                                    C.c_double(alpha), C.c_double(reg), C.c_int32(max_iter), C.c_double(stop_thr),
                                                    _lib.ptr(kappa), _lib.ptr(iters), _lib.ptr(work), C.c_int64(work_bytes),
                                                    C.c_int32(max_support), C.c_int64(max_product), _lib.stream_ptr())
        _lib.check(rc, "tlc_ollivier_ricci_sinkhorn")
        out = kappa.cpu().numpy()
        it = iters.cpu().numpy()
    if np.isnan(out).any():
        raise _lib.TlcError("tlc_ollivier_ricci_sinkhorn: an edge exceeded the workspace (max_support / max_product)")
    return (out, it) if want_iters else out


def otd_lds_codes(max_support):
    """How many 2-bit hop codes the workgroup kernel of tlc_ollivier_ricci_otd keeps in LDS for a batch with this max_support (a larger
    support matrix has its codes in the workspace slot): what 12 bytes per support entry and the control block leave of TLC_OTD_LDS_BYTES."""
    return 4 * max(0, _lib.OTD_LDS_BYTES - ((12 * int(max_support) + 15) // 16) * 16 - 32)


def _otd_fraction(alpha):
    from fractions import Fraction
    try:
        fr = Fraction(alpha).limit_denominator(1024)
    except (TypeError, ValueError, OverflowError):
        raise ValueError("ollivier_ricci_otd: alpha must be a number")
    if fr != Fraction(alpha) or not 0 <= fr <= 1:
        raise ValueError("ollivier_ricci_otd: alpha must be exactly p/q with 0 <= p <= q <= 1024 (the computation is integer); "
                         "got %r" % (alpha,))
    return fr.numerator, fr.denominator


def ollivier_ricci_otd(rowptr, col, edges, alpha=0.5, device=None, want_cost=False, max_product=None):
    """Ollivier-Ricci curvature of the given edges with the EXACT transport distance -- GraphRicciCurvature's
    OllivierRicci(G, alpha, method="OTD") (POT's emd2) as pipelines_GIN.py:79 calls it (tlc_ollivier_ricci_otd).  Integer up to one
    fp64 division: kappa = 1.0 - W / D with W the minimum cost of the transportation problem scaled by D = q * deg(s) * deg(t),
    alpha = p / q.  Bit-identical from run to run, independent of the batch and of an edge's orientation.

    rowptr/col: numpy CSR of the symmetric, loop-free, unit-weight graph (columns ascending); edges: int [E,2] adjacent pairs.
    alpha: a float, Fraction or int that is exactly p/q with q <= 1024 (0.5, 0.25, Fraction(1, 3); 0.3 is not) -- ValueError otherwise.
    Returns float64 numpy [E]; want_cost: (kappa, W int64 [E], D int64 [E]).  max_product (testing): workspace sized for hub edges
    up to this many support pairs only; an edge beyond it comes back NaN with W = -1 instead of raising.
    Not reproduced: the library's nbr_topk cut of neighbourhoods above 3 000, weighted graphs, directed graphs."""
    num, den = _otd_fraction(alpha)
    torch = _lib.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
    rowptr = np.ascontiguousarray(rowptr, dtype=np.int32)
    col = np.ascontiguousarray(col, dtype=np.int32)
    edges = np.ascontiguousarray(edges, dtype=np.int32).reshape(-1, 2)
    E, n = len(edges), len(rowptr) - 1
    if E == 0:
        return (np.zeros(0), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)) if want_cost else np.zeros(0)
    deg = np.diff(rowptr).astype(np.int64)
    ok = (edges >= 0).all(1) & (edges < n).all(1)
    if not ok.all():
        raise ValueError("ollivier_ricci_otd: edge endpoint out of range")
    # the 0/1/2/3 hop-distance rule of the kernel holds for ADJACENT pairs only: every edge must be in the CSR (self pairs get 0)
    keys = np.repeat(np.arange(n, dtype=np.int64), deg) * n + col.astype(np.int64)
    want = edges[:, 0].astype(np.int64) * n + edges[:, 1].astype(np.int64)
    loops = edges[:, 0] == edges[:, 1]
    pos = np.searchsorted(keys, want)
    found = (pos < len(keys)) & (keys[np.minimum(pos, max(len(keys) - 1, 0))] == want) if len(keys) else np.zeros(E, dtype=bool)
    if not (found | loops).all():
        raise ValueError("ollivier_ricci_otd: every pair must be an edge of the CSR (columns ascending)")
    ds, dt = deg[edges[:, 0]], deg[edges[:, 1]]
    na, nb = ds + 1, dt + 1
    prod = na * nb
    big = ((prod > _lib.OTD_WAVE_PRODUCT) | (na + nb > _lib.OTD_WAVE_SUPPORT) | (den * ds * dt > _lib.OTD_WAVE_DENOM)) & ~loops
    max_support = int(max(2, (na + nb)[~loops].max())) if (~loops).any() else 2
    if max_support > _lib.OTD_MAX_SUPPORT:
        raise _lib.TlcError("ollivier_ricci_otd: an edge with deg(s) + deg(t) + 2 = %d > %d (the LDS of a workgroup)" % (max_support, _lib.OTD_MAX_SUPPORT))
    strict = max_product is None
    if strict:
        max_product = int(prod[big].max()) if big.any() else 16
    # tlc_ollivier_ricci_otd_work_bytes sizes for min(E, 32) hub edges in flight; here: one slot per hub edge, up to one per
    # compute unit (256) and 1 GiB in all
    need1 = C.c_int64(0)
    _lib.check(_lib.lib().tlc_ollivier_ricci_otd_work_bytes(C.c_int64(1), C.c_int32(max_support), C.c_int64(int(max_product)), C.byref(need1)),
               "tlc_ollivier_ricci_otd_work_bytes")
    slot = need1.value - 32                                             # 16 (counter) + 16 (a list of one edge) + one slot
    slots = max(1, min(int(big.sum()), 256, (1 << 30) // slot))
    work_bytes = 16 + ((4 * E + 15) // 16) * 16 + slots * slot
    with torch.cuda.device(dev):
        d_rowptr, d_col = torch.from_numpy(rowptr).to(dev), torch.from_numpy(col).to(dev)
        d_edges = torch.from_numpy(edges).to(dev)
        kappa = torch.empty(E, dtype=torch.float64, device=dev)
        cost = torch.empty(E, dtype=torch.int64, device=dev)
        denom = torch.empty(E, dtype=torch.int64, device=dev)
        work = torch.empty(work_bytes, dtype=torch.uint8, device=dev)
        rc = _lib.lib().tlc_ollivier_ricci_otd(C.c_int32(n), _lib.ptr(d_rowptr), _lib.ptr(d_col), C.c_int64(E), _lib.ptr(d_edges),
                                               C.c_int32(num), C.c_int32(den), _lib.ptr(kappa), _lib.ptr(cost), _lib.ptr(denom),
                                               _lib.ptr(work), C.c_int64(work_bytes), C.c_int32(max_support), C.c_int64(int(max_product)),
                                               _lib.stream_ptr())
        _lib.check(rc, "tlc_ollivier_ricci_otd")
        out, w, d = kappa.cpu().numpy(), cost.cpu().numpy(), denom.cpu().numpy()
    if strict and np.isnan(out).any():
        raise _lib.TlcError("tlc_ollivier_ricci_otd: an edge exceeded the workspace or the solver's bound (edge %d)" % int(np.flatnonzero(np.isnan(out))[0]))
    return (out, w, d) if want_cost else out


DIST_NORMS = {"max": 0, "max_eps": _lib.NORM_EPS, "none": _lib.NO_NORM}
DIST_STATUS_NAMES = {_lib.ST_DISCONNECTED: "ST_DISCONNECTED (a node root 0 does not reach, without unreachable_100)",
                     _lib.ST_ZERO_RANGE: "ST_ZERO_RANGE (all values 0 under norm='max')",
                     _lib.ST_BAD_INPUT: "ST_BAD_INPUT (offsets, an id or a root out of range, a loop, a repeated edge, a weight not finite and > 0)"}


def dist_filtration_flags(descriptor="sum", norm="max", include_roots=False, unreachable_100=False):
    """The flag word of tlc_dist_filtration for a descriptor of DESCRIPTOR_FLAG and a norm of DIST_NORMS."""
    if descriptor not in _lib.DESCRIPTOR_FLAG or norm not in DIST_NORMS:
        raise ValueError("dist_filtration: descriptor one of %s and norm one of %s, not %r / %r"
                         % (tuple(_lib.DESCRIPTOR_FLAG), tuple(DIST_NORMS), descriptor, norm))
    return (_lib.DESCRIPTOR_FLAG[descriptor] | DIST_NORMS[norm] | (_lib.INCLUDE_ROOTS if include_roots else 0)
            | (_lib.UNREACHABLE_100 if unreachable_100 else 0))


def dist_filtration_work_bytes(n_graphs, total_nodes, total_edges, vjp=False):
    """Least bytes of workspace of tlc_dist_filtration (vjp=True: of tlc_dist_filtration_vjp) for a batch of these totals: host
    arithmetic, no device."""
    need = C.c_int64(0)
    fn = _lib.lib().tlc_dist_filtration_vjp_work_bytes if vjp else _lib.lib().tlc_dist_filtration_work_bytes
    _lib.check(fn(C.c_int64(int(n_graphs)), C.c_int64(int(total_nodes)), C.c_int64(int(total_edges)), C.byref(need)),
               "tlc_dist_filtration_work_bytes")
    return need.value


def _dist_raise(what, status):
    bad = status.nonzero().flatten().tolist()
    if bad:
        codes = status[bad].tolist()
        raise RuntimeError("%s: graph(s) %s are not computed: status %s (%s)"
                           % (what, bad[:16], codes[:16], "; ".join("%d = %s" % (c, DIST_STATUS_NAMES.get(c, "?")) for c in sorted(set(codes)))))


def _dist_work(work, need, dev, torch):
    """A 256-byte aligned view of at least `need` bytes: of the caller's uint8 tensor, or of a fresh one."""
    if work is None:
        work = torch.empty(need + 256, dtype=torch.uint8, device=dev)
    off = (-work.data_ptr()) % 256
    return work[off:]


@_lib.on_device_of
def dist_filtration(node_offs, edge_offs, edges, w, roots, descriptor="sum", norm="max", include_roots=False, unreachable_100=False,
                    work=None, total_nodes=None, check=True):
    """The distance filtration of a packed batch on the device (tlc_dist_filtration; `filtration.build_fv` /
    `ricci_filtration.build_fv` of the reference bit for bit): per node the weighted shortest-path distance to the root(s) of its graph.

    node_offs / edge_offs int64[B + 1], edges int32[sum m, 2] local ids (each undirected edge once), w float64[sum m] > 0, roots
    int32[B, 2] local ids (column 1 == -1: one root): CUDA tensors.  descriptor 'sum' / 'min' / 'max' over the two distances; norm 'max'
    (/ the maximum), 'max_eps' (/ (the maximum + 1e-10)) or 'none'; unreachable_100: an unreachable root costs 100 instead of
    ST_DISCONNECTED; include_roots: TLC_INCLUDE_ROOTS, accepted for flag parity with the vicinity pipeline, no effect on a packed graph.
    work: a uint8 CUDA tensor of at least `dist_filtration_work_bytes` (+ 255 for alignment) bytes, or None.
    Returns (f float64[sum n], status uint8[B], parent int32[2, sum n]: the tree of include/tlcgnn.h).  check=True raises RuntimeError
    naming the graphs whose status is not ST_OK (their slice of f holds NaN); check=False returns the status for the caller to read."""
    torch = _lib.require_gpu()
    dev = node_offs.device
    flags = dist_filtration_flags(descriptor, norm, include_roots, unreachable_100)
    B = node_offs.numel() - 1
    tot_m = int(edges.shape[0])
    tot_n = int(total_nodes) if total_nodes is not None else (int(node_offs[-1]) if B > 0 else 0)
    f = torch.full((tot_n,), float("nan"), dtype=torch.float64, device=dev)
    parent = torch.full((2, tot_n), -1, dtype=torch.int32, device=dev)
    status = torch.zeros(max(B, 1), dtype=torch.uint8, device=dev)[:B]
    if B > 0:
        need = dist_filtration_work_bytes(B, tot_n, tot_m)
        if work is None and (tot_n > _lib.DIST_WG_NMAX or tot_m > _lib.DIST_WG_MMAX):
            # room for more fallback searches of the whole-device class in flight: up to 255 further slices of 8 B per node, 256 MiB at the most
            need += min(255 * (((8 * tot_n + 255) // 256) * 256), 1 << 28)
        wk = _dist_work(work, need, dev, torch)
        rc = _lib.lib().tlc_dist_filtration(C.c_int64(B), _lib.ptr(node_offs.contiguous()), _lib.ptr(edge_offs.contiguous()),
                                            _lib.ptr(edges.contiguous()), _lib.ptr(w.contiguous()), _lib.ptr(roots.contiguous()),
                                            C.c_int64(tot_n), C.c_int64(tot_m), C.c_uint32(flags), _lib.ptr(f), _lib.ptr(status),
                                            _lib.ptr(parent), _lib.ptr(wk), C.c_int64(wk.numel()), _lib.stream_ptr())
        _lib.check(rc, "tlc_dist_filtration")
        if check:
            _dist_raise("dist_filtration", status)
    return f, status, parent


@_lib.on_device_of
def dist_filtration_vjp(node_offs, edge_offs, edges, w, roots, parent, grad_f, descriptor="sum", norm="max", include_roots=False,
                        unreachable_100=False, work=None, total_nodes=None, check=True):
    """d (sum grad_f . f) / d w of `dist_filtration` (tlc_dist_filtration_vjp: the specification in include/tlcgnn.h): the same inputs
    and options, `parent` of that forward, grad_f float64[sum n] -> (grad_w float64[sum m], status uint8[B]); zeros for an edge off both
    trees.  Under ties among path lengths the tree is a convention, not a derivative."""
    torch = _lib.require_gpu()
    dev = node_offs.device
    flags = dist_filtration_flags(descriptor, norm, include_roots, unreachable_100)
    B = node_offs.numel() - 1
    tot_m = int(edges.shape[0])
    tot_n = int(total_nodes) if total_nodes is not None else (int(node_offs[-1]) if B > 0 else 0)
    gw = torch.full((tot_m,), float("nan"), dtype=torch.float64, device=dev)
    status = torch.zeros(max(B, 1), dtype=torch.uint8, device=dev)[:B]
    if B > 0:
        need = dist_filtration_work_bytes(B, tot_n, tot_m, vjp=True)
        wk = _dist_work(work, need, dev, torch)
        rc = _lib.lib().tlc_dist_filtration_vjp(C.c_int64(B), _lib.ptr(node_offs.contiguous()), _lib.ptr(edge_offs.contiguous()),
                                                _lib.ptr(edges.contiguous()), _lib.ptr(w.contiguous()), _lib.ptr(roots.contiguous()),
                                                C.c_int64(tot_n), C.c_int64(tot_m), C.c_uint32(flags), None, _lib.ptr(parent.contiguous()),
                                                _lib.ptr(grad_f.contiguous()), _lib.ptr(gw), _lib.ptr(status), _lib.ptr(wk),
                                                C.c_int64(wk.numel()), _lib.stream_ptr())
        _lib.check(rc, "tlc_dist_filtration_vjp")
        if check:
            _dist_raise("dist_filtration_vjp", status)
    return gw, status


# ---- vicinity images differentiable in the graph's edge weights (csrc/vic_grad.hip; topo.VicinityImages) -------------------------------
@_lib.on_device_of
def packed_edge_lookup(graph_edges, node_ptr, edge_ptr, ids, edges, pairs=None, one_root=False):
    """Which edge of the graph is every packed vicinity edge, and where are a pair's ends in their vicinity (tlc_packed_edge_lookup).
    graph_edges int32[M, 2]: lo < hi, ascending by (lo, hi); the packed batch of `Vicinities.batch` / `pack_vicinities` /
    `vicinity_filtration(offsets=...)`: node_ptr / edge_ptr int64[B + 1], ids int64 or int32 [sum n] global ids, edges int32[sum m, 2]
    local ids; pairs int32[B, 2] global ids or None.  -> (eid int32[sum m], roots int32[B, 2] or None, status uint8[B]); one_root:
    roots[:, 1] = -1.  A vicinity with an edge outside the list or a missing end: ST_BAD_INPUT, its eid and roots -1."""
    torch = _lib.require_gpu()
    dev = node_ptr.device
    B = node_ptr.numel() - 1
    assert graph_edges.dtype == torch.int32 and edges.dtype == torch.int32 and ids.dtype in (torch.int32, torch.int64)
    assert pairs is None or (pairs.dtype == torch.int32 and tuple(pairs.shape) == (B, 2))
    tot_n, tot_m = int(ids.numel()), int(edges.shape[0])
    eid = torch.full((max(tot_m, 1),), -1, dtype=torch.int32, device=dev)
    roots = torch.full((max(B, 1), 2), -1, dtype=torch.int32, device=dev) if pairs is not None else None
    status = torch.zeros(max(B, 1), dtype=torch.uint8, device=dev)
    rc = _lib.lib().tlc_packed_edge_lookup(C.c_int64(int(graph_edges.shape[0])), _lib.ptr(graph_edges.contiguous()), C.c_int64(B),
                                           _lib.ptr(node_ptr.contiguous()), _lib.ptr(edge_ptr.contiguous()), _lib.ptr(ids.contiguous()),
                                           C.c_int32(int(ids.dtype == torch.int64)), _lib.ptr(edges.contiguous()), C.c_int64(tot_n),
                                           C.c_int64(tot_m), _lib.ptr(pairs.contiguous()) if pairs is not None else None,
                                           C.c_int32(int(bool(one_root))), _lib.ptr(eid), _lib.ptr(roots), _lib.ptr(status), _lib.stream_ptr())
    _lib.check(rc, "tlc_packed_edge_lookup")
    return eid[:tot_m], (roots[:B] if roots is not None else None), status[:B]


def segment_index_work_bytes(n_items, n_keys):
    need = C.c_int64(0)
    _lib.check(_lib.lib().tlc_segment_index_work_bytes(C.c_int64(int(n_items)), C.c_int64(int(n_keys)), C.byref(need)),
               "tlc_segment_index_work_bytes")
    return need.value


def segment_sum_work_bytes(n_keys):
    need = C.c_int64(0)
    _lib.check(_lib.lib().tlc_segment_sum_work_bytes(C.c_int64(int(n_keys)), C.byref(need)), "tlc_segment_sum_work_bytes")
    return need.value


@_lib.on_device_of
def segment_index(key, n_keys, work=None):
    """The items of every key (tlc_segment_index, one-off): key int32[n_items], keys outside 0 .. n_keys-1 skipped -> (seg_ptr
    int64[n_keys + 1], seg_pos int32[n_items]): key k's items are seg_pos[seg_ptr[k]:seg_ptr[k + 1]], ascending."""
    torch = _lib.require_gpu()
    assert key.dtype == torch.int32 and key.dim() == 1
    dev, n = key.device, int(key.numel())
    seg_ptr = torch.empty(int(n_keys) + 1, dtype=torch.int64, device=dev)
    seg_pos = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    wk = _dist_work(work, segment_index_work_bytes(n, n_keys), dev, torch)
    rc = _lib.lib().tlc_segment_index(C.c_int64(n), _lib.ptr(key.contiguous()), C.c_int64(int(n_keys)), _lib.ptr(seg_ptr), _lib.ptr(seg_pos),
                                      _lib.ptr(wk), C.c_int64(wk.numel()), _lib.stream_ptr())
    _lib.check(rc, "tlc_segment_index")
    return seg_ptr, seg_pos[:n]


@_lib.on_device_of
def segment_sum(val, seg_ptr, seg_pos, work=None, out=None):
    """out[k] = the sum of val[seg_pos[j]] over key k's segment (tlc_segment_sum_f64): float64, in the order include/tlcgnn.h states,
    which depends on the segment's length alone -- the deterministic adjoint of the gather val = w[key]."""
    torch = _lib.require_gpu()
    assert val.dtype == torch.float64 and val.numel() == seg_pos.numel()
    dev, M = val.device, seg_ptr.numel() - 1
    if out is None:
        out = torch.empty(max(M, 1), dtype=torch.float64, device=dev)[:M]
    wk = _dist_work(work, segment_sum_work_bytes(M), dev, torch)
    rc = _lib.lib().tlc_segment_sum_f64(C.c_int64(M), _lib.ptr(seg_ptr.contiguous()), _lib.ptr(seg_pos.contiguous()), C.c_int64(int(val.numel())),
                                        _lib.ptr(val.contiguous()), _lib.ptr(out), _lib.ptr(wk), C.c_int64(wk.numel()), _lib.stream_ptr())
    _lib.check(rc, "tlc_segment_sum_f64")
    return out


@_lib.on_device_of
def lp_decode_bwd_pi(pairs, emb_pre, emb, pi, w1, b1, w2, b2, gprob):
    """d loss / d PI of `ops.lp_decode` (tlc_lp_decode_bwd_pi_f32): the arguments of `ops.lp_decode_bwd` -> float32[E, 25]."""
    torch = _lib.require_gpu()
    assert pairs.dtype == torch.int32 and pi.dtype == torch.float32
    E, n = pairs.shape[0], emb_pre.shape[0]
    pre, post, w1, b1, w2, b2, gprob = (t.detach().to(torch.float32).contiguous() for t in (emb_pre, emb, w1, b1, w2.reshape(-1), b2, gprob))
    pairs, pi = pairs.contiguous(), pi.contiguous()
    gpi = torch.empty((E, pi.shape[1]), dtype=torch.float32, device=post.device)
    rc = _lib.lib().tlc_lp_decode_bwd_pi_f32(C.c_int64(E), _lib.ptr(pairs), _lib.ptr(pre), _lib.ptr(post), C.c_int32(n), C.c_int32(pre.shape[1]),
                                             _lib.ptr(pi), C.c_int32(pi.shape[1]), _lib.ptr(w1), _lib.ptr(b1), _lib.ptr(w2), _lib.ptr(b2),
                                             _lib.ptr(gprob), _lib.ptr(gpi), _lib.stream_ptr())
    _lib.check(rc, "tlc_lp_decode_bwd_pi_f32")
    return gpi

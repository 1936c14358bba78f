"""GPU: pipelined image batches (tlc_pd_pi_batch_async) under workloads that change from batch to batch.

The headline number is measured on pipelined batches: chunks rotate over the handle's workspaces, a chunk's second half is deferred
behind the next chunk's first half, and the tier streams are shared between workspaces ("Who owns what").  A chunk that
read a region before writing it would get the previous chunk's values -- invisible whenever the previous batch was the same.  So here
every batch differs from the one before (size, hop, pairs), stream-ordered calls and caller-stream work sit between the submissions,
option poison fills every chunk's payload scratch with 7.25 first, and every output buffer must equal the stream-ordered call for the
same pairs on a separate, fresh handle -- bit for bit -- which itself is checked against the oracle once per distinct batch.

Two graphs: the PubMed-shaped one, and "hub + leaves + chords" components (tests/test_gpu_tiers.py) sized so that every list of a
chunk is reached: TINY, SMALL, MID, compact MEDIUM with and without >= 64 Pos edges (the front list of a pipelined chunk), MEDWIDE,
its divide and conquer (>= 320 Pos) and LARGE with >= 160 Pos (tlc_pd_dc_kernel).  The pairs of a batch are drawn from a fixed pool
per hop, so the oracle runs once per pool."""
import numpy as np
import pytest

from helpers import rel_err

pytestmark = pytest.mark.gpu


def hub_component(n, m, rs, base=0):
    """a hub, n - 1 leaves and m - (n - 1) distinct chords among the leaves; ids from `base` on; returns edges int64[m, 2]"""
    assert m >= n - 1 and m <= (n - 1) + (n - 1) * (n - 2) // 2
    e = set((0, k) for k in range(1, n))
    while len(e) < m:
        a, b = rs.randint(1, n, size=2)
        if a != b:
            e.add((min(a, b), max(a, b)))
    return np.array(sorted(e), dtype=np.int64) + base


# (nodes, edges) of the hub graph's components, at hop 2 for a (hub, leaf) pair: TINY; SMALL; MID; compact MEDIUM with 130 Pos edges
# (the front list of a pipelined chunk, the many-Pos list of a chunk on its own); compact MEDIUM with 31; MEDWIDE (450 nodes);
# MEDWIDE with 330 Pos (divide and conquer); LARGE with 200 Pos (divide and conquer)
HUB_SHAPES = [(12, 16), (50, 90), (100, 150), (300, 429), (300, 330), (450, 600), (301, 630), (601, 800)]

# (pairs, hop) of the mixed workload: around the early pass's cut (4 096 pairs), small and large, in runs of one hop -- hop 2, 1, 3.
# (A hop change rebuilds the ball lists and bounds, which first drains every chunk in flight (quiesce); inside a run the chunks overlap:
# a second half is submitted behind the next chunk's first half, every workspace holds a chunk.)
BATCHES = [(4096, 2), (300, 2), (20000, 2), (17, 2), (4097, 2), (9000, 2), (4095, 2),
           (17, 1), (4097, 1), (300, 1), (20000, 1), (4095, 1), (9000, 1), (4096, 1),
           (9000, 3), (4095, 3), (300, 3), (17, 3), (4096, 3), (20000, 3)]
SYNC_AT = {3, 10, 16}           # ... where the handle under test also runs the batch stream-ordered (twice), asynchronous batches in flight
JOIN_AT = {5, 13, 19}           # ... and where the caller's stream joins the asynchronous batches and their buffers are checked
EARLY_ARENA_BYTES = 256 * 2 * 4096 * 8      # TLC_EARLY_SLOTS slots of 2 x TLC_L_MMAX float64 weights


def arena_floor_bytes(n_pairs):
    """the least a chunk's arena holds (front_prepare): one 4 096-entry region per extraction workgroup -- at least min(n, 256) of the
    main launch (one per scratch slot, >= one per CU) and the early pass's 256 -- and a bump area of max(32 n, 2^20) entries"""
    return 8 * ((min(n_pairs, 256) + 256) * 4096 + max(32 * n_pairs, 1 << 20))


OPTION_SETS = [{}, {"poison": 1}, {"spec_cap": 8}, {"tiny": 0}, {"mh_front_pos": 0}, {"main_beside_early": 0}, {"dc_force_fail": 1},
               {"x_arena": 64}]


class Workload:
    """A graph, a pool of pairs per hop, the seeded batches drawn from the pools, and (lazily) the oracle's rows of each pool."""

    def __init__(self, name, n, edges, kappa, pool_sizes, seed, candidates=None):
        """pools: pool_sizes[hop] pairs drawn from `candidates` (default: the edges), either way round"""
        from tlc_gnn_amd import synth
        self.name = name
        self.rowptr, self.col, self.w = synth.edges_to_csr(n, edges, kappa)
        rs = np.random.RandomState(seed)
        cand = edges if candidates is None else candidates
        self.pools = {}
        for hop, k in pool_sizes.items():
            p = cand[rs.permutation(len(cand))[:k]]
            flip = rs.rand(len(p)) < 0.5
            p[flip] = p[flip][:, ::-1]
            # (and pairs without a vicinity of their own: a self pair, an id out of range, a negative id)
            self.pools[hop] = np.ascontiguousarray(np.concatenate([p, [[0, 0], [n + 5, 1], [-1, 2]]]), dtype=np.int32)
        self.index = [rs.randint(len(self.pools[hop]), size=size) for size, hop in BATCHES]
        self.batches = [self.pools[hop][ix] for ix, (_, hop) in zip(self.index, BATCHES)]
        self._oracle = {}
        self.refs = {}              # option set -> [(rows, status)] of the stream-ordered calls on a fresh handle

    def oracle(self, i):
        from oracle import oracle
        hop = BATCHES[i][1]
        if hop not in self._oracle:
            ref, rst, _ = oracle.pd_pi_batch(self.rowptr, self.col, self.w, self.pools[hop], hop, n_threads=0)
            self._oracle[hop] = (ref, rst)
        ref, rst = self._oracle[hop]
        return ref[self.index[i]], rst[self.index[i]]

    def handle(self, opts):
        from tlc_gnn_amd import engine
        g = engine.DeviceGraph(self.rowptr, self.col, self.w)
        for k, v in opts.items():
            g.set_option(k, v)
        return g


def _hub_workload():
    rs = np.random.RandomState(2024)
    comps, base = [], 0
    for n, m in HUB_SHAPES:
        comps.append(hub_component(n, m, rs, base))
        base += n
    e = np.concatenate(comps)
    # the pool: for every component up to 40 (hub, leaf) pairs (sorted, the hub's edges come first) and 12 chords
    cand = np.concatenate([c[:min(n - 1, 40)] for (n, _), c in zip(HUB_SHAPES, comps)] +
                          [c[n - 1:][:12] for (n, _), c in zip(HUB_SHAPES, comps)])
    k = len(cand)
    return Workload("hub", base, e, rs.uniform(-0.5, 0.9, size=len(e)), {1: k, 2: k, 3: k}, seed=7, candidates=cand)


def _pubmed_workload():
    from tlc_gnn_amd import synth
    n, edges, kappa, _, _ = synth.shaped_graph("PubMed", scale=0.3)
    # (the oracle's cost grows fast with the hop: 2 ms per pair at hop 3 on one core)
    return Workload("PubMed", n, edges, kappa, {1: len(edges), 2: 4000, 3: 400}, seed=11)


_WORKLOADS = {}


@pytest.fixture(scope="module")
def workloads():
    if not _WORKLOADS:
        _WORKLOADS["hub"] = _hub_workload()
        _WORKLOADS["PubMed"] = _pubmed_workload()
    return _WORKLOADS


def _key(opts):
    return tuple(sorted(opts.items()))


def _reference(wl, opts):
    """The stream-ordered rows of every batch on a fresh handle with the same options (poison aside): each batch twice in a row and the
    second call kept -- a chunk on its own sizes its speculative launch, divide and conquer included, from the previous chunk on its
    workspace, and the second call's previous chunk is the same batch.  With the default options each distinct batch is also checked
    against the oracle: status bytes equal, the same zero entries, images within 1e-8 relative."""
    import torch
    ref_opts = {k: v for k, v in opts.items() if k != "poison"}
    key = _key(ref_opts)
    if key in wl.refs:
        return wl.refs[key]
    g = wl.handle(ref_opts)
    rows = []
    for i, pairs in enumerate(wl.batches):
        dev = torch.as_tensor(pairs).cuda()
        g.pd_pi_batch(dev, BATCHES[i][1])
        out, st = g.pd_pi_batch(dev, BATCHES[i][1])
        torch.cuda.synchronize()
        rows.append((out, st))
        if not ref_opts:
            ref, rst = wl.oracle(i)
            o, s = out.cpu().numpy(), st.cpu().numpy()
            assert np.array_equal(s, rst), (wl.name, i)
            assert np.array_equal(o == 0, ref == 0), (wl.name, i)
            nz = ref != 0
            if nz.any():
                assert rel_err(o[nz], ref[nz]).max() < 1e-8, (wl.name, i)
    g.close()
    wl.refs[key] = rows
    return rows


def _compare(wl, what, i, out, st, want, want_st, tol):
    """equal rows and status bytes (tol = 0: bit for bit); else an AssertionError naming the configuration, the batch, the rows, their
    vicinity sizes and the largest difference"""
    import torch
    if tol == 0:
        ok = torch.equal(out, want) and torch.equal(st, want_st)
    else:
        ok = torch.equal(st, want_st) and float((out - want).abs().max()) <= tol * max(1.0, float(want.abs().max()))
    if ok:
        return
    bad = torch.nonzero((out != want).any(dim=1) | (st != want_st)).view(-1)
    g = wl.handle({})                                      # (the vicinity sizes of the batch: a stream-ordered call of its own)
    pairs = torch.as_tensor(wl.batches[i]).cuda()
    g.pd_pi_batch(pairs, BATCHES[i][1])
    nn, mm = g.sizes(len(pairs))
    g.close()
    idx = bad[:8].cpu().numpy()
    raise AssertionError("%s: %s batch %d (%d pairs, hop %d): %d rows differ; first %s  pairs %s  n %s  m2 %s  max |diff| %.3e  "
                         "status %s / %s" % (
                             wl.name, what, i, len(pairs), BATCHES[i][1], bad.numel(), idx.tolist(), wl.batches[i][idx].tolist(),
                             nn[idx].tolist(), mm[idx].tolist(), float((out - want).abs().max()), st[bad[:8]].tolist(),
                             want_st[bad[:8]].tolist()))


def _run_sequence(wl, g, opts, n_ws, seen):
    """The fixed sequence of BATCHES on handle g: asynchronous submissions, stream-ordered calls at SYNC_AT, caller-stream work between
    them (an allocation that is filled, a 64 MB copy), joins at JOIN_AT -- each joined buffer checked against the reference."""
    import torch
    refs = _reference(wl, opts)
    what = "n_ws %d options %s" % (n_ws, opts)
    tol = 1e-12 if "x_arena" in opts else 0         # (the FILL path of an overflowed arena orders tied keys its own way)
    src = torch.full((1 << 23,), 1.5, dtype=torch.float64, device="cuda")
    dst = torch.empty_like(src)
    dev_pairs = [torch.as_tensor(b).cuda() for b in wl.batches]   # (uploaded first: the submissions of a run follow one another closely)
    pending = []
    for i, (size, hop) in enumerate(BATCHES):
        pairs = dev_pairs[i]
        out = torch.full((size, 25), -3.0, dtype=torch.float64, device="cuda")
        st = torch.full((size,), 77, dtype=torch.uint8, device="cuda")
        g.pd_pi_batch(pairs, hop, out=out, status=st, async_=True)
        pending.append((i, out, st))
        junk = torch.empty((size, 2), dtype=torch.int32, device="cuda")
        junk.fill_(-(i + 1))
        dst.copy_(src)
        if i in SYNC_AT:
            want, want_st = refs[i]
            a, a_st = g.pd_pi_batch(pairs, hop)
            # (the first call's speculative launch is sized from whatever chunk ran on workspace 0 before: divide and conquer or the
            # serial walk for the wide MEDIUM-sized vicinities, 1e-12 apart)
            _compare(wl, what + " stream-ordered, first call", i, a, a_st, want, want_st, 1e-12)
            b, b_st = g.pd_pi_batch(pairs, hop)
            _compare(wl, what + " stream-ordered, second call", i, b, b_st, want, want_st, tol)
        if i in JOIN_AT:
            g.join()
            torch.cuda.synchronize()
            for k, o, s in pending:
                _compare(wl, what + " pipelined", k, o, s, refs[k][0], refs[k][1], tol)
            pending = []
            # (the last call's counts: the chunk the join submitted the second half of)
            tc = g.tier_counts()
            seen["medium_wide"] += tc["medium_wide"]
            seen["tiny"] += g.stats()["tier_tiny"]
            seen["dc_pipelined"] += g.dc_stats()[0]
            seen["front_list_last_call"] += g.front_list_count()
    assert not pending
    assert bool((dst == 1.5).all())


@pytest.mark.parametrize("n_ws", [2, 3, 4])
@pytest.mark.parametrize("graph", ["hub", "PubMed"])
def test_mixed_workload_matrix(workloads, graph, n_ws):
    """Every option set of OPTION_SETS on a fresh handle with n_ws workspaces in turn: every pipelined output buffer equals the
    stream-ordered call on a separate handle, bit for bit (arena overflow: 1e-12).  On the hub graph every scheduling branch is reached:
    MEDWIDE, the front list, divide and conquer in a pipelined chunk, TINY, the early pass, speculative list positions beyond their slots.
    And the chunks did overlap: every option set had n_ws workspaces holding a chunk at once, and second halves were submitted behind
    the next chunk's first half."""
    wl = workloads[graph]
    seen = dict(medium_wide=0, tiny=0, dc_pipelined=0, front_list_last_call=0, front_list=0, early=0, beyond_spec=0, deferred=0)
    n_sync = 2 * len(SYNC_AT)
    for opts in OPTION_SETS:
        g = wl.handle(opts)
        g.set_option("n_ws", n_ws)
        _run_sequence(wl, g, opts, n_ws, seen)
        cc = g.chunk_counters()
        assert cc["pipelined_chunks"] == len(BATCHES), (opts, cc)
        assert cc["max_busy_workspaces"] == n_ws, (opts, cc)
        if opts.get("poison"):
            # every chunk poisoned; the last one's bytes are its regions' sizes: the arena's weights (at least arena_floor_bytes of the
            # last batch), the early arena's (once a chunk with the early pass ran on the workspace) and the SMALL slots' (2 x 128
            # entries a pair, allocated only where the breadth-first kernels served a chunk)
            assert cc["poisoned_chunks"] == len(BATCHES) + n_sync, cc
            assert cc["poison_arena_bytes"] >= arena_floor_bytes(BATCHES[-1][0]) and cc["poison_arena_bytes"] % 8 == 0, cc
            assert cc["poison_early_bytes"] in (0, EARLY_ARENA_BYTES), cc
            assert cc["poison_small_bytes"] % (2 * 128 * 8) == 0, cc
            assert cc["poison_bytes"] >= cc["poisoned_chunks"] * 8 * (1 << 16), cc        # (the arena has at least 2^16 entries)
        else:
            assert cc["poisoned_chunks"] == 0 and cc["poison_bytes"] == 0, (opts, cc)
        if opts.get("mh_front_pos") == 0:
            assert cc["front_list"] == 0, cc
        seen["front_list"] += cc["front_list"]
        seen["early"] += cc["early_chunks"]
        seen["beyond_spec"] += cc["beyond_spec_slots"]
        seen["deferred"] += cc["deferred_second_halves"]
        g.close()
    assert seen["tiny"] > 0 and seen["early"] > 0 and seen["deferred"] > 0, seen
    if graph == "hub":
        for k in ("medium_wide", "front_list", "front_list_last_call", "dc_pipelined", "beyond_spec"):
            assert seen[k] > 0, (k, seen)


def test_poison_changes_no_row(workloads):
    """Option poison on one handle, off and on in turn: the same rows, bit for bit, pipelined and stream-ordered; each chunk fills
    its regions and nothing is filled with the option off.  The sizes are known from outside: three workspaces in turn take batches
    0 (4 096 pairs: the early pass), 1 (300 pairs: none -- that workspace never allocates an early arena) and 2 (20 000), so the early
    arena's weights are 16 MiB / 0 / 16 MiB; the extraction runs from the ball lists (no SMALL slots); the arena is at least
    arena_floor_bytes."""
    import torch
    wl = workloads["hub"]
    g = wl.handle({})
    res = {}
    batches = (0, 1, 2)
    assert [BATCHES[i] for i in batches] == [(4096, 2), (300, 2), (20000, 2)]
    for poison in (0, 1, 0, 1):
        g.set_option("poison", poison)
        before = g.chunk_counters()
        outs = []
        for i in batches:
            pairs = torch.as_tensor(wl.batches[i]).cuda()
            outs.append(g.pd_pi_batch(pairs, BATCHES[i][1], async_=True))
            after = g.chunk_counters()                      # (per chunk: the regions of the chunk just submitted)
            if poison:
                assert after["poisoned_chunks"] == before["poisoned_chunks"] + 1
                assert after["poison_early_bytes"] == (0 if i == 1 else EARLY_ARENA_BYTES), (i, after)
                assert after["poison_small_bytes"] == 0, (i, after)
                assert after["poison_arena_bytes"] >= arena_floor_bytes(BATCHES[i][0]), (i, after, arena_floor_bytes(BATCHES[i][0]))
                assert after["poison_bytes"] - before["poison_bytes"] == (
                    after["poison_arena_bytes"] + after["poison_early_bytes"] + after["poison_small_bytes"])
            else:
                assert after["poisoned_chunks"] == before["poisoned_chunks"] and after["poison_bytes"] == before["poison_bytes"]
            before = after
        g.join()
        pairs = torch.as_tensor(wl.batches[1]).cuda()
        outs.append(g.pd_pi_batch(pairs, BATCHES[1][1]))
        torch.cuda.synchronize()
        if poison in res:
            for (a, a_st), (b, b_st) in zip(outs, res[poison]):
                assert torch.equal(a, b) and torch.equal(a_st, b_st)
        res[poison] = outs
    for (a, a_st), (b, b_st) in zip(res[0], res[1]):
        assert torch.equal(a, b) and torch.equal(a_st, b_st)
    g.close()


def test_front_list_switch_and_count(workloads):
    """Option mh_front_pos: the pipelined chunk's compact MEDIUM vicinities with >= 64 Pos edges (default) stand in front of their
    list and are counted (tlc_debug_chunk_counters) -- exactly the compact MEDIUM-sized vicinities with that many Pos edges; at 0 there is
    no front list, at 131 it is empty -- the same rows each way, and a chunk on its own never has one."""
    import torch
    wl = workloads["hub"]
    i = 5                                                   # (9 000 pairs at hop 2)
    assert BATCHES[i] == (9000, 2)
    pairs = torch.as_tensor(wl.batches[i]).cuda()
    hop = BATCHES[i][1]
    g = wl.handle({})
    want, want_st = g.pd_pi_batch(pairs, hop)
    assert g.front_list_count() == 0                        # (a chunk on its own: the many-Pos list instead)
    n, m2 = g.sizes(len(pairs))
    m = m2 // 2
    compact_medium = (n > 0) & ~((n <= 128) & (m <= 256)) & (n <= 384) & (m <= 512)
    assert int((compact_medium & (m - n + 1 == 130)).sum()) > 0
    for value in (64, 0, 131, 130, 64):
        expect = int((compact_medium & (m - n + 1 >= value)).sum()) if value > 0 else 0
        g.set_option("mh_front_pos", value)
        out, st = g.pd_pi_batch(pairs, hop, async_=True)
        g.join()
        torch.cuda.synchronize()
        assert g.front_list_count() == expect, (value, g.front_list_count(), expect)
        assert (expect > 0) == (value in (64, 130)), (value, expect)
        assert torch.equal(out, want) and torch.equal(st, want_st), value
    g.close()


def test_inputs_dropped_by_the_caller_after_submission(workloads):
    """Eight asynchronous batches without a join -- more than the engine keeps alive (six) and than the handle has workspaces (four):
    each batch's pairs tensor is a temporary the caller drops at once, and between the submissions same-sized tensors are allocated
    and filled on the caller's stream (the caching allocator hands freed blocks out again).  After the join every output equals the
    reference.  (All of one hop: a hop change would drain the chunks in flight, and with them the uses of the freed blocks.)"""
    import torch
    wl = workloads["hub"]
    refs = _reference(wl, {})
    g = wl.handle({})
    g.set_option("n_ws", 4)
    order = [1, 0, 2, 3, 4, 5, 6, 3]
    assert len(set(BATCHES[i][1] for i in order)) == 1
    outs = []
    keep = []
    for i in order:
        size, hop = BATCHES[i]
        outs.append((i,) + g.pd_pi_batch(torch.as_tensor(wl.batches[i]).cuda(), hop, async_=True))
        for _ in range(3):
            t = torch.empty((size, 2), dtype=torch.int32, device="cuda")
            t.fill_(-7)
            keep.append(t)
    g.join()
    torch.cuda.synchronize()
    for i, o, s in outs:
        _compare(wl, "inputs dropped", i, o, s, refs[i][0], refs[i][1], 0)
    assert g.chunk_counters()["max_busy_workspaces"] == 4
    assert all(bool((t == -7).all()) for t in keep)
    g.close()

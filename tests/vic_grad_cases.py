"""Numpy restatements of csrc/vic_grad.hip (include/tlcgnn.h): the packed-edge lookup, the segment index, the segment sum in exactly the
header's order, and the decoder's d PI in float32; and the data recipe of test_gpu_lp_train.test_decode_backward_matches_autograd_f64.
No GPU, no torch."""
import numpy as np

ST_OK, ST_BAD_INPUT = 0, 7
LANE_MAX, WAVE_MAX, WG_THREADS = 16, 2048, 256                 # TLC_SEG_LANE_MAX, TLC_SEG_WAVE_MAX, the workgroup's threads


# ---- lookup ----------------------------------------------------------------------------------------------------------------------------
def lookup(graph_edges, node_ptr, edge_ptr, ids, edges, pairs=None, one_root=False):
    """-> (eid int32[sum m], roots int32[B, 2] or None, status uint8[B]): a Python loop over vicinities and their edges, dictionaries
    instead of binary searches."""
    index = {(int(a), int(b)): k for k, (a, b) in enumerate(np.asarray(graph_edges).reshape(-1, 2))}
    B = len(node_ptr) - 1
    eid = np.full(len(edges), -1, np.int32)
    roots = np.full((B, 2), -1, np.int32) if pairs is not None else None
    status = np.zeros(B, np.uint8)
    for g in range(B):
        a, b, ea, eb = int(node_ptr[g]), int(node_ptr[g + 1]), int(edge_ptr[g]), int(edge_ptr[g + 1])
        local = {int(v): k for k, v in enumerate(ids[a:b])}
        got, ok = [], True
        for x, y in edges[ea:eb]:
            k = -1
            if 0 <= x < b - a and 0 <= y < b - a:
                u, v = int(ids[a + x]), int(ids[a + y])
                k = index.get((min(u, v), max(u, v)), -1)
            got.append(k)
            ok &= k >= 0
        r = [-1, -1]
        if pairs is not None:
            r[0] = local.get(int(pairs[g, 0]), -1)
            r[1] = -1 if one_root else local.get(int(pairs[g, 1]), -1)
            ok &= r[0] >= 0 and (one_root or r[1] >= 0)
        if ok:
            eid[ea:eb] = got
            if roots is not None:
                roots[g] = r
        else:
            status[g] = ST_BAD_INPUT
    return eid, roots, status


def lookup_searchsorted(n_nodes, graph_edges, node_ptr, edge_ptr, ids, edges, pairs, one_root=False):
    """The formulation of tests/test_gpu_dist_filt.py:198-205 (every edge present, every end in its vicinity) -> (eid, roots)."""
    ge = np.asarray(graph_edges, np.int64)
    key = ge[:, 0] * n_nodes + ge[:, 1]
    order = np.argsort(key)
    B = len(node_ptr) - 1
    owner = np.repeat(np.arange(B), np.diff(edge_ptr))
    ga, gb = ids[node_ptr[owner] + edges[:, 0]], ids[node_ptr[owner] + edges[:, 1]]
    eid = order[np.searchsorted(key[order], np.minimum(ga, gb).astype(np.int64) * n_nodes + np.maximum(ga, gb))]
    roots = np.array([[np.searchsorted(ids[node_ptr[k]:node_ptr[k + 1]], pairs[k, 0]),
                       -1 if one_root else np.searchsorted(ids[node_ptr[k]:node_ptr[k + 1]], pairs[k, 1])] for k in range(B)], np.int32)
    return eid.astype(np.int32), roots.reshape(B, 2)


# ---- segment index and sum ---------------------------------------------------------------------------------------------------------------
def segment_index(key, n_keys):
    """-> (seg_ptr int64[n_keys + 1], seg_pos int32[len(key)]): the positions of every key ascending, the skipped items at the end"""
    key = np.asarray(key, np.int64)
    k = np.where((key < 0) | (key >= n_keys), n_keys, key)
    seg_pos = np.argsort(k, kind="stable").astype(np.int32)
    seg_ptr = np.searchsorted(k[seg_pos], np.arange(n_keys + 1), side="left").astype(np.int64)
    return seg_ptr, seg_pos


def _fold(p):
    """for d = 32, 16, 8, 4, 2, 1: p[l] = p[l] + p[l + d] for l < d -> p[0]"""
    p = np.array(p, np.float64)
    d = 32
    while d >= 1:
        p[:d] = p[:d] + p[d:2 * d]
        d //= 2
    return p[0]


def _strided(v, lanes):
    """p[l] = +0.0, then + v[l], v[l + lanes], ... in that order"""
    p = np.zeros(lanes, np.float64)
    for j0 in range(0, len(v), lanes):
        chunk = v[j0:j0 + lanes]
        p[:len(chunk)] = p[:len(chunk)] + chunk
    return p


def segment_sum_one(v):
    """The sum of one segment's values v (in segment order) in the header's order for its length."""
    v = np.asarray(v, np.float64)
    L = len(v)
    if L <= LANE_MAX:
        s = np.float64(0.0)
        for x in v:
            s = s + x
        return s
    if L <= WAVE_MAX:
        return _fold(_strided(v, 64))
    p = _strided(v, WG_THREADS)
    q = [_fold(p[64 * w:64 * w + 64]) for w in range(4)]
    return ((q[0] + q[1]) + q[2]) + q[3]


def segment_sum(val, seg_ptr, seg_pos):
    """Every segment in the header's order.  The lane class is stepped for all its segments at once (step j adds item j of the segments
    that have one: the same additions in the same order per segment); the longer ones go one by one through segment_sum_one."""
    val, seg_ptr = np.asarray(val, np.float64), np.asarray(seg_ptr, np.int64)
    L = np.diff(seg_ptr)
    out = np.zeros(len(L), np.float64)
    short = np.nonzero(L <= LANE_MAX)[0]
    s, a, Ls = np.zeros(len(short), np.float64), seg_ptr[short], L[short]
    for j in range(LANE_MAX):
        live = Ls > j
        s[live] = s[live] + val[seg_pos[a[live] + j]]
    out[short] = s
    for k in np.nonzero(L > LANE_MAX)[0]:
        out[k] = segment_sum_one(val[seg_pos[seg_ptr[k]:seg_ptr[k + 1]]])
    return out


def index_work_bytes(n_items, n_keys):
    """TlcSegmentIndexScratch: three u32 arrays, the radix histograms (256 ints per tile of 4 096 items) and 256 totals, each on 256 B"""
    up = lambda v: (v + 255) & ~255
    tiles = (n_items + 4095) // 4096
    return 3 * up(4 * n_items) + up(4 * 256 * tiles) + up(4 * 256)


def sum_work_bytes(n_keys):
    up = lambda v: (v + 255) & ~255
    return 256 + 2 * up(4 * n_keys)


# ---- the decoder ---------------------------------------------------------------------------------------------------------------------------
def decode_data():
    """The recipe of test_decode_backward_matches_autograd_f64: repeated pairs, u == v, zero images, |d| > 40 and d == 0."""
    rs = np.random.RandomState(11)
    n, E = 40, 700
    emb = rs.normal(0, 0.6, size=(n, 16)).astype(np.float32)
    emb[0] = 0.0
    emb[0, 0] = 1.0
    emb[1] = 0.0
    emb[1, 3] = -1.0
    emb[2:12] *= 0.2
    emb[12:] *= 3.0
    pairs = rs.randint(0, n, size=(E, 2)).astype(np.int32)
    pairs[:50] = pairs[50:100]
    pairs[100:130, 1] = pairs[100:130, 0]
    pi = rs.uniform(0, 0.3, size=(E, 25)).astype(np.float32)
    pi[100:110] = 0.0
    pi[200:260] *= 200.0
    w1 = (rs.normal(0, 1.0, size=(25, 41))).astype(np.float32)
    b1 = (rs.randint(0, 5, size=25) * 0.25).astype(np.float32)
    w2 = (rs.randint(-4, 5, size=(1, 25)) * 0.25).astype(np.float32)
    b2 = np.array([-(w2[0].astype(np.float64) @ b1.astype(np.float64))], dtype=np.float32)
    gprob = rs.normal(0, 1.0, size=E).astype(np.float32)
    return dict(emb=emb, pairs=pairs, pi=pi, w1=w1, b1=b1, w2=w2, b2=b2, g=gprob)


def decode_gz(emb_post, pairs, pi, w1, b1, w2, b2, gprob):
    """gz float32[E, 25]: the gradient at the hidden layer's pre-activation, in float32 (the sums of the forward in float32 too; their
    order is not the kernel's, so this is a restatement of the formula, not of the bits)"""
    f = np.float32
    a, b = emb_post[pairs[:, 0]], emb_post[pairs[:, 1]]
    x = np.concatenate([(a - b) * (a - b), pi], 1).astype(f)
    h = (x @ w1.T + b1).astype(f)
    lh = np.where(h > 0, h, f(0.2) * h).astype(f)
    d = (lh @ w2.reshape(-1) + b2[0]).astype(f)
    ad = np.abs(d)
    c = np.minimum(ad, f(40.0))
    ez = np.exp(c - f(2.0)).astype(f)
    p = (f(1.0) / (ez + f(1.0))).astype(f)
    gz = (-gprob * (p * p) * ez).astype(f)
    dd = np.where(ad <= 40.0, gz * np.sign(d).astype(f), f(0.0)).astype(f)
    return ((dd[:, None] * w2.reshape(1, -1)) * np.where(h > 0, f(1.0), f(0.2))).astype(f)


def decode_dpi(gz, w1):
    """d_gpi[i][j] = acc after acc = +0.0; for k ascending: acc = acc + W1[k][16 + j] * gz[i][k], products and sums rounded to f32"""
    f = np.float32
    acc = np.zeros((gz.shape[0], 25), f)
    for k in range(25):
        acc = (acc + (w1[k, 16:][None, :].astype(f) * gz[:, k:k + 1].astype(f)).astype(f)).astype(f)
    return acc

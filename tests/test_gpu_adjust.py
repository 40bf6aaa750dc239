"""Exact adjusted search on the GPU (MI355X only): ``vs_search_adjusted`` through
``FlatIndex.search_adjusted`` and ``VectorStore.search_hybrid``.

Reference for every case (tests/oracle_adjust_index.py ``adjust_reference``): the members scored with
the oracle's canonical fp64 score S, A = float64(scale) * S + float64(bias) in two numpy operations,
ordered by a stable lexicographic sort on (A, id).  ``I``, ``D`` and ``D_raw`` must be equal as bits
under every mode and depth; ``adjust_last_stats`` must equal what ``adjust_need`` predicts from the
reference ranking alone (the two certificates replayed on prefixes of it).

The burst corpus (256 rows, d = 72: the last 64-element chunk is partial; 8 queries) with seven
adjustment schemes.  Depths: the default, (16, 64) and (k, k) -- and (16, 256), under which ``flood``
takes DIRECT at k = 10 with a first list of 16, and (200, 250), under which BOUND meets a negative S_L.
No row of this corpus ranks below 200 for all eight queries (the farthest reaches rank 116): ``sparse``
lifts the six rows farthest from the top of every ranking, all beyond rank 100, and a one-query case
lifts rows ranked below 200 for that query."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import oracle as O
from oracle_adjust_index import (KMAX, SCHEMES, adjust_need, adjust_reference, burst_scheme, far_rows, hybrid_reference,
                                 plain_ranks, plain_rows, resolve_depth)
from oracle_diverse_index import burst_corpus
from oracle_sel_index import filtered_reference
from test_adjust_host import check_hybrid

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "bf16", "f16"]
METRICS = ["ip", "l2"]
KS = [1, 10, 100, 300]
N, D_ = 256, 72
FLT_MAX = np.float32(3.4028235e38)
MODES = ["auto", "direct", "bound", "scan"]


@pytest.fixture(scope="module")
def idx():
    from photo_search_engine_amd import index
    return index


@functools.lru_cache(maxsize=None)
def _stored(dtype):
    x, q = burst_corpus()
    xs = O.round_dtype(x, dtype)
    xs.setflags(write=False)
    return x, xs, q


@functools.lru_cache(maxsize=None)
def _scheme(dtype, metric, name):
    _, xs, q = _stored(dtype)
    scale, bias = burst_scheme(name, O.canon_scores(xs, q, metric), metric)
    scale.setflags(write=False)
    bias.setflags(write=False)
    return scale, bias


@functools.lru_cache(maxsize=None)
def _ref(dtype, metric, name, k, masked=False):
    _, xs, q = _stored(dtype)
    out = adjust_reference(xs, q, *_scheme(dtype, metric, name), k, metric, (np.arange(N) % 3 != 0) if masked else None)
    for a in out:
        a.setflags(write=False)
    return out


def _depths(k):
    return [(0, 0), (16, 64), (k, k), (16, 256), (200, 250)]


def _index(idx, x, dtype, metric):
    ix = idx.FlatIndex(x.shape[1], metric, dtype)
    if x.shape[0]:
        ix.add(np.ascontiguousarray(x))
    return ix


def _eq(res, ref, what=""):
    D, I, R = ref
    np.testing.assert_array_equal(res[1], I, err_msg=f"{what}: I")
    np.testing.assert_array_equal(res[0].view(np.uint32), np.asarray(D).view(np.uint32), err_msg=f"{what}: D")
    np.testing.assert_array_equal(res[2].view(np.uint32), np.asarray(R).view(np.uint32), err_msg=f"{what}: D_raw")


def _stats(ix):
    st = ix.adjust_last_stats()
    return {n: st[n] for n in ("first", "deeper", "scan", "longest", "tier")}


# ---- 1. the burst corpus: schemes x depths x modes -------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_burst_corpus_schemes_depths_and_modes(idx, dtype, metric, k):
    from photo_search_engine_amd import _lib
    x, xs, q = _stored(dtype)
    ix = _index(idx, x, dtype, metric)
    reached = set()
    for name in SCHEMES:
        scale, bias = _scheme(dtype, metric, name)
        m_adj = int((~plain_rows(scale, bias)).sum())
        adj = ix.score_adjust(scale, bias)
        assert adj.rows == N and adj.count == m_adj
        ref = _ref(dtype, metric, name, k)
        if name == "none":  # bit-equal to vs_search
            Dp, Ip = ix.search(q, k)
            np.testing.assert_array_equal(Ip, ref[1])
            np.testing.assert_array_equal(Dp.view(np.uint32), ref[0].view(np.uint32))
        for depth in _depths(k):
            ix.set_adjust_depth(*depth)
            first, limit = resolve_depth(k, m_adj, *depth)
            for mode in MODES:
                ix.set_adjust_mode(mode)
                what = f"{dtype} {metric} {name} k={k} depth={depth} mode={mode}"
                if mode == "direct" and m_adj + k > limit:
                    with pytest.raises(_lib.VsError):
                        ix.search_adjusted(q, k, adj)
                    continue
                _eq(ix.search_adjusted(q, k, adj, return_raw=True), ref, what)
                want, where = adjust_need(xs, q, scale, bias, k, metric, first, limit, mode)
                st = ix.adjust_last_stats()
                print(what, st, want)
                assert _stats(ix) == want and st["queries"] == q.shape[0] and st["adjusted"] == m_adj, what
                reached |= {(want["tier"], w) for w in where}
        adj.close()
    ix.set_adjust_mode("auto")
    # on the CPU: the schemes sent queries to every tier, in the first list and in a deeper one
    want_reached = {("scan", 2), ("bound", 2)}
    if k <= 100:
        want_reached |= {("direct", 0), ("bound", 0)}
    if k <= 10:
        want_reached |= {("direct", 1), ("bound", 1)}
    assert want_reached <= reached, (want_reached - reached)
    ix.close()


def test_schemes_are_what_they_claim(idx):
    """The conditions the schemes are there for, from the reference alone, and the one-query case whose
    lifted rows rank below 200."""
    x, xs, q = _stored("bf16")
    S = O.canon_scores(xs, q, "ip")
    rank = plain_ranks(S, "ip")
    scale, bias = _scheme("bf16", "ip", "sparse")
    far = far_rows(S, "ip")
    assert rank[:, far].min() >= 100 and all(set(far.tolist()) <= set(r.tolist()) for r in _ref("bf16", "ip", "sparse", 10)[1])
    # flood under (16, 64), k = 1: DIRECT, and the first list of 16 holds no plain row for some query
    fs, fb = _scheme("bf16", "ip", "flood")
    st, where = adjust_need(xs, q, fs, fb, 1, "ip", 16, 64)
    assert st["tier"] == "direct" and st["deeper"] >= 3
    st, _ = adjust_need(xs, q, fs, fb, 10, "ip", 16, 256)
    assert st["tier"] == "direct" and st["deeper"] >= 3
    # dense_narrow certifies in a deeper list, dense_wide fails at the limit
    st, _ = adjust_need(xs, q, *_scheme("bf16", "ip", "dense_narrow"), 10, "ip", 16, 64)
    assert st["tier"] == "bound" and st["deeper"] >= 1 and st["scan"] == 0
    st, _ = adjust_need(xs, q, *_scheme("bf16", "ip", "dense_wide"), 10, "ip", 16, 64)
    assert st["tier"] == "bound" and st["scan"] == q.shape[0] and st["longest"] == 64
    # mixed_scale under (200, 250): BOUND, S_L negative for every query, certified all the same
    st, _ = adjust_need(xs, q, *_scheme("bf16", "ip", "mixed_scale"), 10, "ip", 200, 250)
    assert st["tier"] == "bound" and st["first"] == q.shape[0] and all(np.sort(S[qi])[::-1][199] < 0 for qi in range(8))
    # one query, rows ranked below 200 for it, lifted into its top 10
    low = np.flatnonzero(rank[0] >= 200)[:6]
    ix = _index(idx, x, "bf16", "ip")
    adj = ix.score_adjust_sparse(low, None, bias[far])
    b1 = np.zeros((N,), np.float32)
    b1[low] = bias[far]
    ref = adjust_reference(xs, q[:1], np.ones((N,), np.float32), b1, 10, "ip")
    assert set(low.tolist()) <= set(ref[1][0].tolist())
    for depth in ((0, 0), (16, 64), (10, 10)):
        ix.set_adjust_depth(*depth)
        _eq(ix.search_adjusted(q[:1], 10, adj, return_raw=True), ref, f"one query {depth}")
    ix.close()


# ---- 2. selectors, the two creation forms -----------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_selector_and_sparse_creation(idx, dtype, metric):
    x, xs, q = _stored(dtype)
    ix = _index(idx, x, dtype, metric)
    mask = np.arange(N) % 3 != 0
    sel = ix.selector(mask)
    for name in ("sparse", "dense_narrow", "ties"):
        scale, bias = _scheme(dtype, metric, name)
        m_adj = int((~plain_rows(scale, bias)).sum())
        dense = ix.score_adjust(scale, bias)
        rows = np.flatnonzero(~plain_rows(scale, bias))[::-1].copy()  # (any order)
        sparse = ix.score_adjust_sparse(rows, scale[rows], bias[rows])
        assert sparse.count == dense.count == m_adj and sparse.rows == dense.rows == N
        for k in (10, 100):
            ref_m = _ref(dtype, metric, name, k, True)
            for depth in _depths(k)[:3]:
                ix.set_adjust_depth(*depth)
                first, limit = resolve_depth(k, m_adj, *depth)
                for mode in MODES:
                    if mode == "direct" and m_adj + k > limit:
                        continue
                    ix.set_adjust_mode(mode)
                    what = f"{dtype} {metric} {name} k={k} depth={depth} mode={mode}"
                    for s in (sel, mask):
                        _eq(ix.search_adjusted(q, k, dense, sel=s, return_raw=True), ref_m, what + " selector")
                    want, _ = adjust_need(xs, q, scale, bias, k, metric, first, limit, mode, mask)
                    assert _stats(ix) == want, (what, ix.adjust_last_stats(), want)
                    _eq(ix.search_adjusted(q, k, sparse, sel=sel, return_raw=True), ref_m, what + " sparse + selector")
                    _eq(ix.search_adjusted(q, k, sparse, return_raw=True), _ref(dtype, metric, name, k), what + " sparse")
        dense.close()
        sparse.close()
    # a selector that allows nothing, and one that allows fewer rows than k
    scale, bias = _scheme(dtype, metric, "sparse")
    adj = ix.score_adjust(scale, bias)
    ix.set_adjust_mode("auto")
    ix.set_adjust_depth(0, 0)
    D, I, R = ix.search_adjusted(q, 5, adj, sel=np.zeros((N,), bool), return_raw=True)
    worst = -FLT_MAX if metric == "ip" else FLT_MAX
    assert (I == -1).all() and (D == worst).all() and (R == worst).all()
    few = np.zeros((N,), bool)
    few[[3, 44, 200]] = True
    _eq(ix.search_adjusted(q, 10, adj, sel=few, return_raw=True), adjust_reference(xs, q, scale, bias, 10, metric, few), "3 members")
    ix.close()


# ---- 3. the object's life: staleness, rows added later, accounting ----------------------------------------------
def test_staleness_added_rows_and_accounting(idx):
    from photo_search_engine_amd import _lib
    x, xs, q = _stored("bf16")
    ix = _index(idx, x[:200], "bf16", "ip")
    L = ix._L
    scale, bias = _scheme("bf16", "ip", "sparse")
    ix.search(q, 10)
    warm = ix.score_adjust(scale[:200], bias[:200])
    for mode in MODES[1:]:  # (every tier's workspaces exist before the bytes are compared)
        ix.set_adjust_mode(mode)
        ix.search_adjusted(q, 10, warm)
    ix.set_adjust_mode("auto")
    warm.close()
    base = int(L.vs_device_bytes_live())
    adj = ix.score_adjust(scale[:200], bias[:200])
    assert int(L.vs_device_bytes_live()) >= base + 2 * 200 * 4 + 12 * 4  # scale, bias, the id list
    ref = adjust_reference(xs[:200], q, scale[:200], bias[:200], 10, "ip")
    _eq(ix.search_adjusted(q, 10, adj, return_raw=True), ref, "200 rows")
    with_adj = int(L.vs_device_bytes_live())
    # rows added after creation are no members, under every tier, with and without a selector
    old_sel = ix.selector(np.arange(200) % 3 != 0)
    ix.add(np.ascontiguousarray(x[200:]))
    mask = np.arange(N) % 3 != 0
    # (a selector older than the adjustment: the rows behind the selector are not allowed)
    newer = ix.score_adjust(scale, bias)
    ref_o = adjust_reference(xs, q, scale, bias, 10, "ip", mask[:200])
    assert ref_o[1].max() < 200
    for mode in MODES:
        ix.set_adjust_mode(mode)
        _eq(ix.search_adjusted(q, 10, newer, sel=old_sel, return_raw=True), ref_o, f"selector older than the adjustment {mode}")
    newer.close()
    old_sel.close()
    ref_m = adjust_reference(xs, q, scale[:200], bias[:200], 10, "ip", mask)
    assert ref[1].max() < 200 and ref_m[1].max() < 200
    for mode in MODES:
        ix.set_adjust_mode(mode)
        for depth in ((0, 0), (16, 64), (10, 10)):
            ix.set_adjust_depth(*depth)
            if mode == "direct" and depth == (10, 10):
                continue  # (12 adjusted rows + k is beyond this limit: an argument error)
            _eq(ix.search_adjusted(q, 10, adj, return_raw=True), ref, f"rows added later {mode} {depth}")
            _eq(ix.search_adjusted(q, 10, adj, sel=mask, return_raw=True), ref_m, f"rows added later, mask {mode} {depth}")
            if mode == "direct" and depth != (0, 0):
                continue  # (12 adjusted rows + 300 is beyond these limits: an argument error)
            _eq(ix.search_adjusted(q, 300, adj, return_raw=True), adjust_reference(xs, q, scale[:200], bias[:200], 300, "ip"),
                f"rows added later k=300 {mode} {depth}")
    ix.set_adjust_mode("auto")
    ix.set_adjust_depth(0, 0)
    assert int(L.vs_device_bytes_live()) >= with_adj  # (the context's workspaces may have grown; the object stays)
    # scratch is freed before return: a repeated call leaves the count where it was
    ix.search_adjusted(q, 10, adj, sel=mask)
    before = int(L.vs_device_bytes_live())
    ix.search_adjusted(q, 10, adj, sel=mask)
    assert int(L.vs_device_bytes_live()) == before
    adj.close()
    assert int(L.vs_device_bytes_live()) < before
    # a fresh object costs what the closed one did; destroy gives it back
    level = int(L.vs_device_bytes_live())
    again = ix.score_adjust_sparse([1, 2, 3], [2.0, 0.5, 1.0], [0.0, 0.0, 0.25])
    assert again.count == 3 and int(L.vs_device_bytes_live()) > level
    again.close()
    assert int(L.vs_device_bytes_live()) == level
    # stale after a removal that removed a row, and after reset; not after a removal that removed nothing
    adj = ix.score_adjust(None, None)
    assert adj.count == 0 and adj.rows == N
    assert ix.remove_ids(np.zeros((0,), dtype=np.int64)) == 0
    ix.search_adjusted(q, 3, adj)
    assert ix.remove_ids([5]) == 1
    with pytest.raises(_lib.VsError):
        ix.search_adjusted(q, 3, adj)
    adj2 = ix.score_adjust(None, bias[:255])
    ix.search_adjusted(q, 3, adj2)
    ix.reset()
    with pytest.raises(_lib.VsError):
        ix.search_adjusted(q, 3, adj2)
    ix.close()


def _raw(ix, adj, q, nq, k, sel=None, D=True, I=True, R=True, qnull=False):
    n, kk = max(nq, 1), max(k, 1)
    Dv = np.full((n, kk), -7.0, dtype=np.float32)
    Iv = np.full((n, kk), -7, dtype=np.int64)
    Rv = np.full((n, kk), -7.0, dtype=np.float32)
    p = lambda a, on: a.ctypes.data if on else None  # noqa: E731
    rc = ix._L.vs_search_adjusted(ix._h, adj, sel, p(q, not qnull), nq, k, p(Dv, D), p(Iv, I), p(Rv, R))
    return rc, Dv, Iv, Rv


def _untouched(out):
    return (out[1] == -7.0).all() and (out[2] == -7).all() and (out[3] == -7.0).all()


def test_argument_errors_and_empty_inputs(idx):
    from photo_search_engine_amd import _lib
    x, xs, q = _stored("bf16")
    ix = _index(idx, x, "bf16", "ip")
    other = _index(idx, x, "bf16", "ip")
    scale, bias = _scheme("bf16", "ip", "sparse")
    adj, foreign = ix.score_adjust(scale, bias), other.score_adjust(scale, bias)
    ref = _ref("bf16", "ip", "sparse", 10)
    out = _raw(ix, adj._h, q, 0, 5)
    assert out[0] == 0 and _untouched(out)
    assert ix.search_adjusted(np.zeros((0, D_), dtype=np.float32), 5, adj)[1].shape == (0, 5)
    rc, Dv, Iv, Rv = _raw(ix, adj._h, q, 8, 10, R=False)  # D_raw may be NULL
    assert rc == 0 and (Rv == -7.0).all()
    np.testing.assert_array_equal(Iv, ref[1])
    for case in (dict(k=0), dict(k=-3), dict(k=KMAX + 1), dict(D=False), dict(I=False), dict(qnull=True), dict(nq=-1),
                 dict(adj=foreign._h), dict(adj=None)):
        flags = {n: v for n, v in case.items() if n not in ("k", "nq", "adj")}
        out = _raw(ix, case.get("adj", adj._h), q, case.get("nq", 8), case.get("k", 10), **flags)
        assert out[0] == _lib.VS_ERR_ARG and _untouched(out), case
    assert _raw(ix, adj._h, q, 8, KMAX)[0] == 0  # the limit is legal
    foreign_sel = other.selector(np.ones((N,), bool))
    out = _raw(ix, adj._h, q, 8, 10, sel=foreign_sel._h)
    assert out[0] == _lib.VS_ERR_ARG and _untouched(out)
    with pytest.raises(TypeError):
        ix.search_adjusted(q, 3, scale)
    # creation: lengths, values (checked before any upload), ids
    with pytest.raises(ValueError):
        ix.score_adjust(scale[:-1], None)
    h = ctypes.c_void_p()
    assert ix._L.vs_adjust_create(ix._h, scale.ctypes.data, None, N - 1, ctypes.byref(h)) == _lib.VS_ERR_ARG and not h.value
    live = int(ix._L.vs_device_bytes_live())
    for bad_s, bad_b in ((-1.0, 0.0), (np.nan, 0.0), (np.inf, 0.0), (1.0, np.nan), (1.0, -np.inf), (-0.5, np.nan)):
        s, b = scale.copy(), bias.copy()
        s[17], b[17] = bad_s, bad_b
        with pytest.raises(_lib.VsError):
            ix.score_adjust(s, b)
        with pytest.raises(_lib.VsError):
            ix.score_adjust_sparse([4, 17], [1.0, bad_s], [0.0, bad_b])
    for ids in ([1, 1], [-1], [N], [0, N + 5]):
        with pytest.raises(_lib.VsError):
            ix.score_adjust_sparse(ids, None, np.full((len(ids),), 0.5))
    assert int(ix._L.vs_device_bytes_live()) == live
    zero = ix.score_adjust(np.zeros((N,), np.float32), None)  # scale 0 is legal (negative zero too)
    assert zero.count == N
    assert ix.score_adjust(-np.zeros((N,), np.float32) + 1, -np.zeros((N,), np.float32)).count == 0
    # depth and mode settings
    for bad in ((-1, 0), (0, KMAX + 1), (65, 64), (KMAX + 1, KMAX + 1)):
        with pytest.raises(_lib.VsError):
            ix.set_adjust_depth(*bad)
    with pytest.raises(ValueError):
        ix.set_adjust_mode("fast")
    assert ix._L.vs_set_adjust_mode(ix._h, 7) == _lib.VS_ERR_ARG
    ix.set_adjust_mode("direct")
    ix.set_adjust_depth(4, 21)  # 12 adjusted rows + k = 10 > 21
    out = _raw(ix, adj._h, q, 8, 10)
    assert out[0] == _lib.VS_ERR_ARG and _untouched(out)
    ix.set_adjust_depth(4, 22)
    _eq(ix.search_adjusted(q, 10, adj, return_raw=True), ref, "adjusted rows + k == limit")
    # the empty index: all padding
    empty = _index(idx, x[:0], "bf16", "ip")
    ea = empty.score_adjust(None, None)
    assert ea.rows == 0 and ea.count == 0
    D, I, R = empty.search_adjusted(q, 4, ea, return_raw=True)
    assert (I == -1).all() and (D == -FLT_MAX).all() and (R == -FLT_MAX).all()
    assert empty.adjust_last_stats()["first"] == q.shape[0]


# ---- 4. larger shapes ------------------------------------------------------------------------------------------
def test_4096_rows_take_the_batch_screen(idx):
    """4096 rows, d = 136, nine queries: the list search takes the batch screen, not the small index's full
    scan.  200 adjusted rows (DIRECT) and a dense narrow bias (BOUND under the depth (32, 512))."""
    rng = np.random.default_rng(3)
    n, d, nq = 4096, 136, 9
    x = rng.standard_normal((n, d)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    mask = np.arange(n) % 3 != 0
    for dtype, metric in (("bf16", "ip"), ("f32", "l2")):
        xs = O.round_dtype(x, dtype)
        sgn = 1.0 if metric == "ip" else -1.0
        ix = _index(idx, x, dtype, metric)
        rows = rng.permutation(n)[:200]
        s200 = rng.uniform(0.5, 1.5, 200).astype(np.float32)
        b200 = (sgn * rng.uniform(0.0, 0.4, 200)).astype(np.float32)
        scale, bias = np.ones((n,), np.float32), np.zeros((n,), np.float32)
        scale[rows], bias[rows] = s200, b200
        sparse = ix.score_adjust_sparse(rows, s200, b200)
        nb = (sgn * rng.uniform(0.0, 0.01, n)).astype(np.float32)
        narrow = ix.score_adjust(None, nb)
        for k in (10, 100):
            for depth in ((0, 0), (32, 512)):
                ix.set_adjust_depth(*depth)
                for adj, sc, bi, m_adj in ((sparse, scale, bias, 200), (narrow, np.ones((n,), np.float32), nb, n)):
                    first, limit = resolve_depth(k, m_adj, *depth)
                    for m in (None, mask):
                        what = f"4096 rows {dtype} {metric} k={k} depth={depth} m_adj={m_adj} mask={m is not None}"
                        _eq(ix.search_adjusted(q, k, adj, sel=m, return_raw=True), adjust_reference(xs, q, sc, bi, k, metric, m), what)
                        want, _ = adjust_need(xs, q, sc, bi, k, metric, first, limit, "auto", m)
                        assert _stats(ix) == want, (what, ix.adjust_last_stats(), want)
        ix.close()


def test_batch_of_300_queries(idx):
    """More queries than one scan block (256): the direct scan, the walk's query map and the full scan run
    over two blocks, and the queries a deeper list takes are no prefix of the batch."""
    x, xs, q = _stored("bf16")
    ix = _index(idx, x, "bf16", "ip")
    q300 = np.ascontiguousarray(np.tile(q, (38, 1))[:300])
    for name, k, depth in (("flood", 1, (16, 64)), ("flood", 10, (16, 256)), ("dense_narrow", 10, (16, 64)),
                           ("dense_wide", 10, (16, 64)), ("ties", 10, (10, 10))):
        scale, bias = _scheme("bf16", "ip", name)
        adj = ix.score_adjust(scale, bias)
        ref = tuple(np.tile(a, (38, 1))[:300] for a in _ref("bf16", "ip", name, k))
        ix.set_adjust_depth(*depth)
        _eq(ix.search_adjusted(q300, k, adj, return_raw=True), ref, f"300 queries {name} {depth}")
        first, limit = resolve_depth(k, adj.count, *depth)
        want, _ = adjust_need(xs, q300, scale, bias, k, "ip", first, limit)
        assert _stats(ix) == want, (name, ix.adjust_last_stats(), want)
        adj.close()
    ix.close()


# ---- 5. the store route ----------------------------------------------------------------------------------------
def test_store_search_hybrid_on_64_photos(tmp_path):
    from photo_search_engine_amd import vector_store as vsmod
    x, q = burst_corpus()
    meta = [{"photo_path": f"/p/{i}.jpg", "year": 2019 + i % 6} for i in range(64)]
    store = vsmod.VectorStore(dimension=D_, index_path=str(tmp_path / "idx"), metadata_path=str(tmp_path / "meta.json"),
                              metric="cosine", index_type="flat")
    store.add(np.array(x[:64]), meta)

    class View:  # (the brute-force fusion reads the values as stored)
        _x = store.index.reconstruct_n(0, 64)

    class Shim:
        index = View()
        _normalize_query = staticmethod(store._normalize_query)
        search_hybrid = staticmethod(store.search_hybrid)

    check_hybrid(Shim(), q, meta)
    assert store.index.adjust_last_stats()["tier"] == "direct"
    l2 = vsmod.VectorStore(dimension=D_, index_path=str(tmp_path / "l2"), metadata_path=str(tmp_path / "l2.json"),
                           metric="l2", index_type="flat")
    l2.add(np.array(x[:8]), meta[:8])
    with pytest.raises(ValueError):
        l2.search_hybrid(q[0].tolist(), 3, {})

"""Exact diversified search on the GPU (MI355X only): ``vs_search_diverse`` through
``FlatIndex.search_diverse``, ``VectorStore.search_diverse`` and the multi-device route.

Reference for every case (tests/oracle_diverse_index.py ``diverse_reference``): the members ranked by
the oracle's canonical fp64 score, walked best first in explicit loops.  ``D``, ``I``, ``hidden`` and
``examined`` must be bit-equal, whichever tier answered the query.

The burst corpus (256 rows, d = 72: the last 64-element chunk is partial) is the smallest shape that
reaches every tier under ``set_diverse_depth(16, 64)``: at k = 2 and k = 10 its eight queries end in
the first list, in a deeper list and in the full ranking."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import oracle as O
from oracle_diverse_index import burst_corpus, diverse_reference, oracle_diverse_factory, staged_chunk

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "bf16", "f16"]
METRICS = ["ip", "l2"]
N, D_ = 256, 72
FLT_MAX = np.float32(3.4028235e38)


@pytest.fixture(scope="module")
def idx():
    from photo_search_engine_amd import index
    return index


def _radius(metric):
    return np.float32(0.9 if metric == "ip" else 0.2)


@functools.lru_cache(maxsize=None)
def _stored(dtype):
    x, q = burst_corpus()
    xs = O.round_dtype(x, dtype)
    xs.setflags(write=False)
    return x, xs, q


@functools.lru_cache(maxsize=None)
def _ref(dtype, metric, k):
    _, xs, q = _stored(dtype)
    out = diverse_reference(xs, q, k, _radius(metric), metric)
    for a in out:
        a.setflags(write=False)
    return out


def _index(idx, x, dtype, metric):
    ix = idx.FlatIndex(x.shape[1], metric, dtype)
    if x.shape[0]:
        ix.add(np.ascontiguousarray(x))
    return ix


def _eq(res, ref, what=""):
    D, I, hidden, examined = ref
    np.testing.assert_array_equal(res.I, I, err_msg=f"{what}: I")
    np.testing.assert_array_equal(res.D.view(np.uint32), np.asarray(D).view(np.uint32), err_msg=f"{what}: D")
    np.testing.assert_array_equal(res.hidden, hidden, err_msg=f"{what}: hidden")
    np.testing.assert_array_equal(res.examined, examined, err_msg=f"{what}: examined")
    np.testing.assert_array_equal(res.hidden.sum(axis=1) + (res.I >= 0).sum(axis=1), res.examined)


def _tiers(examined, accepted, k, first, limit, members):
    """Queries the contract's tiers answer, from the reference alone: a list of L rows completes a
    query iff it accepted k rows within it, or the list held every member."""
    L0, L1 = min(first, members), min(limit, members)
    done0 = ((accepted == k) & (examined <= L0)) | (L0 >= members)
    done1 = ((accepted == k) & (examined <= L1)) | (L1 >= members)
    return int(done0.sum()), int((done1 & ~done0).sum()), int((~done1).sum())


# ---- 1. the burst corpus under default and forced depths -----------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_burst_corpus_every_tier(idx, dtype, metric):
    x, xs, q = _stored(dtype)
    ix = _index(idx, x, dtype, metric)
    r = _radius(metric)
    seen = np.zeros(3, dtype=np.int64)
    for k in (2, 10):
        ref = _ref(dtype, metric, k)
        plain = ix.search(q, k)[1]
        if k == 10:
            assert (ref[1] != plain).any(axis=1).all()  # every query differs from the plain top-10
        ix.set_diverse_depth(0, 0)
        _eq(ix.search_diverse(q, k, r), ref, f"{dtype} {metric} k={k} default depths")
        st = ix.diverse_last_stats()
        accepted = (ref[1] >= 0).sum(axis=1)
        assert st["queries"] == 8 and (st["first"], st["deeper"], st["full"]) == _tiers(ref[3], accepted, k, 64, 3276, N)
        ix.set_diverse_depth(16, 64)
        _eq(ix.search_diverse(q, k, r), ref, f"{dtype} {metric} k={k} depths (16, 64)")
        st = ix.diverse_last_stats()
        want = _tiers(ref[3], accepted, k, 16, 64, N)
        assert (st["first"], st["deeper"], st["full"]) == want, (st, want)
        seen += want
        ix.set_diverse_depth(1, 1)
        _eq(ix.search_diverse(q, k, r), ref, f"{dtype} {metric} k={k} depths (1, 1)")
        assert ix.diverse_last_stats()["full"] == 8 and ix.diverse_last_stats()["longest"] == N
    # a condition, not a measurement: a run that never left tier 1 proves nothing about tiers 2 and 3
    assert (seen >= 1).all(), seen


# ---- 2. selectors ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_selectors(idx, dtype, metric):
    from photo_search_engine_amd import _lib
    x, xs, q = _stored(dtype)
    r = _radius(metric)
    ix = _index(idx, x[:200], dtype, metric)
    early = ix.selector(np.arange(200) % 2 == 0)  # made before the add: the later rows are not members
    ix.add(np.ascontiguousarray(x[200:]))
    mask = np.arange(N) % 3 != 0
    for depths in ((0, 0), (16, 64)):
        ix.set_diverse_depth(*depths)
        for k in (2, 10):
            _eq(ix.search_diverse(q, k, r, sel=mask), diverse_reference(xs, q, k, r, metric, mask), f"mask k={k} {depths}")
        em = np.zeros((N,), dtype=bool)
        em[:200] = np.arange(200) % 2 == 0
        _eq(ix.search_diverse(q, 10, r, sel=early), diverse_reference(xs, q, 10, r, metric, em), f"early selector {depths}")
        none = ix.search_diverse(q, 4, r, sel=np.zeros((N,), dtype=bool))
        assert (none.I == -1).all() and (none.hidden == 0).all() and (none.examined == 0).all()
        assert (none.D == (-FLT_MAX if metric == "ip" else FLT_MAX)).all()
        one = np.zeros((N,), dtype=bool)
        one[137] = True
        _eq(ix.search_diverse(q, 4, r, sel=one), diverse_reference(xs, q, 4, r, metric, one), f"one row {depths}")
    assert ix.remove_ids([5]) == 1
    with pytest.raises(_lib.VsError) as e:
        ix.search_diverse(q, 4, r, sel=early)
    assert e.value.code == _lib.VS_ERR_ARG


# ---- 3. strictness at the boundary -------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_radius_is_strict(idx, dtype, metric):
    """The closest pair (a, b) of the corpus: at radius exactly float32(S(a, b)) no pair is near and the
    answer is the plain search; one ulp towards the passing side the pair is near and b hides under a."""
    x, xs, _ = _stored(dtype)
    S = O.canon_scores(xs, xs, metric)
    np.fill_diagonal(S, -np.inf if metric == "ip" else np.inf)
    a, b = np.unravel_index(np.argmax(S) if metric == "ip" else np.argmin(S), S.shape)
    a, b = int(min(a, b)), int(max(a, b))
    at = np.float32(S[a, b])
    past = np.nextafter(at, np.float32(-np.inf if metric == "ip" else np.inf), dtype=np.float32)
    q = np.ascontiguousarray(xs[[a]])
    ix = _index(idx, x, dtype, metric)
    ref_at, ref_past = diverse_reference(xs, q, 5, at, metric), diverse_reference(xs, q, 5, past, metric)
    assert a in ref_at[1][0] and b in ref_at[1][0] and (ref_at[2] == 0).all()
    assert (a in ref_past[1][0]) != (b in ref_past[1][0]) and ref_past[2].sum() >= 1
    for depths in ((0, 0), (1, 2)):
        ix.set_diverse_depth(*depths)
        _eq(ix.search_diverse(q, 5, at), ref_at, f"at the boundary {depths}")
        _eq(ix.search_diverse(q, 5, past), ref_past, f"one ulp past {depths}")


# ---- 4. ties: hundreds of identical rows, answered from the full ranking -------------------------------------------
@pytest.mark.parametrize("dtype,metric", [("bf16", "ip"), ("f32", "l2"), ("f16", "ip")])
def test_identical_rows_through_the_full_ranking(idx, dtype, metric):
    rng = np.random.default_rng(21)
    x = rng.standard_normal((320, D_)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    copies = np.sort(rng.permutation(320)[:300])
    x[copies] = x[copies[0]]
    xs = O.round_dtype(x, dtype)
    q = np.ascontiguousarray(xs[[copies[0]]])
    r = np.float32(0.99 if metric == "ip" else 0.02)
    ref = diverse_reference(xs, q, 5, r, metric)
    assert ref[1][0, 0] == copies[0] and ref[2][0, 0] == 299 and ref[3][0] > 300
    ix = _index(idx, x, dtype, metric)
    ix.set_diverse_depth(16, 64)
    _eq(ix.search_diverse(q, 5, r), ref, "ties")
    st = ix.diverse_last_stats()
    assert st["full"] == 1 and st["longest"] == 320
    ix.set_diverse_depth(0, 0)
    _eq(ix.search_diverse(q, 5, r), ref, "ties, default depths")


# ---- 5. infinite radii -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_infinite_radii(idx, dtype, metric):
    x, xs, q = _stored(dtype)
    ix = _index(idx, x, dtype, metric)
    nothing, everything = (np.inf, -np.inf) if metric == "ip" else (-np.inf, np.inf)
    mask = np.arange(N) % 3 != 0
    for sel, members in ((None, N), (mask, int(mask.sum()))):
        D, I = ix.search(q, 10, sel=sel)
        res = ix.search_diverse(q, 10, nothing, sel=sel)
        np.testing.assert_array_equal(res.I, I)
        np.testing.assert_array_equal(res.D.view(np.uint32), D.view(np.uint32))
        assert (res.hidden == 0).all() and (res.examined == 10).all()
        for depths in ((0, 0), (16, 64)):
            ix.set_diverse_depth(*depths)
            res = ix.search_diverse(q, 10, everything, sel=sel)
            np.testing.assert_array_equal(res.I[:, 0], I[:, 0])
            np.testing.assert_array_equal(res.D[:, 0].view(np.uint32), D[:, 0].view(np.uint32))
            assert (res.I[:, 1:] == -1).all() and (res.hidden[:, 0] == members - 1).all()
            assert (res.examined == members).all()
            _eq(res, diverse_reference(xs, q, 10, everything, metric, sel), f"everything near {depths}")
        ix.set_diverse_depth(0, 0)


# ---- 6. exhausted rankings, empty inputs, argument errors --------------------------------------------------------
def _raw(ix, q, nq, k, radius, D=True, I=True, hidden=True, examined=True, qnull=False, rnull=False):
    """``vs_search_diverse`` itself, outputs pre-filled with sentinels: (rc, D, I, hidden, examined)."""
    kk = max(k, 1)
    Dv = np.full((max(nq, 1), kk), -7.0, dtype=np.float32)
    Iv = np.full((max(nq, 1), kk), -7, dtype=np.int64)
    hv = np.full((max(nq, 1), kk), -7, dtype=np.int32)
    ev = np.full((max(nq, 1),), -7, dtype=np.int64)
    r = np.ascontiguousarray(np.broadcast_to(np.asarray(radius, dtype=np.float32), (max(nq, 1),)))
    p = lambda a, on: a.ctypes.data if on else None  # noqa: E731
    rc = ix._L.vs_search_diverse(ix._h, None, p(q, not qnull), nq, k, p(r, not rnull), p(Dv, D), p(Iv, I), p(hv, hidden),
                                 p(ev, examined))
    return rc, Dv, Iv, hv, ev


def test_exhausted_ranking_empty_inputs_and_argument_errors(idx):
    from photo_search_engine_amd import _lib
    x, xs, q = _stored("bf16")
    ix = _index(idx, x, "bf16", "ip")
    r = _radius("ip")
    ref = _ref("bf16", "ip", 60)
    assert ((ref[1] >= 0).sum(axis=1) == 40).all() and (ref[3] == N).all()  # one row per burst, then padding
    for depths in ((0, 0), (16, 64)):
        ix.set_diverse_depth(*depths)
        _eq(ix.search_diverse(q, 60, r), ref, f"k = 60 {depths}")
    ix.set_diverse_depth(0, 0)
    _eq(ix.search_diverse(q, 300, r), diverse_reference(xs, q, 300, r, "ip"), "k beyond the rows")
    # nq = 0 returns at once, nothing is written
    rc, Dv, Iv, hv, ev = _raw(ix, q, 0, 5, r)
    assert rc == 0 and (Dv == -7.0).all() and (Iv == -7).all() and (hv == -7).all() and (ev == -7).all()
    assert ix.search_diverse(np.zeros((0, D_), dtype=np.float32), 5, r).I.shape == (0, 5)
    # hidden and examined may be NULL
    rc, Dv, Iv, hv, ev = _raw(ix, q, 8, 10, r, hidden=False, examined=False)
    assert rc == 0
    np.testing.assert_array_equal(Iv, _ref("bf16", "ip", 10)[1])
    assert (hv == -7).all() and (ev == -7).all()
    # argument errors: checked before anything is launched, outputs untouched
    for case in (dict(k=0), dict(k=-3), dict(k=3277), dict(radius=np.nan), dict(D=False), dict(I=False), dict(qnull=True),
                 dict(rnull=True), dict(nq=-1)):
        rc, Dv, Iv, hv, ev = _raw(ix, q, case.get("nq", 8), case.get("k", 10), case.get("radius", r),
                                  **{n: v for n, v in case.items() if n not in ("k", "radius", "nq")})
        assert rc == _lib.VS_ERR_ARG, case
        assert (Dv == -7.0).all() and (Iv == -7).all() and (hv == -7).all() and (ev == -7).all(), case
    rc = _raw(ix, q, 8, 3276, r)[0]
    assert rc == 0  # vs_search's limit itself is legal
    for bad in ((-1, 0), (0, 3277), (65, 64), (3277, 3277)):
        with pytest.raises(_lib.VsError):
            ix.set_diverse_depth(*bad)
    # the empty index: all padding, examined = 0
    empty = _index(idx, x[:0], "bf16", "ip")
    res = empty.search_diverse(q, 4, r)
    assert (res.I == -1).all() and (res.D == -FLT_MAX).all() and (res.hidden == 0).all() and (res.examined == 0).all()
    assert _raw(empty, q, 8, 3277, r)[0] == _lib.VS_ERR_ARG and _raw(empty, q, 8, 4, np.nan)[0] == _lib.VS_ERR_ARG


# ---- 7. other shapes and mechanics -------------------------------------------------------------------------------
def test_wide_rows_bf16(idx):
    x, q = burst_corpus(d=1536, nbase=80, nq=3, seed=9)
    x = np.ascontiguousarray(x[:512])
    xs = O.round_dtype(x, "bf16")
    ix = _index(idx, x, "bf16", "ip")
    for depths, k in (((0, 0), 10), ((16, 64), 10), ((16, 64), 3)):
        ix.set_diverse_depth(*depths)
        _eq(ix.search_diverse(q, k, 0.9), diverse_reference(xs, q, k, 0.9, "ip"), f"d = 1536 {depths} k={k}")


def test_batch_of_300_and_workspace_accounting(idx):
    x, xs, q = _stored("bf16")
    ix = _index(idx, x, "bf16", "ip")
    L = ix._L
    r = _radius("ip")
    q300 = np.ascontiguousarray(np.tile(q, (38, 1))[:300])
    ref = tuple(np.tile(a, (38,) + (1,) * (a.ndim - 1))[:300] for a in _ref("bf16", "ip", 10))
    rr = np.full((300,), r, dtype=np.float32)
    rr[7::8] = -np.inf  # one radius per query: every eighth one collapses everything
    ref_r = diverse_reference(xs, q300, 10, rr, "ip")
    for depths in ((0, 0), (16, 64)):
        ix.set_diverse_depth(*depths)
        _eq(ix.search_diverse(q300, 10, r), ref, f"300 queries {depths}")
        st = ix.diverse_last_stats()
        assert st["queries"] == 300 and st["first"] + st["deeper"] + st["full"] == 300
        _eq(ix.search_diverse(q300, 10, rr), ref_r, f"300 queries, own radii {depths}")
    before = int(L.vs_device_bytes_live())  # (the context's workspaces exist by now)
    _eq(ix.search_diverse(q300, 10, rr), ref_r, "300 queries again")
    assert ix.diverse_last_stats()["full"] > 0  # the call went through tier 3's own buffers
    assert int(L.vs_device_bytes_live()) == before


def test_tiers_run_over_several_staged_chunks(idx):
    """Lists of 1400 rows make a staged chunk 256 queries (8 MiB of pinned staging, 12 L + 4 bytes per
    query), so 300 queries take two.  Radii: under -inf everything is near and under 0.05 most rows are,
    so such a query stays short past 350 rows (it ends within 1400, or when its list holds every row);
    every seventh query has the ordinary radius and ends in the first list.  The three radii follow
    patterns of period 7 and 3 over queries of period 8, so a chunk that starts at query 256, or at
    pending query 256, and reads its radii from the wrong offset gets another answer.  Depths
    (1400, 1400): tier 1 runs over chunks of 256 + 44.  Depths (350, 1400): tier 1 is one chunk, and the
    258 queries left, which are no prefix of the batch, go through tier 2 as 256 + 2."""
    x, q = burst_corpus(nbase=216)
    x = np.ascontiguousarray(x[:1400])  # (L = 1400 then holds every member: nothing is left to tier 3)
    xs = O.round_dtype(x, "bf16")
    n, k = x.shape[0], 10
    i = np.arange(300)
    rr = np.where(i % 7 == 6, _radius("ip"), np.where(i % 3 == 0, np.float32(0.05), np.float32(-np.inf))).astype(np.float32)
    q300 = np.ascontiguousarray(np.tile(q, (38, 1))[:300])
    by_radius = {r: diverse_reference(xs, q, k, r, "ip") for r in np.unique(rr).tolist()}  # (8 queries each)
    ref = tuple(np.stack([by_radius[float(rr[j])][a][j % 8] for j in range(300)]) for a in range(4))
    accepted = (ref[1] >= 0).sum(axis=1)
    want = {depths: _tiers(ref[3], accepted, k, *depths, n) for depths in ((1400, 1400), (350, 1400))}
    # conditions, from the reference alone: both tier loops run over more than one chunk of 256, and the
    # radii (and with them the answers) of the second chunk differ from those at the same offsets of the first
    assert n == 1400 and staged_chunk(1400, D_) == 256 and staged_chunk(350, D_) >= 300
    assert want[(1400, 1400)] == (300, 0, 0)
    assert want[(350, 1400)][0] >= 1 and want[(350, 1400)][1] >= 257 and want[(350, 1400)][2] == 0
    pending = np.flatnonzero(~((accepted == k) & (ref[3] <= 350)))
    assert pending.shape[0] == want[(350, 1400)][1] and (pending != np.arange(pending.shape[0])).any()
    assert (rr[256:] != rr[:44]).any() and (rr[pending[256:]] != rr[pending[:pending.shape[0] - 256]]).any()
    ix = _index(idx, x, "bf16", "ip")
    for depths in ((1400, 1400), (350, 1400)):
        ix.set_diverse_depth(*depths)
        _eq(ix.search_diverse(q300, k, rr), ref, f"300 queries, lists of 1400, depths {depths}")
        st = ix.diverse_last_stats()
        assert (st["first"], st["deeper"], st["full"]) == want[depths] and st["longest"] == 1400, (st, want[depths])


@pytest.mark.parametrize("index_type,metric", [("flat", "cosine"), ("hnsw", "l2")])
def test_store_route_equals_the_oracle_store(tmp_path, monkeypatch, index_type, metric):
    from photo_search_engine_amd import vector_store as vsmod
    x, q = burst_corpus()
    meta = [{"photo_path": f"/p/{i}.jpg", "year": 2019 + i % 6} for i in range(N)]

    def make(sub):
        store = vsmod.VectorStore(dimension=D_, index_path=str(tmp_path / sub / "idx"),
                                  metadata_path=str(tmp_path / sub / "meta.json"), metric=metric, index_type=index_type)
        store.add(np.array(x), meta)
        return store

    gpu = make("gpu")
    monkeypatch.setattr(vsmod, "_index_factory", oracle_diverse_factory)
    ref = make("ref")
    ref.index._x = gpu.index.reconstruct_n(0, N)  # (the values as stored)
    thr = 0.9 if metric == "cosine" else 0.2
    pred = lambda m: m["year"] != 2020  # noqa: E731
    for qi, k in ((0, 10), (3, 1), (5, 1000)):
        got = gpu.search_diverse(q[qi].tolist(), k, thr)
        assert got == ref.search_diverse(q[qi].tolist(), k, thr) and got
        assert gpu.search_diverse(q[qi].tolist(), k, thr, allowed=pred) == ref.search_diverse(q[qi].tolist(), k, thr,
                                                                                                 allowed=pred)
    assert sum(g["similar_hidden"] for g in gpu.search_diverse(q[5].tolist(), 1000, thr)) == N - 40
    with pytest.raises(ValueError):
        gpu.search_diverse(q[0, :10].tolist(), 3, thr)


def test_multi_device_route_equals_one_device(idx):
    x, xs, q = _stored("f32")
    mi = idx.MultiDeviceFlatIndex(D_, "ip", "f32", devices=(0, 0))
    mi.add(np.ascontiguousarray(x))
    r = _radius("ip")
    _eq(mi.search_diverse(q, 10, r), _ref("f32", "ip", 10), "multi")
    mask = np.arange(N) % 3 != 0
    want = diverse_reference(xs, q, 10, r, "ip", mask)
    _eq(mi.search_diverse(q, 10, r, sel=mask), want, "multi, mask")
    _eq(mi.search_diverse(q, 10, r, sel=mi.selector(mask)), want, "multi, selector")
    mi.close()

"""The adjusted search's reference recipe and the store route, without a GPU: the contract's identities on
``adjust_reference``, the monotonicity claim behind the BOUND certificate, what ``adjust_need`` predicts
for the test schemes, and ``VectorStore.search_hybrid`` on the oracle index against a brute-force fusion
over all rows."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from oracle_adjust_index import (SCHEMES, adjust_bound, adjust_need, adjust_reference, burst_scheme, far_rows,
                                 hybrid_reference, oracle_adjust_factory, plain_ranks, plain_rows, resolve_depth)
from oracle_diverse_index import burst_corpus
from oracle_sel_index import filtered_reference

N, D_ = 256, 72
KS = [1, 10, 100, 300]


@functools.lru_cache(maxsize=None)
def _scores(metric):
    x, q = burst_corpus()
    return x, q, O.canon_scores(x, q, metric)


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_reference_identities(metric):
    x, q, S = _scores(metric)
    ones, zeros = np.ones((N,), np.float32), np.zeros((N,), np.float32)
    mask = np.arange(N) % 3 != 0
    for k in KS:
        for m in (None, mask):
            Dp, Ip = filtered_reference(x, q, np.ones((N,), bool) if m is None else m, k, metric)
            # every row plain (a negative zero bias included): bit-equal to the plain search, D_raw == D
            for b in (zeros, -zeros):
                D, I, R = adjust_reference(x, q, ones, b, k, metric, m)
                np.testing.assert_array_equal(I, Ip)
                np.testing.assert_array_equal(_bits(D), _bits(Dp))
                np.testing.assert_array_equal(_bits(R), _bits(Dp))
            # a uniform power-of-two scale: the same ids, D the scaled value, D_raw untouched
            for s in (0.25, 8.0):
                D, I, R = adjust_reference(x, q, ones * np.float32(s), zeros, k, metric, m)
                np.testing.assert_array_equal(I, Ip)
                np.testing.assert_array_equal(_bits(D[I >= 0]), _bits(Dp[I >= 0] * np.float32(s)))
                np.testing.assert_array_equal(_bits(R), _bits(Dp))
    # rows behind the covered ones are no members
    D, I, _ = adjust_reference(x, q, ones[:200], zeros[:200], 300, metric)
    assert I.max() < 200 and (I >= 0).sum(axis=1).tolist() == [200] * q.shape[0]


def test_bound_monotonicity_on_random_triples():
    """No row behind the list exceeds the bound: for scale in [smin, smax] (>= 0), bias in [bmin, bmax] and
    S no better than S_L, fl(fl(scale S) + bias) is at most (L2: at least) the certificate's bound --
    negative S_L, zero scales and huge magnitudes included."""
    rng = np.random.default_rng(5)
    for trial in range(400):
        mag = 10.0 ** rng.integers(-6, 7)
        scale = np.abs(rng.standard_normal(64) * 10.0 ** rng.integers(-3, 4)).astype(np.float32)
        if trial % 5 == 0:
            scale[rng.integers(0, 64, 8)] = 0.0
        bias = (rng.standard_normal(64) * mag).astype(np.float32)
        S_L = np.float64(rng.standard_normal() * mag)
        for metric in ("ip", "l2"):
            bound = adjust_bound(S_L, scale, bias, metric)
            gap = np.abs(rng.standard_normal(64)) * mag * 10.0 ** rng.integers(-17, 1)
            gap[:4] = 0.0  # (rows tied with the list's last entry are behind it too)
            S = S_L - gap if metric == "ip" else S_L + gap
            A = scale.astype(np.float64) * S
            A = A + bias.astype(np.float64)
            assert np.all(A <= bound) if metric == "ip" else np.all(A >= bound), (trial, metric)


@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_schemes_are_what_they_claim_and_reach_every_tier(metric):
    x, q, S = _scores(metric)
    rank = plain_ranks(S, metric)
    got = {"direct": set(), "bound": set(), "scan": False}
    for name in SCHEMES:
        scale, bias = burst_scheme(name, S, metric)
        m_adj = int((~plain_rows(scale, bias)).sum())
        assert m_adj == {"none": 0, "sparse": 12, "flood": 60, "ties": 40}.get(name, N)
        for k in KS:
            for depth in [(0, 0), (16, 64), (k, k), (16, 256), (200, 250)]:
                first, limit = resolve_depth(k, m_adj, *depth)
                st, where = adjust_need(x, q, scale, bias, k, metric, first, limit)
                assert st["first"] + st["deeper"] + st["scan"] == q.shape[0]
                if st["tier"] in got:
                    got[st["tier"]] |= {w for w in where if w < 2}
                got["scan"] |= st["scan"] > 0
    assert got == {"direct": {0, 1}, "bound": {0, 1}, "scan": True}
    # sparse: six of its rows are far from the top of every query's ranking (no row of this corpus ranks
    # below 200 for all eight queries: the farthest reaches 116), yet enter every top 10
    scale, bias = burst_scheme("sparse", S, metric)
    far = far_rows(S, metric)
    assert rank[:, far].min() >= 100
    _, I, _ = adjust_reference(x, q, scale, bias, 10, metric)
    assert all(set(far.tolist()) <= set(row.tolist()) for row in I)
    # for one query alone such rows exist: ranked below 200, lifted into its top 10
    low = np.flatnonzero(rank[0] >= 200)[:6]
    b1 = np.zeros((N,), np.float32)
    b1[low] = bias[far]
    _, I1, _ = adjust_reference(x, q[:1], np.ones((N,), np.float32), b1, 10, metric)
    assert set(low.tolist()) <= set(I1[0].tolist())
    # ties: more rows tie on A than k, the lowest ids win
    scale, bias = burst_scheme("ties", S, metric)
    D, I, _ = adjust_reference(x, q, scale, bias, 10, metric)
    tied = np.flatnonzero(scale == 0)
    assert tied.shape[0] == 40 and all(row.tolist() == tied[:10].tolist() for row in I) and np.unique(D).shape[0] == 1
    # mixed_scale under the depth (200, 250): the BOUND certificate sees a negative S_L (inner product)
    if metric == "ip":
        assert all(np.sort(S[qi])[::-1][199] < 0 for qi in range(q.shape[0]))


# ---- VectorStore.search_hybrid on the oracle index -------------------------------------------------------
def _store(tmp_path, monkeypatch, metric="cosine", n=N):
    from photo_search_engine_amd import vector_store as vsmod
    monkeypatch.setattr(vsmod, "_index_factory", oracle_adjust_factory)
    x, q = burst_corpus()
    meta = [{"photo_path": f"/p/{i}.jpg", "year": 2019 + i % 6} for i in range(n)]
    store = vsmod.VectorStore(dimension=D_, index_path=str(tmp_path / "idx"), metadata_path=str(tmp_path / "meta.json"),
                              metric=metric, index_type="flat")
    store.add(np.array(x[:n]), meta)
    return store, q, meta


def hybrid_case(store, q, meta, far_count=4):
    """A hybrid query over ``store``: keyword hits on photos far down the vector ranking (and on paths the
    store does not hold), boosts by path and by predicate; returns the arguments and the brute-force pages."""
    n = len(meta)
    xs = store.index._x
    query = store._normalize_query(q[0].tolist())[0]
    D = O.canon_scores(xs, query.reshape(1, -1), "ip")[0]
    order = np.lexsort((np.arange(n), -D))
    paths = [m["photo_path"] for m in meta]
    kw = {paths[order[-1 - j]]: 0.95 - 0.1 * j for j in range(far_count)}  # the worst vector hits
    kw[paths[order[3]]] = 0.1      # a weak keyword hit pulls a good vector hit down
    kw["/nowhere/else.jpg"] = 1.0  # ignored
    by_path = {paths[order[n // 2]]: 1.8, paths[order[1]]: 0.5, "/nowhere/else.jpg": 3.0}
    return xs, query, paths, kw, by_path


def check_hybrid(store, q, meta, top_k=10):
    xs, query, paths, kw, by_path = hybrid_case(store, q, meta)
    n = len(meta)
    pred = lambda m: 1.25 if m["year"] == 2021 else 1.0  # noqa: E731
    cases = [(None, lambda row: 1.0, None), (by_path, lambda row: by_path.get(paths[row], 1.0), None),
             (pred, lambda row: pred(meta[row]), None),
             (by_path, lambda row: by_path.get(paths[row], 1.0), lambda m: m["year"] != 2020)]
    for boosts, boost_of_row, allowed in cases:
        for wv, wk in ((0.8, 0.2), (0.5, 0.5)):
            mask = None if allowed is None else [allowed(m) for m in meta]
            want = hybrid_reference(xs, query, paths, kw, boost_of_row, wv, wk, top_k, mask)
            got = store.search_hybrid(q[0].tolist(), top_k, kw, vector_weight=wv, keyword_weight=wk, boosts=boosts,
                                      allowed=allowed)
            assert [(meta.index(r["metadata"]), r["score"], r["vector_score"], r["keyword_score"]) for r in got] == want
    # the keyword hits from the bottom of the vector ranking made the page
    got = store.search_hybrid(q[0].tolist(), top_k, kw, vector_weight=0.2, keyword_weight=0.8)
    D = O.canon_scores(xs, query.reshape(1, -1), "ip")[0]
    worst = int(np.lexsort((np.arange(n), -D))[-1])
    assert worst in [meta.index(r["metadata"]) for r in got]
    return kw


def test_store_search_hybrid_equals_the_brute_force_fusion(tmp_path, monkeypatch):
    store, q, meta = _store(tmp_path, monkeypatch)
    kw = check_hybrid(store, q, meta)
    # no hits and no boosts: the plain page, score == vector_score
    plain = store.search(q[0].tolist(), 10)
    page = store.search_hybrid(q[0].tolist(), 10, {})
    assert [r["metadata"] for r in page] == [r["metadata"] for r in plain]
    assert all(r["score"] == r["vector_score"] == (p["distance"] + 1.0) / 2.0 and r["keyword_score"] is None
               for r, p in zip(page, plain))
    # the clamp
    assert len(store.search_hybrid(q[0].tolist(), 1000, kw)) == N


def test_store_search_hybrid_adjusts_only_hits_and_boosted_rows(tmp_path, monkeypatch):
    store, q, meta = _store(tmp_path, monkeypatch)
    made = []
    real = store.index.score_adjust_sparse

    def spy(ids, scale=None, bias=None):
        adj = real(ids, scale, bias)
        made.append((np.asarray(ids).tolist(), adj.count))
        return adj

    monkeypatch.setattr(store.index, "score_adjust_sparse", spy)
    kw = {"/p/7.jpg": 0.9, "/p/9.jpg": 0.4, "/gone.jpg": 0.7}
    store.search_hybrid(q[0].tolist(), 5, kw, boosts={"/p/9.jpg": 2.0, "/p/100.jpg": 1.5, "/p/101.jpg": 1.0})
    assert made == [([7, 9, 100], 3)]  # unknown paths and a boost of exactly 1 adjust nothing
    store.search_hybrid(q[0].tolist(), 5, {"/gone.jpg": 0.7})
    assert made[-1] == ([], 0)
    store.search_hybrid(q[0].tolist(), 5, {}, boosts=lambda m: 1.0)
    assert made[-1] == ([], 0)


def test_store_search_hybrid_value_errors(tmp_path, monkeypatch):
    store, q, meta = _store(tmp_path, monkeypatch)
    l2, _, _ = _store(tmp_path / "l2", monkeypatch, metric="l2", n=16)
    with pytest.raises(ValueError):
        l2.search_hybrid(q[0].tolist(), 5, {})
    for bad in ({"vector_weight": -0.1}, {"keyword_weight": float("nan")}, {"boosts": {"/p/1.jpg": -1.0}},
                {"boosts": {"/p/1.jpg": float("inf")}}, {"boosts": lambda m: -2.0}):
        with pytest.raises(ValueError):
            store.search_hybrid(q[0].tolist(), 5, {"/p/1.jpg": 0.5}, **bad)
    with pytest.raises(ValueError):
        store.search_hybrid(q[0].tolist(), 5, {"/p/1.jpg": float("nan")})
    with pytest.raises(ValueError):
        store.search_hybrid(q[0].tolist()[:-1], 5, {})
    with pytest.raises(ValueError):
        store.search_hybrid(q[0].tolist(), 0, {})


def test_oracle_index_adjust_surface(tmp_path):
    ix = oracle_adjust_factory(D_, "cosine")
    x, q = burst_corpus()
    ix.add(np.array(x))
    rng = np.random.default_rng(2)
    ids = rng.permutation(N)[:30]
    s, b = rng.uniform(0, 2, 30).astype(np.float32), rng.normal(0, 0.2, 30).astype(np.float32)
    sparse = ix.score_adjust_sparse(ids, s, b)
    ds, db = np.ones((N,), np.float32), np.zeros((N,), np.float32)
    ds[ids], db[ids] = s, b
    dense = ix.score_adjust(ds, db)
    assert sparse.count == dense.count == 30 and sparse.rows == N
    for a, c in zip(ix.search_adjusted(q, 10, sparse, return_raw=True), ix.search_adjusted(q, 10, dense, return_raw=True)):
        np.testing.assert_array_equal(a, c)
    for bad in ((np.full((N,), -1.0), None), (None, np.full((N,), np.nan)), (np.full((N,), np.inf), None)):
        with pytest.raises(RuntimeError):
            ix.score_adjust(*bad)
    with pytest.raises(RuntimeError):
        ix.score_adjust_sparse([1, 1], None, [0.5, 0.5])
    with pytest.raises(ValueError):
        ix.score_adjust(np.ones((N - 1,)))
    ix.remove_ids([3])
    with pytest.raises(RuntimeError):
        ix.search_adjusted(q, 10, dense)

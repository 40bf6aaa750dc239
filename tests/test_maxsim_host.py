"""The multi-vector search's reference recipe and the store route, without a GPU: the contract's identities
on ``maxsim_reference``, where ``maxsim_need`` sends a query (first list, deeper list, scan, the row cap), and
``VectorStore.search_multivector`` on the oracle index against explicit loops over all rows."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from oracle_diverse_index import burst_corpus
from oracle_group_index import burst_keys, group_reference
from oracle_maxsim_index import (KEY_PAD, group_codes, maxsim_need, maxsim_reference, oracle_maxsim_factory,
                                 resolve_depth)
from oracle_sel_index import filtered_reference

N, D_ = 256, 72


@functools.lru_cache(maxsize=None)
def _corpus(dtype="f32"):
    x, q = burst_corpus()
    xs = O.round_dtype(x, dtype)
    keys = np.array(burst_keys())
    keys[::11] = -3  # some rows ungrouped, under one repeated negative key
    for a in (xs, keys):
        a.setflags(write=False)
    return xs, q, keys


def _q3(q, m):
    return np.ascontiguousarray(np.stack([np.roll(q, -j, axis=0) for j in range(m)], axis=1))


def maxsim_loops(xs, queries, keys, metric, top_k, allowed=None):
    """``[(key, F, size, [(row, score)] per query)]`` in explicit loops over every row."""
    ip = metric == "ip"
    S = O.canon_scores(xs, np.stack(queries), metric)
    groups = {}
    for row in range(len(keys)):
        if allowed is not None and not allowed[row]:
            continue
        tok = (0, int(keys[row])) if keys[row] >= 0 else (1, row)  # grouped groups by key, then ungrouped rows
        best = groups.setdefault(tok, {"key": int(keys[row]), "size": 0, "best": [None] * len(queries)})
        best["size"] += 1
        for j in range(len(queries)):
            s = S[j, row]
            if best["best"][j] is None or (s > best["best"][j][1] if ip else s < best["best"][j][1]):
                best["best"][j] = (row, s)
    out = []
    for tok, g in groups.items():
        f = g["best"][0][1]
        for j in range(1, len(queries)):
            f = f + g["best"][j][1]
        out.append(((-f if ip else f), tok, g["key"], f, g["size"], g["best"]))
    out.sort(key=lambda t: (t[0], t[1]))
    return [(key, float(f), size, [(row, float(np.float32(s))) for row, s in best]) for _, _, key, f, size, best in out[:top_k]]


@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_reference_identities(metric):
    xs, q, keys = _corpus()
    mask = np.arange(N) % 3 != 0
    for m_ in (None, mask):
        # against explicit loops
        for m in (1, 3, 8):
            q3 = _q3(q, m)
            Ko, F, U, J, Z = maxsim_reference(xs, q3, 300, metric, keys, mask=m_)
            for a in (0, 5):
                want = maxsim_loops(xs, list(q3[a]), keys, metric, 300, m_)
                n = len(want)
                assert (Ko[a, n:] == KEY_PAD).all() and (Z[a, n:] == 0).all() and (J[a, n:] == -1).all()
                assert np.isinf(F[a, n:]).all() and n < 300
                got = [(int(Ko[a, r]), float(F[a, r]), int(Z[a, r]), list(zip(J[a, r].tolist(), U[a, r].tolist()))) for r in range(n)]
                assert got == want
        # m = 1: the grouped search with one row per group (the groups' best scores are distinct here)
        k = 10
        Ko, F, U, J, Z = maxsim_reference(xs, q[:, None, :], k, metric, keys, mask=m_)
        Kg, Dg, Ig, _, Zg, _ = group_reference(xs, q, keys, k, 1, metric, m_)
        np.testing.assert_array_equal(Ko, Kg)
        np.testing.assert_array_equal(F.astype(np.float32), Dg[:, :, 0])
        np.testing.assert_array_equal(J[:, :, 0], Ig[:, :, 0])
        np.testing.assert_array_equal(Z, Zg)
        # every key distinct and m = 1: the plain (filtered) search
        Dp, Ip = filtered_reference(xs, q, np.ones((N,), bool) if m_ is None else m_, k, metric)
        Ko, F, U, J, Z = maxsim_reference(xs, q[:, None, :], k, metric, 3 * np.arange(N), mask=m_)
        np.testing.assert_array_equal(J[:, :, 0], Ip)
        np.testing.assert_array_equal(Ko, 3 * Ip)
        np.testing.assert_array_equal(U[:, :, 0].view(np.uint32), Dp.view(np.uint32))
        # a permutation of the sub-queries permutes D_sub / I_sub; F moves by the order of the additions only
        q3 = _q3(q, 3)
        ref = maxsim_reference(xs, q3, N, metric, keys, mask=m_)
        perm = [2, 0, 1]
        rp = maxsim_reference(xs, q3[:, perm], N, metric, keys, mask=m_)
        for a in range(q3.shape[0]):
            pos = {int(kk): r for r, kk in enumerate(rp[0][a].tolist())}
            ungrouped = rp[0][a] < 0
            for r, kk in enumerate(ref[0][a].tolist()):
                if kk == KEY_PAD or kk < 0:
                    continue
                r2 = pos[kk]
                np.testing.assert_array_equal(rp[2][a, r2], ref[2][a, r][perm])
                np.testing.assert_array_equal(rp[3][a, r2], ref[3][a, r][perm])
                # (either order rounds twice, each time by at most 2^-53 of a partial sum <= sum |M_j|; the
                # fp32 sub-scores stand in for M_j, hence the 1.001)
                bound = 4 * 2.0 ** -53 * 1.001 * float(np.abs(ref[2][a, r].astype(np.float64)).sum())
                assert abs(rp[1][a, r2] - ref[1][a, r]) <= bound and rp[4][a, r2] == ref[4][a, r]
            assert ungrouped.sum() == (ref[0][a] < 0).sum()
    # rows behind the covered ones are no members
    short = maxsim_reference(xs, _q3(q, 2), 10, metric, keys[:200])
    np.testing.assert_array_equal(short[0], maxsim_reference(xs[:200], _q3(q, 2), 10, metric, keys[:200])[0])
    assert short[3].max() < 200
    codes, key_of, G = group_codes(np.array([5, -1, 2, 5, -7]))
    assert codes.tolist() == [1, 2, 0, 1, 3] and key_of.tolist() == [2, 5, -1, -7] and G == 2


def test_need_reaches_the_first_list_a_deeper_list_the_scan_and_the_row_cap():
    xs, q, keys = _corpus()
    q3 = _q3(q, 3)
    k = 5
    first, limit = resolve_depth(k, 3)
    assert (first, limit) == (64, 2730) and resolve_depth(100, 8) == (400, 1024) and resolve_depth(10, 2, 16, 16) == (16, 16)
    st, where = maxsim_need(xs, q3, k, "ip", keys, first, limit)
    assert st["first"] + st["deeper"] + st["scan"] == 8 and st["tier"] == "lists"
    # lists that hold every member complete whatever the bound or the cap says
    st, where = maxsim_need(xs, q3, k, "ip", keys, N, N, walk_rows=1)
    assert where == [0] * 8 and st["longest"] == N
    # a list of one row per sub-query has at most 3 candidates: never k = 5 of them
    st, where = maxsim_need(xs, q3, k, "ip", keys, 1, 1)
    assert where == [2] * 8 and st == {"first": 0, "deeper": 0, "scan": 8, "longest": 1, "tier": "lists"}
    st, where = maxsim_need(xs, q3, k, "ip", keys, 1, 0 or 2730)
    assert st["first"] == 0 and st["deeper"] + st["scan"] == 8 and 1 in where
    # the row cap sends everything on that the lists do not hold entirely, at once: no deeper list is searched
    st, where = maxsim_need(xs, q3, k, "ip", keys, 16, 64, walk_rows=1)
    assert where == [2] * 8 and st == {"first": 0, "deeper": 0, "scan": 8, "longest": 16, "tier": "lists"}
    # the default cap grows with the batch: 400 rows per query of the call, up to 256 queries
    big = np.zeros((N,), dtype=np.int64)  # one group of every row: any candidate is all 256 rows
    assert maxsim_need(xs, q3[:1], 1, "ip", big, 16, 64, walk_rows=255)[1] == [2]
    assert maxsim_need(xs, q3[:1], 1, "ip", big, 16, 64, walk_rows=256)[1] != [2]
    assert maxsim_need(xs, q3[:1], 1, "ip", big, 16, 64)[0] == maxsim_need(xs, q3[:1], 1, "ip", big, 16, 64, walk_rows=400)[0]
    st, where = maxsim_need(xs, q3, k, "ip", keys, 16, 64, tier="scan")
    assert st == {"first": 0, "deeper": 0, "scan": 8, "longest": 0, "tier": "scan"}
    st, where = maxsim_need(xs, q3, k, "ip", keys, 16, 64, mask=np.zeros((N,), bool))
    assert st["first"] == 8 and where == [0] * 8


# ---- VectorStore.search_multivector on the oracle index ------------------------------------------------
def _store(tmp_path, monkeypatch, metric="cosine", n=N, index_type="flat"):
    from photo_search_engine_amd import vector_store as vsmod
    monkeypatch.setattr(vsmod, "_index_factory", oracle_maxsim_factory)
    x, q = burst_corpus()
    meta = [{"photo_path": f"/p/{i}.jpg", "year": 2019 + i % 6} for i in range(n)]
    for i, md in enumerate(meta):
        if i % 9 != 4:
            md["trip"] = f"trip-{(7 * i) % 23}"  # (items without the field are ungrouped)
    store = vsmod.VectorStore(dimension=D_, index_path=str(tmp_path / "idx"), metadata_path=str(tmp_path / "meta.json"),
                              metric=metric, index_type=index_type)
    if n:
        store.add(np.array(x[:n]), meta)
    return store, q, meta


def _check(store, q, meta, metric, group_by, keys, value_of):
    xs = store.index._x
    wordings = [(2.5 * q[0]).tolist(), q[3].tolist(), (0.5 * q[0] + 0.5 * q[5]).tolist()]  # (normalised by the store)
    queries = [store._normalize_query(w)[0] for w in wordings]
    pred = lambda md: md["year"] != 2020  # noqa: E731
    for allowed in (None, pred):
        mask = None if allowed is None else [allowed(md) for md in meta]
        for top_k in (1, 7):
            got = store.search_multivector(wordings, top_k, group_by, allowed=allowed)
            want = maxsim_loops(xs, queries, keys, metric, top_k, mask)
            assert len(got) == len(want) and 1 <= len(got) <= top_k
            for g, (key, f, size, best) in zip(got, want):
                assert set(g) == {"group", "score", "size", "matches"}
                assert g["group"] == (value_of(key) if key >= 0 else None) and g["score"] == f and g["size"] == size
                assert [(meta.index(mt["metadata"]), mt["distance"]) for mt in g["matches"]] == best


def test_store_search_multivector_equals_explicit_loops(tmp_path, monkeypatch):
    store, q, meta = _store(tmp_path, monkeypatch)
    # a field: coded in order of first appearance, ungrouped where it is missing
    values, keys = [], np.empty((N,), dtype=np.int64)
    for i, md in enumerate(meta):
        v = md.get("trip")
        if v is None:
            keys[i] = -1
        else:
            if v not in values:
                values.append(v)
            keys[i] = values.index(v)
    _check(store, q, meta, "ip", "trip", keys, lambda key: values[key])
    _check(store, q, meta, "ip", "trip", keys, lambda key: values[key])  # (the cached keys)
    # a callable
    years = sorted({md["year"] for md in meta}, key=[md["year"] for md in meta].index)
    ykeys = np.asarray([years.index(md["year"]) for md in meta], dtype=np.int64)
    _check(store, q, meta, "ip", lambda md: md["year"], ykeys, lambda key: years[key])
    # a sequence of ints: the keys themselves, negative = ungrouped
    seq = (np.arange(N) % 17).astype(np.int64) * 1000
    seq[::5] = -2
    _check(store, q, meta, "ip", seq, seq, lambda key: key)
    # the clamp, and a filter that leaves fewer groups than top_k
    assert len(store.search_multivector([q[0].tolist(), q[1].tolist()], 100000, seq)) == len(np.unique(seq[seq >= 0])) + int((seq < 0).sum())
    few = store.search_multivector([q[0].tolist(), q[1].tolist()], 10, "trip", allowed=[3, 44, 200])
    assert sum(g["size"] for g in few) == 3 and all(len(g["matches"]) == 2 for g in few)
    l2, _, meta16 = _store(tmp_path / "l2", monkeypatch, metric="l2", n=16)
    k16 = np.arange(16, dtype=np.int64) // 4
    _check(l2, q, meta16, "l2", k16, k16, lambda key: key)
    # an HNSW store answers through the exact flat path
    hn, _, _ = _store(tmp_path / "hnsw", monkeypatch, index_type="hnsw")
    _check(hn, q, meta, "ip", seq, seq, lambda key: key)


def test_store_argument_errors(tmp_path, monkeypatch):
    store, q, meta = _store(tmp_path, monkeypatch)
    two = [q[0].tolist(), q[1].tolist()]
    with pytest.raises(ValueError):
        store.search_multivector([], 5, "trip")
    with pytest.raises(ValueError):
        store.search_multivector([q[0].tolist(), q[1].tolist()[:-1]], 5, "trip")
    with pytest.raises(ValueError):
        store.search_multivector([q[0].tolist()] * 9, 5, "trip")
    with pytest.raises(ValueError):
        store.search_multivector(two, 0, "trip")
    with pytest.raises(ValueError):
        store.search_multivector(two, 5, np.arange(N - 1))
    empty, _, _ = _store(tmp_path / "empty", monkeypatch, n=0)
    assert empty.search_multivector(two, 5, "trip") == []
    with pytest.raises(ValueError):
        empty.search_multivector([], 5, "trip")

    class NoMaxsim:  # a multi-device index has no search_maxsim
        ntotal = N
    store.index = NoMaxsim()
    with pytest.raises(NotImplementedError):
        store.search_multivector(two, 5, "trip")


def test_store_top_k_beyond_the_limit(tmp_path, monkeypatch):
    """``k = min(top_k, ntotal)`` first, then ``ValueError`` beyond ``min(3276, 8192 // m)``: 1024 at 8 embeddings."""
    from photo_search_engine_amd import vector_store as vsmod
    monkeypatch.setattr(vsmod, "_index_factory", oracle_maxsim_factory)
    rng = np.random.default_rng(2)
    n, d = 1100, 8
    store = vsmod.VectorStore(dimension=d, index_path=str(tmp_path / "idx"), metadata_path=str(tmp_path / "meta.json"),
                              metric="cosine", index_type="flat")
    store.add(rng.standard_normal((n, d)).astype(np.float32), [{"photo_path": f"/p/{i}.jpg"} for i in range(n)])
    eight = rng.standard_normal((8, d)).tolist()
    keys = np.arange(n, dtype=np.int64)
    assert len(store.search_multivector(eight, 1024, keys)) == 1024
    with pytest.raises(ValueError):
        store.search_multivector(eight, 1025, keys)
    assert len(store.search_multivector(eight[:2], 5000, keys)) == n  # (clamped to ntotal, below 3276)


def test_oracle_index_maxsim_surface():
    ix = oracle_maxsim_factory(D_, "cosine")
    xs, q, keys = _corpus()
    ix.add(np.array(xs))
    groups = ix.group_keys(keys)
    q3 = _q3(q, 3)
    res = ix.search_maxsim(q3, 10, groups)
    for g, w in zip(res, maxsim_reference(xs, q3, 10, "ip", keys)):
        np.testing.assert_array_equal(g, w)
    assert res.scores.dtype == np.float64 and res.sub_scores.shape == (8, 10, 3) and len(tuple(res)) == 5
    sel = ix.selector(np.arange(N) % 3 != 0)
    for g, w in zip(ix.search_maxsim(q3, 10, groups, sel=sel), maxsim_reference(xs, q3, 10, "ip", keys, mask=np.arange(N) % 3 != 0)):
        np.testing.assert_array_equal(g, w)
    for bad in (q, q3[:, :, :-1], np.zeros((2, 9, D_), np.float32), np.zeros((2, 0, D_), np.float32)):
        with pytest.raises(ValueError):
            ix.search_maxsim(bad, 5, groups)
    with pytest.raises(RuntimeError):
        ix.search_maxsim(_q3(q, 8), 1025, groups)
    ix.remove_ids([3])
    with pytest.raises(RuntimeError):
        ix.search_maxsim(q3, 5, groups)

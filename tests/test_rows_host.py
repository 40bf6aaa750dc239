"""Host side of the queries taken from stored rows (CPU only): the wrappers' argument handling, the
host forms of the self filters (the multi-device route), the recipes themselves, and
``VectorStore.search_similar`` / ``duplicate_pairs`` / ``find_duplicates`` over a checker-backed index
(tests/oracle_rows_index.py).  The HIP path is held to the same recipes bit for bit in
tests/test_gpu_rows.py."""
import numpy as np
import pytest

from oracle import oracle as O
from oracle_range_index import range_reference
from oracle_rows_index import oracle_rows_factory, rows_range_reference, rows_topk_reference
from photo_search_engine_amd import index as idxmod
from photo_search_engine_amd import vector_store as vsmod


# ---- wrappers ---------------------------------------------------------------------------------------
def test_row_ids_and_wrapper_validation_come_before_any_library_call():
    assert idxmod.row_ids([3, 1, 3], 5).tolist() == [3, 1, 3] and idxmod.row_ids([], 5).shape == (0,)
    assert idxmod.row_ids(np.array([2, 0], dtype=np.int32), 5).dtype == np.int64
    for bad in ([[1, 2]], [0.5], np.zeros((2, 2), dtype=np.int64)):
        with pytest.raises(ValueError):
            idxmod.row_ids(bad, 5)
    ix = idxmod.FlatIndex.__new__(idxmod.FlatIndex)
    ix.d, ix._h, ix._L = 8, None, None
    with pytest.raises(ValueError):
        ix.range_search_rows(0.5, ids=[0], self_mode="below")
    with pytest.raises(ValueError):
        ix.range_search_rows(0.5, ids=[0], max_total=0)
    mi = idxmod.MultiDeviceFlatIndex.__new__(idxmod.MultiDeviceFlatIndex)
    mi.d, mi._h, mi._L, mi._prune_copy = 8, None, None, None
    with pytest.raises(ValueError):
        mi.range_search_rows(0.5, ids=[0], self_mode="below")
    with pytest.raises(ValueError):
        mi.range_search_rows(0.5, ids=[0], max_total=-1)


@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_host_self_filters_equal_the_recipes(metric):
    """``drop_self_topk`` / ``filter_range_self`` (the multi-device route: unfiltered search, host
    filter) give what the recipes give."""
    rng = np.random.default_rng(7)
    n, d = 200, 16
    x = rng.standard_normal((n, d)).astype(np.float32)
    x[40] = x[9]
    x[150] = x[9]
    ids = np.array([150, 9, 40, 3, 150], dtype=np.int64)
    mt = 0 if metric == "ip" else 1
    for k in (1, 5, n - 1, n + 4):
        S, I = O.knn_exact(x, x[ids], min(k + 1, n), metric)
        D2, I2 = idxmod.drop_self_topk(S.astype(np.float32), I, ids, k, mt)
        Dr, Ir = rows_topk_reference(x, ids, k, metric)
        np.testing.assert_array_equal(I2, Ir)
        np.testing.assert_array_equal(D2, Dr)
    radius = np.float32(0.5 if metric == "ip" else 30.0)
    full = range_reference(x, x[ids], radius, metric)
    for mode in ("keep", "drop", "above"):
        got = idxmod.filter_range_self(*full, ids, idxmod.SELF_MODES[mode])
        want = rows_range_reference(x, ids, radius, metric, self_mode=mode)
        for g, w in zip(got, want):
            np.testing.assert_array_equal(g, w)


# ---- the recipes ------------------------------------------------------------------------------------------
def test_topk_recipe_drops_by_id_not_by_position():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((50, 8)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    x[30] = x[4]
    D, I = rows_topk_reference(x, [30, 4], 3, "ip")
    assert I[0, 0] == 4 and 30 not in I[0] and I[1, 0] == 30 and 4 not in I[1]
    Dk, Ik = rows_topk_reference(x, [30], 3, "ip", drop_self=False)
    assert Ik[0, :2].tolist() == [4, 30] and Dk[0, 0] == Dk[0, 1]
    # a row that is not among its own k + 1 best (inner product, a short row): the first k stand
    x[7] *= 1e-3
    S, Ie = O.knn_exact(x, x[7:8], 4, "ip")
    assert 7 not in Ie[0]
    D, I = rows_topk_reference(x, [7], 3, "ip")
    assert I[0].tolist() == Ie[0, :3].tolist()
    # k beyond the rows: everything but the row, then padding
    D, I = rows_topk_reference(x, [0], 60, "ip")
    assert (I[0, :49] >= 0).all() and 0 not in I[0] and (I[0, 49:] == -1).all()


def test_range_recipe_above_is_half_of_drop():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((80, 8)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    la, Da, Ia = rows_range_reference(x, None, 0.3, "ip", self_mode="above")
    ld, Dd, Id = rows_range_reference(x, None, 0.3, "ip", self_mode="drop")
    lk, _, _ = rows_range_reference(x, None, 0.3, "ip", self_mode="keep")
    assert la[-1] > 0 and ld[-1] == 2 * la[-1] and lk[-1] == ld[-1] + 80
    qa = np.repeat(np.arange(80), np.diff(la))
    qd = np.repeat(np.arange(80), np.diff(ld))
    assert (Ia > qa).all()
    assert set(zip(qa.tolist(), Ia.tolist())) == {(i, j) for i, j in zip(qd.tolist(), Id.tolist()) if i < j}


# ---- VectorStore ------------------------------------------------------------------------------------------
@pytest.fixture
def VS(monkeypatch):
    monkeypatch.setattr(vsmod, "_index_factory", oracle_rows_factory)
    return vsmod.VectorStore


def _store(VS, tmp_path, metric, n=120, d=24, seed=3, X=None):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d)).astype(np.float32) if X is None else X
    store = VS(dimension=X.shape[1], index_path=str(tmp_path / "idx"), metadata_path=str(tmp_path / "meta.json"),
               metric=metric)
    store.add(X, [{"photo_path": f"/p/{i}.jpg", "year": 2020 + i % 5} for i in range(X.shape[0])])
    return store


@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_search_similar_is_search_of_the_stored_row_minus_the_photo(VS, tmp_path, metric):
    store = _store(VS, tmp_path, metric)
    store.add_item(store.index.reconstruct(17).tolist(), {"photo_path": "/p/copy.jpg", "year": 2021})  # a twin of 17
    for i, k in ((17, 1), (17, 10), (120, 5), (0, 119)):
        path = store.metadata[i]["photo_path"]
        D, I = store.index.search(store.index.reconstruct(i).reshape(1, -1), k + 1)
        want = [{"metadata": store.metadata[j], "distance": float(dist)}
                for dist, j in zip(D[0].tolist(), I[0].tolist()) if j != i][:k]
        got = store.search_similar(path, k)
        assert got == want and len(got) == k
        assert all(r["metadata"]["photo_path"] != path for r in got)
    assert store.search_similar("/p/copy.jpg", 1)[0]["metadata"]["photo_path"] == "/p/17.jpg"  # the lower-id twin stays


def test_search_similar_guards(VS, tmp_path):
    store = _store(VS, tmp_path, "cosine", n=15)
    with pytest.raises(ValueError):
        store.search_similar("/p/nope.jpg", 3)
    assert len(store.search_similar("/p/3.jpg", 15)) == 14  # top_k >= ntotal: clamped to ntotal - 1
    assert len(store.search_similar("/p/3.jpg", 1000)) == 14
    assert store.search_similar("/p/3.jpg", 0) == []
    empty = VS(dimension=24, index_path=str(tmp_path / "e"), metadata_path=str(tmp_path / "em"))
    assert empty.search_similar("/p/3.jpg", 3) == []  # the empty-store guard comes first
    assert empty.find_duplicates(0.9) == [] and empty.duplicate_pairs(0.9)[0].shape == (0,)
    one = _store(VS, tmp_path / "one", "cosine", n=1)
    assert one.search_similar("/p/0.jpg", 3) == []


def _chain_rows(rng, d=24):
    """Unit rows with a planted chain a-b, b-c whose ends a, c are further apart than the links."""
    X = rng.standard_normal((60, d)).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    e = np.zeros((3, d), dtype=np.float32)
    t = 0.25  # angle between neighbours of the chain: cos t = 0.969, cos 2t = 0.878
    e[0, 0], e[1, :2], e[2, :2] = 1.0, (np.cos(t), np.sin(t)), (np.cos(2 * t), np.sin(2 * t))
    X[[5, 41, 22]] = e  # a = 5, b = 41, c = 22
    X[50] = X[33]       # and an exact duplicate pair
    return X


def test_duplicate_pairs_and_groups_on_a_planted_chain(VS, tmp_path):
    X = _chain_rows(np.random.default_rng(9))
    store = _store(VS, tmp_path, "cosine", X=X)
    i, j, dist = store.duplicate_pairs(0.95)
    pairs = list(zip(i.tolist(), j.tolist()))
    assert (i < j).all() and len(set(pairs)) == len(pairs)
    assert set(pairs) == {(5, 41), (22, 41), (33, 50)}  # a-c (cos 0.878) is below the threshold
    for a, b, dd in zip(i.tolist(), j.tolist(), dist.tolist()):
        D, I = store.index.search(store.index.reconstruct(a).reshape(1, -1), 60)
        assert dd == float(D[0][I[0].tolist().index(b)])  # the distance search reports
    assert store.find_duplicates(0.95) == [[5, 22, 41], [33, 50]]
    assert store.find_duplicates(0.999) == [[33, 50]]
    assert store.find_duplicates(0.87) == [[5, 22, 41], [33, 50]]
    with pytest.raises(Exception, match="found 3 results"):
        store.duplicate_pairs(0.95, max_pairs=2)


def test_duplicates_l2_and_allowed_restricts_both_sides(VS, tmp_path):
    X = _chain_rows(np.random.default_rng(9))
    store = _store(VS, tmp_path, "l2", X=X)
    assert store.find_duplicates(0.1) == [[5, 22, 41], [33, 50]]  # squared distances: 0.062 link, 0.245 ends
    # a predicate that leaves b out: the chain falls apart, the exact pair stays
    allowed = lambda m: m["photo_path"] != "/p/41.jpg"  # noqa: E731
    assert store.find_duplicates(0.1, allowed=allowed) == [[33, 50]]
    i, j, _ = store.duplicate_pairs(0.1, allowed=[5, 41, 33])
    assert list(zip(i.tolist(), j.tolist())) == [(5, 41)]
    mask = np.zeros(60, dtype=bool)
    mask[[22, 41, 50]] = True
    assert store.find_duplicates(0.1, allowed=mask) == [[22, 41]]
    assert store.find_duplicates(0.1, allowed=[7]) == []
    # search_similar under a predicate: only allowed items, the photo itself out even when allowed
    got = store.search_similar("/p/41.jpg", 3, allowed=lambda m: m["year"] == 2021)
    assert len(got) == 3 and all(r["metadata"]["year"] == 2021 for r in got)
    assert all(r["metadata"]["photo_path"] != "/p/41.jpg" for r in got)  # (41 % 5 == 1: it is allowed)
    D, I = store.index.search(store.index.reconstruct(41).reshape(1, -1), 4, sel=lambda_mask(store, 2021))
    assert [r["metadata"]["photo_path"] for r in got] == [f"/p/{j}.jpg" for j in I[0].tolist() if j != 41][:3]


def lambda_mask(store, year):
    return np.array([m["year"] == year for m in store.metadata])

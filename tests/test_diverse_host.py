"""Host side of the diversified search (CPU only): the recipe itself on hand-made cases, the symmetry
of the pair score it rests on, and ``VectorStore.search_diverse`` over a checker-backed index
(tests/oracle_diverse_index.py).  The HIP path is held to the same recipe bit for bit in
tests/test_gpu_diverse.py."""
import numpy as np
import pytest

from oracle import oracle as O
from oracle_diverse_index import burst_corpus, diverse_reference, oracle_diverse_factory
from photo_search_engine_amd import index as idxmod
from photo_search_engine_amd import vector_store as vsmod


# ---- the recipe -------------------------------------------------------------------------------------------
def _plane_rows(angles_deg, d=8):
    x = np.zeros((len(angles_deg), d), dtype=np.float32)
    a = np.deg2rad(np.asarray(angles_deg, dtype=np.float64))
    x[:, 0] = np.cos(a)
    x[:, 1] = np.sin(a)
    return x


def test_chain_is_not_transitive_the_walk_order_decides():
    """Unit rows at 0, 20 and 40 degrees, threshold cos 25: 0-20 and 20-40 are near, 0-40 is not.  The
    walk accepts 0, hides 20 under it, and accepts 40 (it is near no ACCEPTED row)."""
    x = _plane_rows([0.0, 20.0, 40.0])
    q = _plane_rows([0.0])
    r = np.float32(np.cos(np.deg2rad(25.0)))
    D, I, hidden, examined = diverse_reference(x, q, 3, r, "ip")
    assert I[0].tolist() == [0, 2, -1]
    assert hidden[0].tolist() == [1, 0, 0]
    assert examined[0] == 3
    assert D[0, 0] == np.float32(O.canon_scores(x[[0]], q, "ip")[0, 0]) and D[0, 2] == -np.float32(3.4028235e38)
    # the same under L2 (|a - b|^2 = 2 - 2 cos)
    D, I, hidden, examined = diverse_reference(x, q, 3, np.float32(2.0 - 2.0 * float(r)), "l2")
    assert I[0].tolist() == [0, 2, -1] and hidden[0].tolist() == [1, 0, 0] and examined[0] == 3
    # walking from the middle: 20 takes both ends
    D, I, hidden, examined = diverse_reference(x, _plane_rows([20.0]), 3, r, "ip")
    assert I[0].tolist() == [1, -1, -1] and hidden[0].tolist() == [2, 0, 0] and examined[0] == 3


def test_recipe_stops_at_k_and_counts_what_it_examined():
    x, q = burst_corpus()
    for metric, r in (("ip", 0.9), ("l2", 0.2)):
        D, I, hidden, examined = diverse_reference(x, q, 10, r, metric)
        S, Ik = O.knn_exact(x, q, 10, metric)
        assert (I >= 0).all() and ((I != Ik).any(axis=1)).all()  # every query differs from the plain top-10
        np.testing.assert_array_equal(hidden.sum(axis=1) + 10, examined)
        assert examined.min() > 10
        D2, I2, _, ex2 = diverse_reference(x, q, 2, r, metric)
        np.testing.assert_array_equal(I2, I[:, :2])  # prefix-stable
        assert (ex2 <= examined).all()
        D60, I60, h60, ex60 = diverse_reference(x, q, 60, r, metric)
        assert ((I60 >= 0).sum(axis=1) == 40).all() and (ex60 == 256).all()  # one per burst, ranking exhausted
        np.testing.assert_array_equal(h60.sum(axis=1) + 40, ex60)
    # infinite radii: nothing near = the plain search; everything near = the top row alone
    D, I, hidden, examined = diverse_reference(x, q, 10, np.inf, "ip")
    S, Ik = O.knn_exact(x, q, 10, "ip")
    np.testing.assert_array_equal(I, Ik)
    np.testing.assert_array_equal(D, S.astype(np.float32))
    assert (hidden == 0).all() and (examined == 10).all()
    D, I, hidden, examined = diverse_reference(x, q, 10, -np.inf, "ip")
    np.testing.assert_array_equal(I[:, 0], Ik[:, 0])
    assert (I[:, 1:] == -1).all() and (hidden[:, 0] == 255).all() and (examined == 256).all()
    # a mask restricts the members
    mask = np.arange(256) % 3 != 0
    D, I, hidden, examined = diverse_reference(x, q, 60, 0.9, "ip", mask)
    assert (I[I >= 0] % 3 != 0).all() and (examined == int(mask.sum())).all()


@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_pair_score_is_symmetric_bit_for_bit(dtype, metric):
    x, _ = burst_corpus()
    xs = O.round_dtype(x, dtype)
    S = O.canon_scores(xs, xs, metric)
    np.testing.assert_array_equal(S.view(np.uint64), S.T.copy().view(np.uint64))


# ---- wrappers ---------------------------------------------------------------------------------------------
def test_wrapper_validation_comes_before_any_library_call():
    ix = idxmod.FlatIndex.__new__(idxmod.FlatIndex)
    ix.d, ix._h, ix._L = 8, None, None
    with pytest.raises(ValueError):
        ix.search_diverse(np.zeros((2, 7), dtype=np.float32), 3, 0.5)
    with pytest.raises(ValueError):
        ix.search_diverse(np.zeros((2, 8), dtype=np.float32), 3, [0.5, 0.5, 0.5])
    with pytest.raises(ValueError):
        ix.search_diverse(np.zeros((2, 8), dtype=np.float32), 3, np.nan)
    res = idxmod.DiverseResult(1, 2, 3, 4)
    assert tuple(res) == (1, 2, 3, 4) and res.hidden == 3


# ---- VectorStore ------------------------------------------------------------------------------------------
@pytest.fixture
def VS(monkeypatch):
    monkeypatch.setattr(vsmod, "_index_factory", oracle_diverse_factory)
    return vsmod.VectorStore


def _store(VS, tmp_path, metric, X):
    store = VS(dimension=X.shape[1], index_path=str(tmp_path / "idx"), metadata_path=str(tmp_path / "meta.json"),
               metric=metric)
    store.add(X, [{"photo_path": f"/p/{i}.jpg", "year": 2020 + i % 5} for i in range(X.shape[0])])
    return store


@pytest.mark.parametrize("metric,threshold", [("cosine", 0.9), ("l2", 0.2)])
def test_store_search_diverse_result_dicts_and_allowed_forms(VS, tmp_path, metric, threshold):
    x, q = burst_corpus()
    store = _store(VS, tmp_path, metric, np.array(x))
    xs = store.index.reconstruct_n(0, 256)
    m = "ip" if metric == "cosine" else "l2"
    qn = store._normalize_query(q[0].tolist())
    D, I, hidden, _ = diverse_reference(xs, qn, 10, threshold, m)
    got = store.search_diverse(q[0].tolist(), 10, threshold)
    assert got == [{"metadata": store.metadata[i], "distance": float(dist), "similar_hidden": int(h)}
                   for dist, i, h in zip(D[0].tolist(), I[0].tolist(), hidden[0].tolist())]
    assert len(got) == 10 and sum(g["similar_hidden"] for g in got) > 0
    assert [g["metadata"] for g in got] != [r["metadata"] for r in store.search(q[0].tolist(), 10)]
    # the allowed forms: mask, ids, predicate, selector -- one answer
    mask = np.arange(256) % 3 != 0
    Dm, Im, hm, _ = diverse_reference(xs, qn, 10, threshold, m, mask)
    want = [{"metadata": store.metadata[i], "distance": float(dist), "similar_hidden": int(h)}
            for dist, i, h in zip(Dm[0].tolist(), Im[0].tolist(), hm[0].tolist()) if i != -1]
    for allowed in (mask, np.flatnonzero(mask), lambda md: int(md["photo_path"][3:-4]) % 3 != 0, store.selector(mask)):
        assert store.search_diverse(q[0].tolist(), 10, threshold, allowed=allowed) == want
    assert all(int(g["metadata"]["photo_path"][3:-4]) % 3 != 0 for g in want)


def test_store_search_diverse_guards_and_clamp(VS, tmp_path):
    x, q = burst_corpus()
    store = _store(VS, tmp_path, "cosine", np.array(x[:30]))
    got = store.search_diverse(q[0].tolist(), 1000, 0.9)  # top_k beyond ntotal: clamped, then the ranking runs out
    xs = store.index.reconstruct_n(0, 30)
    D, I, hidden, examined = diverse_reference(xs, store._normalize_query(q[0].tolist()), 30, 0.9, "ip")
    assert [g["metadata"]["photo_path"] for g in got] == [f"/p/{i}.jpg" for i in I[0].tolist() if i != -1]
    assert len(got) + sum(g["similar_hidden"] for g in got) == 30 == examined[0]
    with pytest.raises(ValueError):
        store.search_diverse(q[0, :10].tolist(), 3, 0.9)  # dimension
    assert store.search_diverse(q[0].tolist(), 5, 0.9, allowed=np.zeros((30,), dtype=bool)) == []
    empty = VS(dimension=72, index_path=str(tmp_path / "e"), metadata_path=str(tmp_path / "em"))
    assert empty.search_diverse(q[0].tolist(), 3, 0.9) == []
    assert empty.search_diverse(q[0, :10].tolist(), 3, 0.9) == []  # the empty-store guard comes first

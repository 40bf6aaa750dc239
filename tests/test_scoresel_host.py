"""Score selectors without a GPU: the recipe's identities, the wrappers' argument checks, and
``VectorStore.similar_to`` / ``similar_to_items`` over the oracle index."""
import numpy as np
import pytest

from oracle import oracle as O
from oracle_diverse_index import burst_corpus
from oracle_range_index import range_reference
from oracle_scoresel_index import oracle_scoresel_factory, scoresel_reference
from photo_search_engine_amd import index as idxmod

N, D_ = 256, 72


@pytest.fixture(scope="module")
def corpus():
    x, q = burst_corpus()
    return O.round_dtype(x, "bf16"), q[:5]


def _lists(xs, q, r, metric):
    lims, _, I = range_reference(xs, q, r, metric)
    return [set(I[lims[i]:lims[i + 1]].tolist()) for i in range(q.shape[0])]


# ---- the recipe --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_reference_identities(corpus, metric):
    xs, q = corpus
    S, _ = O.knn_exact(xs, q, 120, metric)
    r = S[:, 119].astype(np.float32)
    lists = _lists(xs, q, r, metric)
    union, inter = set.union(*lists), set.intersection(*lists)
    assert 0 < len(inter) < len(union) < N  # (the case tells the modes apart)
    mask = np.arange(N) % 3 != 0
    for m in (None, mask):
        member = np.ones(N, dtype=bool) if m is None else m
        for mode, rows in (("any", union), ("all", inter)):
            want = np.zeros(N, dtype=bool)
            want[sorted(rows)] = True
            got = scoresel_reference(xs, q, r, metric, mode, False, m)
            np.testing.assert_array_equal(got, want & member)
            neg = scoresel_reference(xs, q, r, metric, mode, True, m)
            np.testing.assert_array_equal(neg, member & ~want)  # the complement within the members
            assert not (got & neg).any() and ((got | neg) == member).all()


@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_reference_infinite_radii_and_no_query(corpus, metric):
    xs, q = corpus
    mask = np.arange(N) % 4 == 1
    every = np.float32(-np.inf if metric == "ip" else np.inf)
    for mode in ("any", "all"):
        assert scoresel_reference(xs, q, every, metric, mode).all()
        np.testing.assert_array_equal(scoresel_reference(xs, q, every, metric, mode, mask=mask), mask)
        assert not scoresel_reference(xs, q, every, metric, mode, True, mask).any()
        assert not scoresel_reference(xs, q, -every, metric, mode).any()
        np.testing.assert_array_equal(scoresel_reference(xs, q, -every, metric, mode, True, mask), mask)
    # one query passes everything, the others nothing: ANY everything, ALL nothing
    r = np.full((q.shape[0],), -every, dtype=np.float32)
    r[2] = every
    assert scoresel_reference(xs, q, r, metric, "any").all()
    assert not scoresel_reference(xs, q, r, metric, "all").any()
    # nq = 0: ANY passes nothing, ALL everything
    none = np.zeros((0, D_), dtype=np.float32)
    r0 = np.zeros((0,), dtype=np.float32)
    assert not scoresel_reference(xs, none, r0, metric, "any").any()
    assert scoresel_reference(xs, none, r0, metric, "all").all()
    np.testing.assert_array_equal(scoresel_reference(xs, none, r0, metric, "any", True, mask), mask)
    assert not scoresel_reference(xs, none, r0, metric, "all", True, mask).any()


def test_reference_mask_shorter_than_the_index(corpus):
    xs, q = corpus
    short = np.ones(200, dtype=bool)
    short[::2] = False
    for negate in (False, True):
        got = scoresel_reference(xs, q, np.float32(-np.inf), "ip", "any", negate, short)
        assert got.shape == (N,) and not got[200:].any()  # rows behind the mask are no members
        np.testing.assert_array_equal(got[:200], np.zeros(200, dtype=bool) if negate else short)


# ---- the wrappers ------------------------------------------------------------------------------------------
def test_wrappers_validate_before_any_library_call():
    """The argument checks of ``selector_from_range`` / ``_rows`` come before the handle is touched."""
    ix = idxmod.FlatIndex.__new__(idxmod.FlatIndex)
    ix.d, ix._h, ix._L = 8, None, None
    q = np.zeros((2, 8), dtype=np.float32)
    with pytest.raises(ValueError):
        ix.selector_from_range(np.zeros((2, 7), dtype=np.float32), 0.0)
    with pytest.raises(ValueError):
        ix.selector_from_range(q, [0.0, 1.0, 2.0])
    with pytest.raises(ValueError):
        ix.selector_from_range(q, np.nan)
    with pytest.raises(ValueError):
        ix.selector_from_range(q, 0.0, mode="most")
    with pytest.raises(ValueError):
        ix.selector_from_range_rows([[1, 2]], 0.0)
    with pytest.raises(ValueError):
        ix.selector_from_range_rows([1.5], 0.0)
    with pytest.raises(ValueError):
        ix.selector_from_range_rows([1, 2], [0.0])
    with pytest.raises(ValueError):
        ix.selector_from_range_rows([1, 2], np.nan)
    with pytest.raises(ValueError):
        ix.selector_from_range_rows([1, 2], 0.0, mode="none")
    with pytest.raises(ValueError):
        idxmod.set_scoresel_staging_bytes(0)
    mi = idxmod.MultiDeviceFlatIndex.__new__(idxmod.MultiDeviceFlatIndex)
    mi.d, mi._h, mi._L, mi._prune_copy = 8, None, None, None
    with pytest.raises(ValueError):
        mi.selector_from_range(np.zeros((2, 7), dtype=np.float32), 0.0)
    with pytest.raises(ValueError):
        mi.selector_from_range(q, [0.0])
    with pytest.raises(ValueError):
        mi.selector_from_range(q, 0.0, mode="most")
    with pytest.raises(ValueError):
        mi.selector_from_range_rows([1, 2], [0.0])


def test_mask_selector_to_mask():
    s = idxmod.MaskSelector(11, [0, 3, 10])
    assert s.to_mask().tolist() == [i in (0, 3, 10) for i in range(11)] and s.count == 3


# ---- the store ---------------------------------------------------------------------------------------------
def _store(tmp_path, monkeypatch, metric):
    from photo_search_engine_amd import vector_store as vsmod
    monkeypatch.setattr(vsmod, "_index_factory", oracle_scoresel_factory)
    x, q = burst_corpus()
    meta = [{"photo_path": f"/p/{i}.jpg", "year": 2019 + i % 6} for i in range(N)]
    store = vsmod.VectorStore(dimension=D_, index_path=str(tmp_path / "idx"), metadata_path=str(tmp_path / "meta.json"),
                              metric=metric, index_type="flat")
    store.add(np.array(x), meta)
    return store, q


@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_store_similar_to(tmp_path, monkeypatch, metric):
    store, q = _store(tmp_path, monkeypatch, metric)
    qa, qb = q[0].tolist(), q[1].tolist()
    ranked_b = store.search(qb, N)
    threshold = ranked_b[80]["distance"]  # strict: the 80 better items match
    near_b = {h["metadata"]["photo_path"] for h in store.search_range(qb, threshold)}
    assert len(near_b) == 80
    sel = store.similar_to(qb, threshold)
    assert sel.count == 80 == store.count_matches(qb, threshold)
    # as `allowed` of a search: the ranking of qa among the items near qb, and among the others
    ranked_a = [h["metadata"]["photo_path"] for h in store.search(qa, N)]
    got = [h["metadata"]["photo_path"] for h in store.search(qa, 20, allowed=sel)]
    assert got == [p for p in ranked_a if p in near_b][:20]
    far = store.similar_to(qb, threshold, negate=True)
    assert far.count == N - 80
    got = [h["metadata"]["photo_path"] for h in store.search(qa, 20, allowed=far)]
    assert got == [p for p in ranked_a if p not in near_b][:20]
    # as `allowed` of the facet counts
    t_a = store.search(qa, 100)[99]["distance"]
    hits = store.search_range(qa, t_a)
    facets = store.facet_counts(qa, t_a, "year", allowed=sel)
    years = [h["metadata"]["year"] for h in hits if h["metadata"]["photo_path"] in near_b]
    assert facets["total"] == len(years) > 0
    assert facets["counts"] == {y: years.count(y) for y in sorted(set(years))}
    # `allowed` restricts both sides
    pred = lambda m: m["year"] != 2020  # noqa: E731
    inside = store.similar_to(qb, threshold, allowed=pred)
    outside = store.similar_to(qb, threshold, allowed=pred, negate=True)
    n_pred = sum(1 for m in store.metadata if pred(m))
    assert inside.count == store.count_matches(qb, threshold, allowed=pred) and inside.count + outside.count == n_pred
    # set operators
    assert (sel & far).count == 0 and (sel | far).count == N and (sel - inside).count == 80 - inside.count
    assert (~sel).count == far.count
    with pytest.raises(ValueError):
        store.similar_to(qb[:-1], threshold)


@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_store_similar_to_items(tmp_path, monkeypatch, metric):
    store, _ = _store(tmp_path, monkeypatch, metric)
    paths = ["/p/3.jpg", "/p/77.jpg"]
    near = [store.search_similar(p, 30) for p in paths]
    thresholds = [hits[-1]["distance"] for hits in near]
    threshold = max(thresholds) if metric == "cosine" else min(thresholds)  # (the tighter of the two)
    want = [{p} | {h["metadata"]["photo_path"] for h in hits
                   if (h["distance"] > threshold if metric == "cosine" else h["distance"] < threshold)}
            for p, hits in zip(paths, near)]
    sel = store.similar_to_items(paths, threshold)
    allowed = {store.metadata[i]["photo_path"] for i in np.flatnonzero(sel.to_mask()).tolist()}
    assert allowed == want[0] | want[1] and set(paths) <= allowed  # the photos themselves are in
    both = store.similar_to_items(paths, threshold, mode="all")
    assert {store.metadata[i]["photo_path"] for i in np.flatnonzero(both.to_mask()).tolist()} == want[0] & want[1]
    rest = store.similar_to_items(paths, threshold, negate=True)
    assert rest.count == N - sel.count and not (set(paths) & {store.metadata[i]["photo_path"]
                                                                for i in np.flatnonzero(rest.to_mask()).tolist()})
    assert store.similar_to_items(paths[0], threshold).count == len(want[0])  # one path as a string
    with pytest.raises(ValueError):
        store.similar_to_items(["/p/3.jpg", "/nowhere.jpg"], threshold)


def test_store_selectors_of_an_empty_store(tmp_path, monkeypatch):
    from photo_search_engine_amd import vector_store as vsmod
    monkeypatch.setattr(vsmod, "_index_factory", oracle_scoresel_factory)
    store = vsmod.VectorStore(dimension=D_, index_path=str(tmp_path / "idx"), metadata_path=str(tmp_path / "meta.json"),
                              metric="cosine", index_type="flat")
    with pytest.raises(RuntimeError):
        store.similar_to([0.0] * D_, 0.5)
    with pytest.raises(RuntimeError):
        store.similar_to_items(["/p/0.jpg"], 0.5)

"""Facet counts without a GPU: the recipe's identities, the wrappers' argument checks, and
``VectorStore.facet_counts`` / ``count_matches`` over the oracle index."""
import numpy as np
import pytest

from oracle import oracle as O
from oracle_diverse_index import burst_corpus
from oracle_facet_index import facet_reference, oracle_facet_factory
from oracle_group_index import burst_keys
from oracle_range_index import range_reference
from photo_search_engine_amd import index as idxmod

N, D_ = 256, 72


@pytest.fixture(scope="module")
def corpus():
    x, q = burst_corpus()
    keys = burst_keys().copy()
    keys[keys % 5 == 0] = -3  # ungrouped rows
    return O.round_dtype(x, "bf16"), q[:5], keys


# ---- the recipe --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_reference_identities(corpus, metric):
    xs, q, keys = corpus
    nq = q.shape[0]
    S, _ = O.knn_exact(xs, q, 40, metric)
    r = S[:, 39].astype(np.float32)
    mask = np.arange(N) % 3 != 0
    totals, counts, gkeys = facet_reference(xs, q, r, metric, keys, mask=mask)
    lims, _, I = range_reference(xs, q, r, metric, mask)
    assert gkeys.tolist() == sorted(set(keys[keys >= 0].tolist()))
    G = gkeys.shape[0]
    assert counts.shape == (nq, G + 1)
    np.testing.assert_array_equal(totals, np.diff(lims))
    np.testing.assert_array_equal(totals, counts.sum(axis=1))
    for i in range(nq):
        got = keys[I[lims[i]:lims[i + 1]]]
        for g, key in enumerate(gkeys.tolist()):
            assert counts[i, g] == int((got == key).sum())
        assert counts[i, G] == int((got < 0).sum())
    # an infinite radius: the group sizes under the mask; the opposite infinity: nothing
    every = np.float32(-np.inf if metric == "ip" else np.inf)
    totals, counts, _ = facet_reference(xs, q, every, metric, keys, mask=mask)
    assert (totals == int(mask.sum())).all()
    for g, key in enumerate(gkeys.tolist()):
        assert (counts[:, g] == int(((keys == key) & mask).sum())).all()
    assert (counts[:, G] == int(((keys < 0) & mask).sum())).all()
    totals, counts, _ = facet_reference(xs, q, -every, metric, keys, mask=mask)
    assert not totals.any() and not counts.any()


def test_reference_members_are_the_covered_rows(corpus):
    xs, q, keys = corpus
    every = np.float32(-np.inf)
    # keys over the first 200 rows: the rest are no members, whatever the mask allows
    totals, counts, _ = facet_reference(xs, q, every, "ip", keys[:200], mask=np.ones(N, dtype=bool))
    assert (totals == 200).all() and (counts.sum(axis=1) == 200).all()
    # a mask shorter than the index (a selector made before rows were added) selects none of the later rows
    totals, _, _ = facet_reference(xs, q, every, "ip", keys, mask=np.ones(100, dtype=bool))
    assert (totals == 100).all()
    # without keys: every row, one number per query
    totals, counts, gkeys = facet_reference(xs, q, every, "ip")
    assert (totals == N).all() and counts is None and gkeys is None


# ---- the wrappers ------------------------------------------------------------------------------------------
def test_wrappers_validate_before_any_library_call():
    """The argument checks of ``range_count`` come before the handle is touched."""
    ix = idxmod.FlatIndex.__new__(idxmod.FlatIndex)
    ix.d, ix._h, ix._L = 8, None, None
    q = np.zeros((2, 8), dtype=np.float32)
    with pytest.raises(ValueError):
        ix.range_count(np.zeros((2, 7), dtype=np.float32), 0.0)
    with pytest.raises(ValueError):
        ix.range_count(q, [0.0, 1.0, 2.0])
    with pytest.raises(ValueError):
        ix.range_count(q, np.nan)
    with pytest.raises(TypeError):
        ix.range_count(q, 0.0, groups=[1, 2, 3])
    with pytest.raises(ValueError):
        ix.set_facet_hist("shared")
    with pytest.raises(ValueError):
        idxmod.set_facet_staging_bytes(0)
    mi = idxmod.MultiDeviceFlatIndex.__new__(idxmod.MultiDeviceFlatIndex)
    mi.d, mi._h, mi._L, mi._prune_copy = 8, None, None, None
    with pytest.raises(ValueError):
        mi.range_count(np.zeros((2, 7), dtype=np.float32), 0.0)
    with pytest.raises(ValueError):
        mi.range_count(q, [0.0])
    with pytest.raises(TypeError):
        mi.range_count(q, 0.0, groups=object())


# ---- the store ---------------------------------------------------------------------------------------------
def _store(tmp_path, monkeypatch, metric):
    from photo_search_engine_amd import vector_store as vsmod
    monkeypatch.setattr(vsmod, "_index_factory", oracle_facet_factory)
    x, q = burst_corpus()
    burst = burst_keys()
    meta = [{"photo_path": f"/p/{i}.jpg", "year": 2019 + i % 6, "day": None if burst[i] % 5 == 0 else f"day-{burst[i]}"}
            for i in range(N)]
    for i in range(0, N, 50):
        del meta[i]["day"]  # a missing field means ungrouped, as None does
    store = vsmod.VectorStore(dimension=D_, index_path=str(tmp_path / "idx"), metadata_path=str(tmp_path / "meta.json"),
                              metric=metric, index_type="flat")
    store.add(np.array(x), meta)
    return store, q, meta


@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_store_facet_counts_and_count_matches(tmp_path, monkeypatch, metric):
    store, q, meta = _store(tmp_path, monkeypatch, metric)
    ranked = store.search(q[0].tolist(), N)
    threshold = ranked[60]["distance"]  # strict: the 60 better items match
    hits = store.search_range(q[0].tolist(), threshold)
    assert len(hits) == 60
    assert store.count_matches(q[0].tolist(), threshold) == 60
    # a field: the items without it land in "ungrouped"
    got = store.facet_counts(q[0].tolist(), threshold, "day")
    days = [h["metadata"].get("day") for h in hits]
    want = {}
    for m in meta:  # (ascending key order = order of first appearance in the store)
        v = m.get("day")
        if v is not None and v not in want and days.count(v):
            want[v] = days.count(v)
    assert got == {"total": 60, "counts": want, "ungrouped": days.count(None)}
    assert list(got["counts"]) == list(want) and got["ungrouped"] > 0
    assert sum(got["counts"].values()) + got["ungrouped"] == got["total"]
    # a predicate for `allowed`
    pred = lambda m: m["year"] != 2020  # noqa: E731
    hits = store.search_range(q[0].tolist(), threshold, allowed=pred)
    assert store.count_matches(q[0].tolist(), threshold, allowed=pred) == len(hits) < 60
    got = store.facet_counts(q[0].tolist(), threshold, "year", allowed=pred)
    years = [h["metadata"]["year"] for h in hits]
    assert got["total"] == len(hits) and got["ungrouped"] == 0 and 2020 not in got["counts"]
    assert got["counts"] == {y: years.count(y) for y in (2019, 2021, 2022, 2023, 2024) if years.count(y)}
    # a callable and integer keys say the same thing
    by_call = store.facet_counts(q[0].tolist(), threshold, lambda m: m["year"], allowed=pred)
    assert by_call == got
    by_ints = store.facet_counts(q[0].tolist(), threshold, [m["year"] - 2000 for m in meta], allowed=pred)
    assert by_ints["counts"] == {y - 2000: n for y, n in sorted(got["counts"].items())}
    # the cached groups of a field serve search_grouped and facet_counts alike
    page = store.search_grouped(q[0].tolist(), 3, "year", group_size=2)
    assert len(page) == 3
    assert store.facet_counts(q[0].tolist(), threshold, "year", allowed=pred) == got
    # nothing matches
    nothing = float("inf") if metric == "cosine" else float("-inf")
    assert store.facet_counts(q[0].tolist(), nothing, "day") == {"total": 0, "counts": {}, "ungrouped": 0}
    assert store.count_matches(q[0].tolist(), nothing) == 0


def test_store_facets_of_an_empty_store(tmp_path, monkeypatch):
    from photo_search_engine_amd import vector_store as vsmod
    monkeypatch.setattr(vsmod, "_index_factory", oracle_facet_factory)
    store = vsmod.VectorStore(dimension=D_, index_path=str(tmp_path / "idx"), metadata_path=str(tmp_path / "meta.json"),
                              metric="cosine", index_type="flat")
    assert store.count_matches([0.0] * D_, 0.5) == 0
    assert store.facet_counts([0.0] * D_, 0.5, "day") == {"total": 0, "counts": {}, "ungrouped": 0}

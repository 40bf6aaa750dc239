"""Grouped search without a GPU: the reference recipe's own identities (tests/oracle_group_index.py) and
``VectorStore.search_grouped`` on the oracle-backed index -- each ``group_by`` form, the cache of a
field's group keys and what drops it, and the ``ValueError``s."""
import numpy as np
import pytest

from oracle import oracle as O
from oracle_diverse_index import burst_corpus
from oracle_group_index import (KEY_PAD, OracleGroups, burst_keys, expected_rounds, group_reference,
                                oracle_group_factory)
from oracle_sel_index import filtered_reference

N, D_ = 256, 72
BASE = 2 ** 40


@pytest.fixture(scope="module")
def corpus():
    x, q = burst_corpus()
    return O.round_dtype(x, "bf16"), q, burst_keys()


@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_reference_identities(corpus, metric):
    xs, q, burst = corpus
    mask = np.arange(N) % 3 != 0
    for sel in (None, mask):
        m = np.ones((N,), dtype=bool) if sel is None else sel
        # all keys negative, or all distinct, and g = 1: the plain (filtered) search
        D, I = filtered_reference(xs, q, m, 300, metric)
        for keys in (np.full((N,), -3, dtype=np.int64), np.arange(N, dtype=np.int64)[::-1] + BASE):
            Ko, Dg, Ig, found, sizes, need = group_reference(xs, q, keys, 300, 1, metric, sel)
            np.testing.assert_array_equal(Ig[:, :, 0], I)
            np.testing.assert_array_equal(Dg[:, :, 0].view(np.uint32), D.view(np.uint32))
            np.testing.assert_array_equal(Ko, np.where(I >= 0, keys[np.maximum(I, 0)], KEY_PAD))
            np.testing.assert_array_equal(found, I >= 0)
            np.testing.assert_array_equal(sizes, I >= 0)
            assert (need == int(m.sum())).all()  # k > members: complete with the last member
        # all keys equal: the one group holds the first g entries of the plain search
        D, I = filtered_reference(xs, q, m, 7, metric)
        Ko, Dg, Ig, found, sizes, need = group_reference(xs, q, np.full((N,), 5, dtype=np.int64), 3, 7, metric, sel)
        np.testing.assert_array_equal(Ig[:, 0, :], I)
        np.testing.assert_array_equal(Dg[:, 0, :].view(np.uint32), D.view(np.uint32))
        assert (Ko[:, 0] == 5).all() and (Ko[:, 1:] == KEY_PAD).all() and (Ig[:, 1:] == -1).all()
        assert (found[:, 0] == 7).all() and (sizes[:, 0] == int(m.sum())).all() and (need == 7).all()
    # groups follow their best member, members follow the ranking, sizes count the members
    keys = burst + BASE
    Ko, Dg, Ig, found, sizes, need = group_reference(xs, q, keys, 10, 3, metric)
    D, I = filtered_reference(xs, q, np.ones((N,), dtype=bool), N, metric)
    for qi in range(q.shape[0]):
        first_seen = list(dict.fromkeys(keys[I[qi]].tolist()))[:10]
        assert Ko[qi].tolist() == first_seen
        for s, key in enumerate(first_seen):
            rows = I[qi][keys[I[qi]] == key]
            assert Ig[qi, s, : found[qi, s]].tolist() == rows[:3].tolist() and sizes[qi, s] == rows.shape[0]
            assert found[qi, s] == min(3, rows.shape[0])
        last = max(int(np.flatnonzero(I[qi] == Ig[qi, s, found[qi, s] - 1])[0]) for s in range(10))
        assert need[qi] == last + 1
    # rows behind the keys, and an empty member set
    Ko, Dg, Ig, found, sizes, need = group_reference(xs, q, keys[:100], 5, 2, metric)
    assert Ig.max() < 100 and (found > 0).all()
    Ko, Dg, Ig, found, sizes, need = group_reference(xs, q, keys, 5, 2, metric, np.zeros((N,), dtype=bool))
    assert (Ig == -1).all() and (Ko == KEY_PAD).all() and (found == 0).all() and (sizes == 0).all() and (need == 0).all()


def test_replayed_rounds_agree_with_need(corpus):
    xs, q, burst = corpus
    keys = np.where(burst % 5 == 0, -1 - burst, burst + BASE)
    for k, g, first, limit in ((10, 3, 16, 64), (10, 3, 30, 30), (4, 8, 32, 32), (10, 1, 10, 10)):
        need = group_reference(xs, q, keys, k, g, "ip")[5]
        sim = expected_rounds(xs, q, keys, k, g, "ip", first, limit)
        for qi, (tier, rounds) in enumerate(sim):
            want = 0 if need[qi] <= min(first, limit) else 1 if need[qi] <= limit else 2
            assert tier == want and (rounds >= 1) == (tier == 2)


def _store(tmp_path, monkeypatch, metric="cosine", index_type="flat"):
    from photo_search_engine_amd import vector_store as vsmod
    monkeypatch.setattr(vsmod, "_index_factory", oracle_group_factory)
    x, q = burst_corpus()
    burst = burst_keys()
    meta = [{"photo_path": f"/p/{i}.jpg", "year": 2019 + i % 6, "day": None if burst[i] % 5 == 0 else f"day-{burst[i]}"}
            for i in range(N)]
    for i in range(0, N, 50):
        del meta[i]["day"]  # a missing field means ungrouped, as None does
    store = vsmod.VectorStore(dimension=D_, index_path=str(tmp_path / "idx"), metadata_path=str(tmp_path / "meta.json"),
                              metric=metric, index_type=index_type)
    store.add(np.array(x), meta)
    return store, x, q, burst, meta


@pytest.mark.parametrize("index_type,metric", [("flat", "cosine"), ("hnsw", "l2")])
def test_store_search_grouped_every_group_by_form(tmp_path, monkeypatch, index_type, metric):
    store, x, q, burst, meta = _store(tmp_path, monkeypatch, metric, index_type)
    kind = "ip" if metric == "cosine" else "l2"
    xs = store.index._x
    query = store._normalize_query(q[0].tolist())
    plain = store.search(q[0].tolist(), N)
    day = [m.get("day") for m in meta]
    # a field name
    page = store.search_grouped(q[0].tolist(), 10, "day", group_size=3)
    assert len(page) == 10 and all(1 <= len(p["items"]) <= 3 and p["size"] >= len(p["items"]) for p in page)
    seen, order = set(), []
    for hit in plain:  # the groups in order of their best item
        value = hit["metadata"].get("day")
        token = value if value is not None else ("alone", hit["metadata"]["photo_path"])
        if token not in seen:
            seen.add(token)
            order.append((value, hit))
    for p, (value, best) in zip(page, order):
        assert p["group"] == value and p["items"][0] == best
        if value is None:
            assert p["size"] == 1 and len(p["items"]) == 1
        else:
            assert p["size"] == day.count(value)
            assert p["items"] == [h for h in plain if h["metadata"].get("day") == value][:3]
    # a callable and a sequence of ints give the same page when they say the same thing
    codes = {}
    ints = [codes.setdefault(v, len(codes)) if v is not None else -1 for v in day]
    by_call = store.search_grouped(q[0].tolist(), 10, lambda m: m.get("day"), group_size=3)
    by_ints = store.search_grouped(q[0].tolist(), 10, ints, group_size=3)
    assert by_call == page
    assert [(p["size"], p["items"]) for p in by_ints] == [(p["size"], p["items"]) for p in page]
    assert [p["group"] for p in by_ints] == [None if p["group"] is None else codes[p["group"]] for p in page]
    # against the reference, with a filter
    pred = lambda m: m["year"] != 2020  # noqa: E731
    mask = np.array([pred(m) for m in meta])
    keys = np.asarray(ints, dtype=np.int64)
    Ko, Dg, Ig, found, sizes, _ = group_reference(xs, query, keys, 10, 3, kind, mask)
    got = store.search_grouped(q[0].tolist(), 10, "day", group_size=3, allowed=pred)
    assert [p["size"] for p in got] == sizes[0].tolist()
    assert [[meta.index(h["metadata"]) for h in p["items"]] for p in got] == [Ig[0, s, : found[0, s]].tolist()
                                                                             for s in range(10)]
    assert [[h["distance"] for h in p["items"]] for p in got] == [[float(v) for v in Dg[0, s, : found[0, s]]]
                                                                  for s in range(10)]
    # the clamp and the short page
    assert len(store.search_grouped(q[0].tolist(), 1000, "year")) == 6
    everything = store.search_grouped(q[0].tolist(), 1000, "day", group_size=12)
    assert sum(len(p["items"]) for p in everything) == N


def test_store_cache_and_what_drops_it(tmp_path, monkeypatch):
    store, x, q, burst, meta = _store(tmp_path, monkeypatch)
    made = []
    real = store.index.group_keys
    monkeypatch.setattr(store.index, "group_keys", lambda keys: made.append(1) or real(keys))
    page = store.search_grouped(q[0].tolist(), 5, "day", group_size=2)
    assert store.search_grouped(q[1].tolist(), 5, "day") and len(made) == 1  # the field's keys are cached
    store.search_grouped(q[0].tolist(), 5, lambda m: m.get("day"))
    store.search_grouped(q[0].tolist(), 5, lambda m: m.get("day"))
    assert len(made) == 3  # callables are not
    store.search_grouped(q[0].tolist(), 5, "year")
    store.search_grouped(q[0].tolist(), 5, "day")
    assert len(made) == 5  # one field at a time
    assert isinstance(store._group_cache["day"][2], OracleGroups)

    def dropped(action):
        store.search_grouped(q[0].tolist(), 5, "day")
        assert "day" in store._group_cache
        action()
        assert store._group_cache == {}

    dropped(lambda: store.add_item(x[0].tolist(), {"photo_path": "/p/new.jpg", "day": "day-new"}))
    assert store.search_grouped(x[0].tolist(), 1, "day", group_size=5)[0]["size"] >= 1
    dropped(lambda: store.add(np.array(x[:2]), [{"photo_path": "/p/a.jpg"}, {"photo_path": "/p/b.jpg"}]))
    dropped(lambda: store.remove_ids([1]))
    dropped(lambda: store.remove_items(["/p/2.jpg"]))
    dropped(lambda: store.update_item(x[3].tolist(), {"photo_path": "/p/3.jpg", "day": "day-moved"}))
    moved = store.search_grouped(x[3].tolist(), 1, "day")
    assert moved[0]["group"] == "day-moved" and moved[0]["size"] == 1
    store.save()
    dropped(lambda: store.load())
    assert store.search_grouped(q[0].tolist(), 5, "day", group_size=2)
    dropped(store.clear)
    assert store.search_grouped(q[0].tolist(), 5, "day") == []
    assert page


def test_store_value_errors(tmp_path, monkeypatch):
    store, x, q, burst, meta = _store(tmp_path, monkeypatch)
    with pytest.raises(ValueError):
        store.search_grouped(q[0, :10].tolist(), 3, "day")  # the dimension guard of search()
    with pytest.raises(ValueError):
        store.search_grouped(q[0].tolist(), 200, "day", group_size=17)  # 3400 > 3276
    assert store.search_grouped(q[0].tolist(), 4000, "day", group_size=12)  # top_k is clamped to ntotal first
    for bad in (dict(top_k=0), dict(group_size=0), dict(top_k=-2)):
        with pytest.raises(ValueError):
            store.search_grouped(q[0].tolist(), bad.get("top_k", 3), "day", group_size=bad.get("group_size", 1))
    for bad in (list(range(N - 1)), np.zeros((N, 2), dtype=np.int64), [0.5] * N):
        with pytest.raises(ValueError):
            store.search_grouped(q[0].tolist(), 3, bad)


def test_python_argument_helpers():
    from photo_search_engine_amd.index import GROUP_KG_MAX, group_args, group_key_array
    assert group_args(1092, 3) == (1092, 3) and GROUP_KG_MAX == 3276
    for bad in ((0, 1), (1, 0), (1093, 3), (3277, 1)):
        with pytest.raises(ValueError):
            group_args(*bad)
    assert group_key_array([3, -1, 2 ** 40], 3).dtype == np.int64
    assert group_key_array([], 0).shape == (0,)
    for bad, n in (([1, 2], 3), ([[1, 2]], 2), ([1.0, 2.0], 2), (np.array([2 ** 63], dtype=np.uint64), 1)):
        with pytest.raises(ValueError):
            group_key_array(bad, n)

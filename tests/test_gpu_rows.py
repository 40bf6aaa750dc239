"""Queries taken from stored rows on the GPU (MI355X only): ``vs_search_rows`` / ``vs_range_search_rows``.

Reference for every case (tests/oracle_rows_index.py): query ``i`` is the stored value of row ``ids[i]``
(``O.round_dtype``); top-k is the oracle's exact search at ``k + 1`` with the row itself dropped by id,
range is ``range_reference`` with the self / above mask per query.  ``lims``, ids and distances must be
bit-equal under every tier, screen and scan-limit setting."""
import numpy as np
import pytest

from oracle import oracle as O
from oracle_range_index import range_reference
from oracle_rows_index import oracle_rows_factory, rows_range_reference, rows_topk_reference
from test_gpu_range import _modes

pytestmark = pytest.mark.gpu

N, D_ = 3000, 64


@pytest.fixture(scope="module")
def idx():
    from photo_search_engine_amd import index
    return index


def _unit_rows(seed, n=N, d=D_):
    x = np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _eq(got, want, what=""):
    for g, w, name in zip(got, want, ("first", "second", "third")):
        np.testing.assert_array_equal(g, w, err_msg=f"{what}: {name} array")


# ---- top-k ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_topk_rows(idx, dtype, metric):
    """n of {1, 2, 9, 300} (one query, the scan-limit path, one MFMA block, more than one block), k of
    {1, 10, N - 1}, the scan limit off and at its default, both screens."""
    x = _unit_rows(3)
    xs = O.round_dtype(x, dtype)
    rng = np.random.default_rng(4)
    ix = idx.FlatIndex(D_, metric, dtype)
    ix.add(x)
    for n in (1, 2, 9, 300):
        ids = rng.integers(0, N, size=n)
        ids[0] = N - 1
        if n >= 9:
            ids[1], ids[2], ids[3] = 0, 256, ids[4]  # (the ends, a tile border, a repeat)
        for k in (1, 10, N - 1):
            ref = rows_topk_reference(xs, ids, k, metric)
            assert (ref[1] != ids[:, None]).all()
            keep = rows_topk_reference(xs, ids, k, metric, drop_self=False) if k == 10 else None
            for screen in ("native", "int8"):
                ix.set_screen(screen)
                for limit in (0, 192 << 20):
                    ix.set_scan_limit(limit)
                    what = f"n={n} k={k} {screen} limit={limit}"
                    D, I = ix.search_rows(ids, k)
                    _eq((I, D), (ref[1], ref[0]), what)
                    if k == 10:
                        Dk, Ik = ix.search_rows(ids, k, drop_self=False)
                        _eq((Ik, Dk), (keep[1], keep[0]), what + " keep")
                        Ds, Is = ix.search(xs[ids], k)  # KEEP is vs_search on those vectors
                        _eq((Ik, Dk), (Is, Ds), what + " keep vs search")
    ix.close()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_ties_drop_the_row_itself_not_the_first_slot(idx, dtype):
    x = _unit_rows(5)
    x[900] = x[5]
    x[2500] = x[5]
    xs = O.round_dtype(x, dtype)
    ix = idx.FlatIndex(D_, "ip", dtype)
    ix.add(x)
    others = np.array([17, 2999, 0, 1200, 301, 77, 2048, 511, 1023], dtype=np.int64)
    for ids in (np.array([900, 2500]), np.concatenate([[900, 2500], others])):
        for limit in (0, 192 << 20):
            ix.set_scan_limit(limit)
            D, I = ix.search_rows(ids, 4)
            _eq((I, D), rows_topk_reference(xs, ids, 4, "ip")[::-1], f"drop n={len(ids)}")
            assert I[0, :2].tolist() == [5, 2500] and I[1, :2].tolist() == [5, 900]  # the lower-id twins first
            assert D[0, 0] == D[0, 1] and D[1, 0] == D[1, 1]
            Dk, Ik = ix.search_rows(ids, 4, drop_self=False)
            assert Ik[0, :3].tolist() == [5, 900, 2500] and Ik[1, :3].tolist() == [5, 900, 2500]  # KEEP returns it
            _eq((Ik, Dk), rows_topk_reference(xs, ids, 4, "ip", drop_self=False)[::-1], "keep")
    ix.close()


def test_self_not_among_the_top(idx):
    """Inner product over unnormalised rows: a short row's own score is far from its best, so it is not
    among its k + 1 and DROP returns the first k unchanged."""
    rng = np.random.default_rng(6)
    x = rng.standard_normal((N, D_)).astype(np.float32)
    short = np.array([3, 256, 1500, 2999, 10, 11, 12, 13, 14, 15], dtype=np.int64)
    x[short] *= np.float32(1e-3)
    ix = idx.FlatIndex(D_, "ip", "f32")
    ix.add(x)
    for ids in (short[:2], short):
        S, Ie = O.knn_exact(x, x[ids], 11, "ip")
        assert (Ie != ids[:, None]).all()
        D, I = ix.search_rows(ids, 10)
        _eq((I, D), (Ie[:, :10], S[:, :10].astype(np.float32)), "first k unchanged")
        _eq((I, D), rows_topk_reference(x, ids, 10, "ip")[::-1], "recipe")
    ix.close()


@pytest.mark.parametrize("metric,dtype", [("ip", "bf16"), ("l2", "f32")])
def test_topk_rows_with_a_selector(idx, metric, dtype):
    x = _unit_rows(7)
    xs = O.round_dtype(x, dtype)
    rng = np.random.default_rng(8)
    mask = rng.random(N) < 0.05
    allowed, barred = np.flatnonzero(mask), np.flatnonzero(~mask)
    ids = np.concatenate([allowed[:6], barred[:6], allowed[:1]])  # the query row allowed, and not
    ix = idx.FlatIndex(D_, metric, dtype)
    ix.add(x)
    sel = ix.selector(mask)
    for k in (1, 10, int(mask.sum()) + 3):
        ref = rows_topk_reference(xs, ids, k, metric, mask)
        keep = rows_topk_reference(xs, ids, k, metric, mask, drop_self=False)
        for mode in ("scan", "overfetch", "auto"):
            ix.set_sel_mode(mode)
            for pick in (ids, ids[:2]):
                D, I = ix.search_rows(pick, k, sel=sel)
                _eq((I, D), (ref[1][:len(pick)], ref[0][:len(pick)]), f"k={k} {mode} n={len(pick)}")
                assert ix.sel_last_stats()["m"] == int(mask.sum())
                if mode != "auto":
                    assert ix.sel_last_stats()["tier"] == mode
            Dk, Ik = ix.search_rows(ids, k, sel=mask, drop_self=False)
            _eq((Ik, Dk), (keep[1], keep[0]), f"keep k={k} {mode}")
            Ds, Is = ix.search(xs[ids], k, sel=sel)
            _eq((Ik, Dk), (Is, Ds), "keep vs search_sel")
    ix.set_sel_mode("auto")
    sel.close()
    ix.close()


# ---- range ------------------------------------------------------------------------------------------------
def _planted(seed, dtype):
    """Unit rows with 60 planted groups of 2-5 near-identical rows (a base row plus 1e-3 noise) at ids
    that include 0, 255, 256, 257 and N - 1."""
    rng = np.random.default_rng(seed)
    x = _unit_rows(seed + 100)
    free = np.setdiff1d(np.arange(N), [0, 255, 256, 257, N - 1])
    spots = list(rng.permutation(free))
    forced = [0, 255, 256, 257, N - 1]
    groups = []
    for g in range(60):
        size = 2 + g % 4
        members = [forced.pop()] if forced else []
        while len(members) < size:
            members.append(int(spots.pop()))
        base = x[members[0]].copy()
        for m in members[1:]:
            v = base + np.float32(1e-3) * rng.standard_normal(D_).astype(np.float32)
            x[m] = v / np.linalg.norm(v)
        groups.append(sorted(members))
    return x, O.round_dtype(x, dtype), groups


def _pairs(lims, I, ids=None):
    first = np.repeat(np.arange(len(lims) - 1) if ids is None else ids, np.diff(lims))
    return list(zip(first.tolist(), I.tolist()))


@pytest.mark.parametrize("metric,dtype", [("ip", "f32"), ("l2", "f32"), ("ip", "bf16"), ("l2", "bf16"), ("ip", "f16")])
def test_range_rows_self_join(idx, metric, dtype):
    from photo_search_engine_amd import _lib
    x, xs, groups = _planted(11, dtype)
    radius = np.float32(0.95 if metric == "ip" else 2.0 - 2.0 * 0.95)
    ix = idx.FlatIndex(D_, metric, dtype)
    ix.add(x)
    every = rows_range_reference(xs, None, radius, metric, self_mode="keep")  # (computed once, filtered below)
    above = rows_range_reference(xs, None, radius, metric, self_mode="above", keep=every)
    drop = rows_range_reference(xs, None, radius, metric, self_mode="drop", keep=every)
    want_pairs = {(a, b) for g in groups for a in g for b in g if a < b}
    assert set(_pairs(above[0], above[2])) == want_pairs and int(drop[0][-1]) == 2 * int(above[0][-1])
    # explicit ids, descending with repeats; and a selector over half of the rows
    ids = np.concatenate([np.arange(N - 1, -1, -7), [N - 1, 256, 256, 0]]).astype(np.int64)
    mask = np.arange(N) % 2 == 0
    mask[[0, 255, 256, 257, N - 1]] = True
    keeps = {"ids": rows_range_reference(xs, ids, radius, metric, None, "keep"),
             "sel": rows_range_reference(xs, None, radius, metric, mask, "keep")}
    refs = {(mode, which): rows_range_reference(xs, i, radius, metric, m, mode, keep=keeps[which])
            for mode in ("above", "drop", "keep")
            for which, i, m in (("ids", ids, None), ("sel", None, mask))}
    try:
        for tier in _modes(dtype, 256, None):
            ix.set_range_mode(tier)
            got_a = ix.range_search_rows(radius)  # ids=None, self_mode="above": the duplicate finder's call
            _eq(got_a, above, f"above {tier}")
            assert ix.range_last_stats()["total"] == int(above[0][-1])
            if tier != "auto":
                assert ix.range_last_stats()["tier"] == tier
            got_d = ix.range_search_rows(radius, self_mode="drop")
            _eq(got_d, drop, f"drop {tier}")
            assert int(got_d[0][-1]) == 2 * int(got_a[0][-1])
            assert set(_pairs(got_a[0], got_a[2])) == {(i, j) for i, j in _pairs(got_d[0], got_d[2]) if i < j}
            for mode in ("above", "drop", "keep"):
                _eq(ix.range_search_rows(radius, ids=ids, self_mode=mode), refs[mode, "ids"], f"ids {mode} {tier}")
            _eq(ix.range_search_rows(radius, ids=ids, self_mode="keep"), ix.range_search(xs[ids], radius), "keep")
        for tier in _modes(dtype, 256, mask):
            ix.set_range_mode(tier)
            for mode in ("above", "drop", "keep"):
                _eq(ix.range_search_rows(radius, sel=mask, self_mode=mode), refs[mode, "sel"], f"sel {mode} {tier}")
        # max_total below the filtered total raises and names the filtered count (not the unfiltered one)
        ix.set_range_mode("auto")
        total = int(above[0][-1])
        _eq(ix.range_search_rows(radius, max_total=total), above, "max_total = total")
        for cap in (total - 1, 1):
            with pytest.raises(_lib.VsError) as e:
                ix.range_search_rows(radius, max_total=cap)
            assert e.value.code == _lib.VS_ERR_ARG and f"found {total} results" in str(e.value)
        _eq(ix.range_search_rows(radius), above, "after the error")
    finally:
        ix.set_range_mode("auto")
    ix.close()


@pytest.mark.parametrize("mode", ["above", "drop"])
def test_range_rows_many_identical_rows(idx, mode):
    """N = 3000 with 600 identical rows, radius just below their score: long segments under the filter.
    (At this N a query's first-pass region holds every row -- 32 MiB / (12 B x 256 queries) = 10922
    slots -- so no segment outgrows it here; test_range_rows_overflow_reruns is the size where they do.)"""
    x = _unit_rows(13)
    rng = np.random.default_rng(14)
    same = np.sort(rng.choice(N, size=600, replace=False))
    x[same] = x[same[0]]
    score = np.float32(O.canon_scores(x[same[:1]], x[same[:1]], "ip")[0, 0])
    radius = np.nextafter(score, np.float32(-np.inf))
    ix = idx.FlatIndex(D_, "ip", "f32")
    ix.add(x)
    ids = np.concatenate([same[:150], same[-150:], np.setdiff1d(np.arange(N), same)[:12]])
    ref = rows_range_reference(x, ids, radius, "ip", self_mode=mode)
    counts = np.diff(ref[0])
    want = 600 - 1 - np.arange(150) if mode == "above" else np.full(150, 599)
    assert counts[:150].tolist() == want.tolist() and (counts[300:] == 0).all()
    _eq(ix.range_search_rows(radius, ids=ids, self_mode=mode), ref, mode)
    ix.close()


def test_range_rows_overflow_reruns(idx):
    """The size at which a segment outgrows its first-pass region (10922 slots per query in a block of
    256) and its query is rerun into a region of the counted size: 11600 identical rows of 12000.  The
    rerun must count what the first pass counted -- the filtered answer -- or the call fails with "a
    rerun counted differently"."""
    n = 12000
    x = _unit_rows(15, n=n)
    rng = np.random.default_rng(16)
    same = np.sort(rng.choice(n, size=11600, replace=False))
    x[same] = x[same[0]]
    score = np.float32(O.canon_scores(x[same[:1]], x[same[:1]], "ip")[0, 0])
    radius = np.nextafter(score, np.float32(-np.inf))
    ix = idx.FlatIndex(D_, "ip", "f32")
    ix.add(x)
    ids = np.concatenate([same[:128], same[-100:], np.setdiff1d(np.arange(n), same)[:28]])  # one block of 256
    for mode, over in (("drop", 228), ("above", 128)):
        ref = rows_range_reference(x, ids, radius, "ip", self_mode=mode)
        assert int((np.diff(ref[0]) > 10922).sum()) == over  # segments past the region, and some within it
        _eq(ix.range_search_rows(radius, ids=ids, self_mode=mode), ref, mode)
        assert ix.range_last_stats()["total"] == int(ref[0][-1])
    ix.close()


# ---- errors -----------------------------------------------------------------------------------------------
def test_argument_errors(idx):
    from photo_search_engine_amd import _lib
    import ctypes
    x = _unit_rows(17, n=500)
    ix = idx.FlatIndex(D_, "ip", "f32")
    ix.add(x)

    def arg_error(call):
        with pytest.raises(_lib.VsError) as e:
            call()
        assert e.value.code == _lib.VS_ERR_ARG

    for bad in ([500], [-1], [3, 500, 4]):
        arg_error(lambda: ix.search_rows(bad, 3))
        arg_error(lambda: ix.range_search_rows(0.5, ids=bad))
    arg_error(lambda: ix.search_rows([3], 0))
    # ABOVE on the top-k call; ids = NULL with n != ntotal (through the C ABI: the wrapper cannot say either)
    ids = np.array([3, 4], dtype=np.int64)
    D = np.empty((2, 3), dtype=np.float32)
    I = np.empty((2, 3), dtype=np.int64)
    rc = ix._L.vs_search_rows(ix._h, None, ids.ctypes.data, 2, 3, idx.SELF_MODES["above"], D.ctypes.data, I.ctypes.data)
    assert rc == _lib.VS_ERR_ARG
    r = np.full((499,), 0.5, dtype=np.float32)
    h = ctypes.c_void_p()
    rc = ix._L.vs_range_search_rows(ix._h, None, None, 499, r.ctypes.data, idx.SELF_MODES["above"], 0, ctypes.byref(h))
    assert rc == _lib.VS_ERR_ARG and not h.value
    rc = ix._L.vs_range_search_rows(ix._h, None, ids.ctypes.data, 2, r.ctypes.data, 3, 0, ctypes.byref(h))
    assert rc == _lib.VS_ERR_ARG and not h.value
    arg_error(lambda: _nan_radius(ix))  # (through the C ABI: the wrapper rejects NaN itself)
    # n = 0 and the empty index behave as in the calls these extend
    D0, I0 = ix.search_rows([], 3)
    assert D0.shape == (0, 3) and I0.shape == (0, 3)
    lims, _, _ = ix.range_search_rows(0.5, ids=[])
    assert lims.tolist() == [0]
    # a stale selector after remove_ids
    sel = ix.selector(np.arange(500) % 2 == 0)
    assert ix.search_rows([3, 4], 3, sel=sel)[1].shape == (2, 3)
    assert ix.remove_ids([7]) == 1
    arg_error(lambda: ix.search_rows([3, 4], 3, sel=sel))
    arg_error(lambda: ix.range_search_rows(0.5, ids=[3, 4], sel=sel))
    arg_error(lambda: ix.search_rows([499], 3))  # (ntotal is 499 now)
    sel.close()
    ix.reset()
    lims, D, I = ix.range_search_rows(0.5)  # empty index, ids=None: n = ntotal = 0
    assert lims.tolist() == [0] and D.shape == (0,) and I.shape == (0,)
    arg_error(lambda: ix.search_rows([0], 3))
    ix.close()


def _nan_radius(ix):
    import ctypes
    from photo_search_engine_amd import _lib
    ids = np.array([3, 4], dtype=np.int64)
    r = np.array([0.5, np.nan], dtype=np.float32)
    h = ctypes.c_void_p()
    _lib.check(ix._L.vs_range_search_rows(ix._h, None, ids.ctypes.data, 2, r.ctypes.data, 1, 0, ctypes.byref(h)))


# ---- multi-device and the store -----------------------------------------------------------------------------
def test_multi_device_rows_equal_one_device(idx):
    x, xs, _ = _planted(19, "f32")
    mi = idx.MultiDeviceFlatIndex(D_, "ip", "f32", devices=(0, 0))
    mi.add(x)
    ids = np.array([0, 255, 2999, 256, 256, 1000], dtype=np.int64)
    _eq(mi.search_rows(ids, 5)[::-1], rows_topk_reference(xs, ids, 5, "ip")[::-1], "multi top-k")
    for mode in ("above", "drop", "keep"):
        _eq(mi.range_search_rows(0.95, ids=ids, self_mode=mode), rows_range_reference(xs, ids, 0.95, "ip", None, mode),
            f"multi range {mode}")
    _eq(mi.range_search_rows(0.95), rows_range_reference(xs, None, 0.95, "ip"), "multi self-join")
    mi.close()


@pytest.mark.parametrize("index_type,metric", [("flat", "cosine"), ("hnsw", "l2")])
def test_store_similar_and_duplicates_equal_the_oracle_store(tmp_path, monkeypatch, index_type, metric):
    from photo_search_engine_amd import vector_store as vsmod
    n, d = 500, 64
    x = _unit_rows(23, n=n, d=d)
    rng = np.random.default_rng(24)
    for a, b in ((10, 400), (400, 77), (3, 499), (250, 251)):
        v = x[a] + np.float32(2e-3) * rng.standard_normal(d).astype(np.float32)
        x[b] = v / np.linalg.norm(v)
    meta = [{"photo_path": f"/p/{i}.jpg", "year": 2019 + i % 6} for i in range(n)]

    def make(sub):
        store = vsmod.VectorStore(dimension=d, index_path=str(tmp_path / sub / "idx"),
                                  metadata_path=str(tmp_path / sub / "meta.json"), metric=metric, index_type=index_type)
        store.add(x, meta)
        return store

    gpu = make("gpu")
    monkeypatch.setattr(vsmod, "_index_factory", oracle_rows_factory)
    ref = make("ref")
    ref.index._x = gpu.index.reconstruct_n(0, n)  # (the values as stored)
    thr = 0.99 if metric == "cosine" else 0.02
    pred = lambda m: m["year"] != 2020  # noqa: E731
    for path, k in (("/p/400.jpg", 5), ("/p/0.jpg", 1), ("/p/499.jpg", 600)):
        assert gpu.search_similar(path, k) == ref.search_similar(path, k)
        assert gpu.search_similar(path, k, allowed=pred) == ref.search_similar(path, k, allowed=pred)
    assert len(gpu.search_similar("/p/499.jpg", 600)) == n - 1
    groups = gpu.find_duplicates(thr)
    assert groups == ref.find_duplicates(thr) and [10, 77, 400] in groups and [3, 499] in groups
    assert gpu.find_duplicates(thr, allowed=pred) == ref.find_duplicates(thr, allowed=pred)
    for g, r in zip(gpu.duplicate_pairs(thr), ref.duplicate_pairs(thr)):
        np.testing.assert_array_equal(g, r)
    with pytest.raises(ValueError):
        gpu.search_similar("/p/none.jpg", 3)

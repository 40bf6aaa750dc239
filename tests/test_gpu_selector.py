"""Exact filtered search on the GPU (MI355X only): id selectors on the flat index.

Reference for every case (tests/oracle_sel_index.py ``filtered_reference``): the oracle's canonical
fp64 scores of the allowed rows alone (stored values, ``O.round_dtype``), their top-k under (score,
then id), mapped back to row ids, padded with ``-1`` / ``-+FLT_MAX``.  Ids and distances must be
bit-equal, under the scan tier, the overfetch tier and the library's own choice alike.
"""
import threading

import numpy as np
import pytest

from oracle import oracle as O
from oracle_sel_index import filtered_reference

pytestmark = pytest.mark.gpu

MODES = ("scan", "overfetch", "auto")
K_MAX = 3276  # KP_MAX * 4 / 5


@pytest.fixture(scope="module")
def idx():
    from photo_search_engine_amd import index
    return index


def _check(ix, xs, q, mask, k, metric, sel=None, modes=MODES):
    """Search under every mode, compare each with the reference; returns the stats per mode."""
    Dref, Iref = filtered_reference(xs, q, mask, k, metric)
    s = sel if sel is not None else ix.selector(mask)
    stats = {}
    try:
        for mode in modes:
            ix.set_sel_mode(mode)
            D, I = ix.search(q, k, sel=s)
            np.testing.assert_array_equal(I, Iref, err_msg=f"ids, mode {mode}")
            np.testing.assert_array_equal(D, Dref, err_msg=f"distances, mode {mode}")
            stats[mode] = ix.sel_last_stats()
    finally:
        ix.set_sel_mode("auto")
        if sel is None:
            s.close()
    if "scan" in stats:
        assert stats["scan"]["tier"] == "scan"
    return stats


# ---- compaction -----------------------------------------------------------------------------------
def _masks(n, rng):
    first = np.zeros(n, dtype=bool)
    first[0] = True
    last = np.zeros(n, dtype=bool)
    last[n - 1] = True
    return {"all": np.ones(n, dtype=bool), "none": np.zeros(n, dtype=bool), "first": first, "last": last,
            "alternating": np.arange(n) % 2 == 0, "random_0.1%": rng.random(n) < 0.001, "random_50%": rng.random(n) < 0.5}


@pytest.mark.parametrize("n", [1, 7, 8, 63, 64, 65, 511, 513, 70001])
def test_compaction(idx, n):
    """Rows x_i = (i, 0, ...) under L2: the query (c, 0, ...) ranks the allowed ids by |i - c| (ties to
    the lower id), so k = m returns the whole id list, and for 70,001 rows (two compaction workgroups
    of 65,536 ids) windows of K_MAX ids around 24 centres cover it end to end."""
    rng = np.random.default_rng(n)
    x = np.zeros((n, 32), dtype=np.float32)
    x[:, 0] = np.arange(n)
    ix = idx.FlatIndex(32, "l2", "f32")
    ix.add(x)
    centres = np.linspace(0, n - 1, 24 if n > K_MAX else 2)
    q = np.zeros((centres.shape[0], 32), dtype=np.float32)
    q[:, 0] = np.round(centres)
    for name, mask in _masks(n, rng).items():
        ids = np.flatnonzero(mask)
        m = int(ids.shape[0])
        sel = ix.selector(mask)
        assert sel.count == m, name
        k = max(1, min(m, K_MAX))
        _check(ix, x, q, mask, k, "l2", sel=sel)
        if 0 < m <= K_MAX:
            ix.set_sel_mode("scan")
            _, I = ix.search(q, m, sel=sel)
            assert all(set(row.tolist()) == set(ids.tolist()) for row in I), name
        sel.close()
        # an over-long bitmap with stray bits past n: ignored on the host and on the device alike
        stray = np.full(((n + 7) // 8 + 11,), 0xFF, dtype=np.uint8)
        packed = idx.pack_allowed(n, mask)
        stray[: packed.shape[0]] = packed
        if n % 8:
            stray[packed.shape[0] - 1] |= np.uint8((0xFF << (n % 8)) & 0xFF)
        sel = idx.Selector.from_bitmap(ix, stray)
        assert sel.count == m, name
        _check(ix, x, q, mask, k, "l2", sel=sel, modes=("scan", "overfetch"))
        sel.close()
    ix.close()


# ---- the list-driven scan (and the two other modes over the same cases) -----------------------------------
SCAN_CASES = [
    # metric, dtype, d, N, m, nq, k
    ("ip", "f32", 100, 3000, 1, 1, 1),
    ("l2", "f32", 1536, 3000, 37, 2, 10),
    ("ip", "f32", 1536, 20000, 5000, 9, 100),
    ("l2", "f32", 100, 20000, 5000, 1, 200),
    ("ip", "bf16", 1536, 3000, 37, 9, 100),     # m < k: padding
    ("l2", "bf16", 100, 20000, 5000, 2, 100),
    ("ip", "bf16", 100, 3000, 1, 2, 10),
    ("l2", "bf16", 1536, 20000, 5000, 1, 200),
    ("ip", "f16", 100, 20000, 5000, 9, 200),
    ("l2", "f16", 1536, 3000, 37, 1, 200),      # m < k: padding, k > 64
    ("ip", "f16", 1536, 20000, 5000, 2, 1),
    ("l2", "f16", 100, 3000, 1, 9, 10),
    ("ip", "f32", 100, 3000, 37, 300, 10),      # more than one 256-query block
    ("l2", "bf16", 32, 200000, 150000, 2, 100),  # ranges longer than one 512-entry batch per workgroup
]


@pytest.mark.parametrize("metric,dtype,d,N,m,nq,k", SCAN_CASES)
def test_scan_cases(idx, metric, dtype, d, N, m, nq, k):
    rng = np.random.default_rng(d * 7 + N + m + nq + k)
    x = rng.standard_normal((N, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    mask = np.zeros(N, dtype=bool)
    mask[rng.choice(N, size=m, replace=False)] = True
    ix = idx.FlatIndex(d, metric, dtype)
    ix.add(x)
    before = (ix.full_scan_count(), ix.uncertified_count())
    _check(ix, O.round_dtype(x, dtype), q, mask, k, metric, modes=("scan",))
    assert (ix.full_scan_count(), ix.uncertified_count()) == before  # the scan tier is counted nowhere
    stats = _check(ix, O.round_dtype(x, dtype), q, mask, k, metric)
    assert stats["scan"]["m"] == m and stats["overfetch"]["tier"] == "overfetch" and stats["overfetch"]["kprime"] >= k
    ix.close()


# ---- ties -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("allowed_copies,k", [(2000, 50), (2000, 1000)])
def test_ties_give_the_lowest_allowed_ids(idx, allowed_copies, k):
    rng = np.random.default_rng(17)
    N, d = 8000, 64
    x = rng.standard_normal((N, d)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    v = x[0].copy()
    copies = np.sort(rng.choice(N, size=6000, replace=False))
    x[copies] = v
    mask = np.zeros(N, dtype=bool)
    mask[copies[::3][:allowed_copies]] = True       # every third identical row
    mask[np.setdiff1d(np.arange(N), copies)[::2]] = True  # and half of the other rows
    q = np.stack([v, x[np.setdiff1d(np.arange(N), copies)[1]]])
    ix = idx.FlatIndex(d, "ip", "f32")
    ix.add(x)
    _check(ix, x, q, mask, k, "ip")
    ix.set_sel_mode("scan")
    _, I = ix.search(q[:1], k, sel=mask)
    np.testing.assert_array_equal(I[0], copies[::3][:allowed_copies][:k])  # the k lowest allowed ids
    ix.set_sel_mode("auto")
    ix.close()


# ---- the overfetch tier ------------------------------------------------------------------------------
def test_overfetch_falls_back_to_the_scan(idx):
    """4,000 copies of query 0 fill every k' <= 3,276 of its unfiltered list and none is allowed: the
    prefix is unproven, and the scan answers the query."""
    rng = np.random.default_rng(23)
    N, d, nq, k = 12000, 64, 16, 10
    x = rng.standard_normal((N, d)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    blocked = np.sort(rng.choice(N, size=4000, replace=False))
    x[blocked] = q[0]
    mask = np.ones(N, dtype=bool)
    mask[blocked] = False
    ix = idx.FlatIndex(d, "ip", "f32")
    ix.add(x)
    stats = _check(ix, x, q, mask, k, "ip")
    assert stats["overfetch"]["tier"] == "overfetch" and stats["overfetch"]["rescanned"] >= 1
    assert stats["overfetch"]["kprime"] < 3276 and stats["overfetch"]["m"] == 8000
    ix.close()


@pytest.mark.parametrize("screen", ["int8", "native"])
def test_overfetch_needs_no_fallback(idx, screen):
    rng = np.random.default_rng(29)
    N, d, nq, k = 20000, 128, 64, 10
    x = rng.standard_normal((N, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    mask = rng.random(N) < 0.5
    ix = idx.FlatIndex(d, "ip", "bf16")
    ix.set_screen(screen)
    ix.add(x)
    stats = _check(ix, O.round_dtype(x, "bf16"), q, mask, k, "ip")
    assert stats["overfetch"]["tier"] == "overfetch" and stats["overfetch"]["rescanned"] == 0
    ix.close()


# ---- lifetime ----------------------------------------------------------------------------------------
def test_selector_lifetime_and_argument_errors(idx):
    from photo_search_engine_amd import _lib
    rng = np.random.default_rng(31)
    n, d = 1000, 48
    x = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((3, d)).astype(np.float32)
    ix = idx.FlatIndex(d, "l2", "f32")
    ix.add(x)
    mask = rng.random(n) < 0.3
    sel = ix.selector(mask)
    ix.add(np.concatenate([q, q, q]))  # the nearest rows of every query, added after the selector
    xs = np.concatenate([x, q, q, q])
    later = np.concatenate([mask, np.zeros(9, dtype=bool)])
    for nq in (1, 3):
        _check(ix, xs, q[:nq], later, 20, "l2", sel=sel)
    _, I = ix.search(q, int(mask.sum()) + 50, sel=sel)
    assert I.max() < n and (I >= 0).sum(axis=1).tolist() == [int(mask.sum())] * 3
    with pytest.raises(_lib.VsError) as e:
        ix.search(q, 0, sel=sel)
    assert e.value.code == _lib.VS_ERR_ARG
    with pytest.raises(_lib.VsError) as e:
        idx.Selector.from_bitmap(ix, np.zeros(((n + 9) + 7) // 8 - 1, dtype=np.uint8))  # one byte short
    assert e.value.code == _lib.VS_ERR_ARG
    other = idx.FlatIndex(d, "l2", "f32")
    other.add(xs)
    with pytest.raises(_lib.VsError) as e:
        other.search(q, 5, sel=sel)  # another index's selector
    assert e.value.code == _lib.VS_ERR_ARG
    other.close()
    ix.reset()
    ix.add(xs)
    with pytest.raises(_lib.VsError) as e:
        ix.search(q, 5, sel=sel)  # stale after reset
    assert e.value.code == _lib.VS_ERR_ARG
    sel.close()
    _check(ix, xs, q, later, 5, "l2")  # a selector made after the reset works
    ix.close()


# ---- concurrency -------------------------------------------------------------------------------------
def test_two_threads_two_selectors(idx):
    rng = np.random.default_rng(37)
    N, d, k = 6000, 96, 10
    x = rng.standard_normal((N, d)).astype(np.float32)
    ix = idx.FlatIndex(d, "ip", "f32")
    ix.add(x)
    masks = [np.arange(N) % 2 == 0, np.arange(N) % 3 == 1]
    qs = [rng.standard_normal((nq, d)).astype(np.float32) for nq in (2, 24)]  # (scan / overfetch under AUTO)
    refs = [filtered_reference(x, qs[t], masks[t], k, "ip") for t in range(2)]
    sels = [ix.selector(m) for m in masks]
    errors = []

    def work(t):
        try:
            for _ in range(15):
                D, I = ix.search(qs[t], k, sel=sels[t])
                np.testing.assert_array_equal(I, refs[t][1])
                np.testing.assert_array_equal(D, refs[t][0])
        except BaseException as exc:  # noqa: BLE001 - reported by the main thread
            errors.append(exc)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    for s in sels:
        s.close()
    ix.close()
    assert not errors, errors[0]


# ---- multi-device --------------------------------------------------------------------------------------
def test_multi_device_filtered_search(idx):
    rng = np.random.default_rng(41)
    N, d, nq, k = 3 * 65536 + 1000, 32, 5, 10
    x = rng.standard_normal((N, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    one_chunk = np.zeros(N, dtype=bool)
    one_chunk[65536 + rng.choice(65536, size=300, replace=False)] = True
    tail = np.zeros(N, dtype=bool)
    tail[3 * 65536 + 7] = True  # fewer allowed rows than k, in the last (partial) chunk
    mi = idx.MultiDeviceFlatIndex(d, "ip", "f32", devices=(0, 0, 0))
    mi.add(x)
    single = idx.FlatIndex(d, "ip", "f32")
    single.add(x)
    for mask in (rng.random(N) < 0.01, one_chunk, tail):
        Dref, Iref = filtered_reference(x, q, mask, k, "ip")
        D, I = mi.search(q, k, sel=mask)
        np.testing.assert_array_equal(I, Iref)
        np.testing.assert_array_equal(D, Dref)
        Ds, Is = single.search(q, k, sel=mask)
        np.testing.assert_array_equal(Is, I)
        np.testing.assert_array_equal(Ds, D)
        D, I = mi.search(q, k, sel=np.flatnonzero(mask))
        np.testing.assert_array_equal(I, Iref)
        ms = mi.selector(mask)
        assert ms.count == int(mask.sum())
        D, I = mi.search(q, k, sel=ms)
        np.testing.assert_array_equal(I, Iref)
        np.testing.assert_array_equal(D, Dref)
    mi.close()
    single.close()
    # shards with fewer rows than k (5 rows on the second device, none on the third)
    n2 = 65536 + 5
    mi = idx.MultiDeviceFlatIndex(d, "ip", "f32", devices=(0, 0, 0))
    mi.add(x[:n2])
    assert mi.shard_rows() == [65536, 5, 0]
    mask = np.zeros(n2, dtype=bool)
    mask[65536:] = True
    mask[rng.choice(65536, size=40, replace=False)] = True
    Dref, Iref = filtered_reference(x[:n2], q, mask, k, "ip")
    D, I = mi.search(q, k, sel=mask)
    np.testing.assert_array_equal(I, Iref)
    np.testing.assert_array_equal(D, Dref)
    mi.close()


# ---- VectorStore -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_vector_store_allowed(tmp_path, metric):
    from photo_search_engine_amd.vector_store import VectorStore
    rng = np.random.default_rng(43)
    n, d = 2000, 64
    X = rng.standard_normal((n, d)).astype(np.float32)
    store = VectorStore(dimension=d, index_path=str(tmp_path / "idx"), metadata_path=str(tmp_path / "meta.json"),
                        metric=metric)
    store.add(X, [{"photo_path": f"/p/{i}.jpg", "year": 2019 + i % 6} for i in range(n)])
    qv = rng.standard_normal((d,)).astype(np.float32)

    def expected(mask, top_k):
        k = min(top_k, n)
        D, I = filtered_reference(store.index.reconstruct_n(0, n), store._normalize_query(qv.tolist()), mask, k,
                                  "ip" if metric == "cosine" else "l2")
        return [{"metadata": store.metadata[i], "distance": float(dist)}
                for dist, i in zip(D[0].tolist(), I[0].tolist()) if i != -1]

    mask = np.array([m["year"] == 2023 for m in store.metadata])
    want = expected(mask, 10)
    assert len(want) == 10
    assert store.search(qv.tolist(), 10, allowed=lambda m: m["year"] == 2023) == want
    assert store.search(qv.tolist(), 10, allowed=mask) == want
    assert store.search(qv.tolist(), 10, allowed=np.flatnonzero(mask).tolist()) == want
    sel = store.selector(lambda m: m["year"] == 2023)
    assert sel.count == int(mask.sum())
    assert store.search(qv.tolist(), 10, allowed=sel) == want
    sel.close()
    three = store.search(qv.tolist(), 10, allowed=[5, 1500, 77])
    assert len(three) == 3 and three == expected(np.isin(np.arange(n), [5, 1500, 77]), 10)
    assert store.search(qv.tolist(), 10, allowed=[]) == []
    assert store.search(qv.tolist(), 10) == expected(np.ones(n, dtype=bool), 10)  # the two-argument call

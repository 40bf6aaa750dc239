"""Exact row removal on the GPU (MI355X only): ``FlatIndex.remove_ids`` (``vs_remove_ids``).

After a removal the index must be indistinguishable from one built by ``add`` of the surviving rows
in order.  Reference for every case: the oracle over ``x_stored[keep]`` -- ``O.round_dtype`` for the
stored values, ``O.knn_exact`` for searches, ``filtered_reference`` (tests/oracle_sel_index.py) for
filtered ones, ``range_reference`` (tests/oracle_range_index.py) for range searches.  Ids and
distances must be bit-equal.
"""
import threading

import numpy as np
import pytest

from oracle import hnsw_oracle as H
from oracle import oracle as O
from oracle_range_index import range_reference
from oracle_sel_index import filtered_reference

pytestmark = pytest.mark.gpu

FLT_MAX = np.float32(3.4028235e38)


@pytest.fixture(scope="module")
def idx():
    from photo_search_engine_amd import index
    return index


def _search_ref(xs, q, k, metric):
    """(D, I) of the exact top-k of ``q`` over rows ``xs`` in faiss layout (k > rows: padded)."""
    nq, n = int(q.shape[0]), int(xs.shape[0])
    D = np.full((nq, k), -FLT_MAX if metric == "ip" else FLT_MAX, dtype=np.float32)
    I = np.full((nq, k), -1, dtype=np.int64)
    kk = min(k, n)
    if kk:
        S, Ik = O.knn_exact(xs, q, kk, metric)
        D[:, :kk] = S.astype(np.float32)
        I[:, :kk] = Ik
    return D, I


def _check_search(ix, xs, q, k, metric, msg=""):
    D, I = ix.search(q, k)
    Dref, Iref = _search_ref(xs, q, k, metric)
    np.testing.assert_array_equal(I, Iref, err_msg=f"ids {msg}")
    np.testing.assert_array_equal(D, Dref, err_msg=f"distances {msg}")


# ---- 1. the compaction pattern ------------------------------------------------------------------------
def _remove_masks(n, rng):
    def rng_mask(lo, hi):
        m = np.zeros(n, dtype=bool)
        m[max(0, min(lo, n)):max(0, min(hi, n))] = True
        return m
    first = np.zeros(n, dtype=bool)
    first[0] = True
    last = np.zeros(n, dtype=bool)
    last[n - 1] = True
    return {"none": np.zeros(n, dtype=bool), "all": np.ones(n, dtype=bool), "first": first, "last": last,
            "alternating": np.arange(n) % 2 == 0, "random_0.1%": rng.random(n) < 0.001,
            "random_50%": rng.random(n) < 0.5, "middle_tile": rng_mask(256, 512), "straddle": rng_mask(200, 300)}


def _compaction_case(idx, n):
    rng = np.random.default_rng(n)
    x = np.zeros((n, 32), dtype=np.float32)
    x[:, 0] = np.arange(n)
    centres = np.linspace(0, n - 1, 6)
    q = np.zeros((centres.shape[0], 32), dtype=np.float32)
    q[:, 0] = np.round(centres)
    for name, mask in _remove_masks(n, rng).items():
        ix = idx.FlatIndex(32, "l2", "f32")
        ix.add(x)
        cap = ix.capacity
        keep = np.flatnonzero(~mask)
        assert ix.remove_ids(mask) == int(mask.sum()), name
        assert ix.ntotal == keep.shape[0] and ix.capacity == cap, name
        got = ix.reconstruct_n(0, keep.shape[0])
        assert got.tobytes() == x[keep].tobytes(), name
        if keep.shape[0]:
            _check_search(ix, x[keep], q, min(100, keep.shape[0] + 3), "l2", name)
            _check_search(ix, x[keep], q[3:4], min(10, keep.shape[0]), "l2", name + " (small-corpus scan)")
            ix.set_scan_limit(0)
            _check_search(ix, x[keep], q[:2], min(10, keep.shape[0]), "l2", name + " (screened)")
        ix.close()


@pytest.mark.parametrize("n", [1, 7, 255, 256, 257, 511, 513, 70001])
def test_compaction(idx, n):
    """Rows x_i = (i, 0, ...) under L2 (as test_gpu_selector.py::test_compaction): a misplaced row shows
    in ``reconstruct_n`` and in the ranking around each query (c, 0, ...)."""
    _compaction_case(idx, n)


def test_compaction_in_one_tile_batches(idx):
    """70,001 rows with the bounce buffer at its floor, one tile: hundreds of batches, each reading
    only rows no earlier batch has written."""
    idx.set_remove_staging_bytes(1)
    try:
        _compaction_case(idx, 70001)
    finally:
        idx.set_remove_staging_bytes(idx.REMOVE_STAGING_DEFAULT)


# ---- 2. every stored form -------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [96, 128])
@pytest.mark.parametrize("screen", ["native", "int8"])
@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_every_stored_form(idx, dtype, metric, screen, d):
    n = 3000
    rng = np.random.default_rng(d * 13 + len(dtype) + (7 if metric == "l2" else 0) + (3 if screen == "int8" else 0))
    x = rng.standard_normal((n, d)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    if metric == "l2":  # norms over 2^-3 .. 2^3: a misplaced sqn entry changes the ranking
        x *= np.exp2(rng.uniform(-3.0, 3.0, size=(n, 1))).astype(np.float32)
    q = rng.standard_normal((32, d)).astype(np.float32)
    mask = rng.random(n) < 0.3
    ix = idx.FlatIndex(d, metric, dtype)
    ix.set_screen(screen)
    ix.add(x)
    ix.set_scan_limit(0)
    assert ix.remove_ids(mask) == int(mask.sum())
    xs = O.round_dtype(x, dtype)[~mask]
    assert ix.reconstruct_n(0, xs.shape[0]).tobytes() == xs.tobytes()
    for nq in (1, 4, 32):
        for k in (10, 100):
            _check_search(ix, xs, q[:nq], k, metric, f"nq={nq} k={k}")
    ix.close()


# ---- 3. group residuals ---------------------------------------------------------------------------------
def _clustered(n, d, n_clusters, sigma, seed):
    """normalise(c[cid] + sigma g), inserted cluster by cluster (the recipe of
    tests/test_gpu_int8_clustered.py ``_mixture``, sort=True, with numpy's generator; g has unit
    norm in expectation instead of exactly)."""
    c = np.random.default_rng(900 + d).standard_normal((n_clusters, d), dtype=np.float32)  # (shared centres)
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d), dtype=np.float32)
    x *= np.float32(sigma / np.sqrt(d))
    x += c[np.sort(rng.integers(0, n_clusters, n))]
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x


# Group residuals belong to the direct int8 screen, which needs a padded int8 dimension of at least
# 512 (include/vs.h): at d = 128 the index keeps no group means, so the case runs there
# without them and at d = 512, the smallest dimension that has them, with them.  Batches screen the
# group-residual codes only from 1024 tiles on (4 per CU; below, the native screen answers), so the
# third case keeps that many after the removal.
@pytest.mark.parametrize("n,d,groups", [(2 * 4096 + 500, 128, False), (2 * 4096 + 500, 512, True),
                                        (72 * 4096 + 500, 512, True)])
def test_group_residuals(idx, n, d, groups):
    x = _clustered(n, d, max(4, n // 2200), 0.3, 31 + d)
    q = _clustered(32, d, max(4, n // 2200), 0.3, 77 + d)
    ix = idx.FlatIndex(d, "ip", "bf16")
    ix.set_screen("int8")
    ix.add(x)
    ix.set_scan_limit(0)
    st = ix.screen_state()
    assert st["screen"] == 1 and st["group_residuals"] == int(groups)
    rng = np.random.default_rng(5)
    mask = rng.random(n) < 0.1
    mask[4000:4201] = True  # crosses the edge of groups 0 and 1
    assert ix.remove_ids(mask) == int(mask.sum())
    assert ix.screen_state()["group_residuals"] == int(groups)
    xs = O.round_dtype(x, "bf16")[~mask]
    assert ix.reconstruct_n(0, xs.shape[0]).tobytes() == xs.tobytes()
    ix.set_timing(True)
    for rep in range(2):
        _check_search(ix, xs, q, 10, "ip")
        if rep == 0 and xs.shape[0] >= 1024 * 256:  # the batch did screen the requantised codes
            assert ix.timing_fetch()[1] == "mfma_i8"
    ix.close()


# ---- 4. add after remove --------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,metric,screen", [("f32", "l2", "native"), ("bf16", "ip", "int8")])
def test_add_after_remove(idx, dtype, metric, screen):
    n, d = 2000, 96
    rng = np.random.default_rng(41)
    x = rng.standard_normal((n + 600, d)).astype(np.float32)
    q = rng.standard_normal((16, d)).astype(np.float32)
    ix = idx.FlatIndex(d, metric, dtype)
    ix.set_screen(screen)
    ix.add(x[:n])
    ix.set_scan_limit(0)
    cap = ix.capacity
    xs = O.round_dtype(x, dtype)
    mask = rng.random(n) < 0.25
    assert ix.remove_ids(mask) == int(mask.sum()) and ix.capacity == cap
    ix.add(x[n:n + 300])
    cur = np.concatenate([xs[:n][~mask], xs[n:n + 300]])
    assert ix.ntotal == cur.shape[0] and ix.reconstruct_n(0, cur.shape[0]).tobytes() == cur.tobytes()
    for nq in (2, 16):
        _check_search(ix, cur, q[:nq], 20, metric, f"after add, nq={nq}")
    cap = ix.capacity
    mask2 = rng.random(cur.shape[0]) < 0.25
    mask2[-5:] = True  # rows added after the first removal go too
    assert ix.remove_ids(np.flatnonzero(mask2)) == int(mask2.sum()) and ix.capacity == cap
    cur = cur[~mask2]
    ix.add(x[n + 300:])
    cur = np.concatenate([cur, xs[n + 300:]])
    assert ix.reconstruct_n(0, cur.shape[0]).tobytes() == cur.tobytes()
    for nq in (2, 16):
        _check_search(ix, cur, q[:nq], 20, metric, f"after the second round, nq={nq}")
    ix.close()


# ---- 5. stale and fresh handles ---------------------------------------------------------------------------
def test_stale_and_fresh_handles(idx):
    from photo_search_engine_amd import _lib
    from photo_search_engine_amd.hnsw import HNSWGraph
    n, d = 1500, 48
    rng = np.random.default_rng(53)
    x = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((5, d)).astype(np.float32)
    ix = idx.FlatIndex(d, "ip", "f32")
    ix.add(x)
    allowed = rng.random(n) < 0.4
    sel = ix.selector(allowed)
    g = H.layered_knn_graph(x, 6, "ip", seed=4)
    hg = HNSWGraph(ix, g)
    S_ref, I_ref = H.search(x, g, q, 5, 32, "ip")
    # a removal of nothing leaves both usable
    assert ix.remove_ids(np.zeros(n, dtype=bool)) == 0 and ix.remove_ids([]) == 0
    Dref, Iref = filtered_reference(x, q, allowed, 10, "ip")
    D, I = ix.search(q, 10, sel=sel)
    assert np.array_equal(I, Iref) and np.array_equal(D, Dref)
    D, I = hg.search(q, 5, 32)
    assert np.array_equal(I, I_ref) and np.array_equal(D, S_ref.astype(np.float32))
    # a removal of one row makes both stale
    mask = np.zeros(n, dtype=bool)
    mask[700] = True
    assert ix.remove_ids(mask) == 1
    with pytest.raises(_lib.VsError):
        ix.search(q, 10, sel=sel)
    with pytest.raises(_lib.VsError):
        ix.range_search(q, 0.0, sel=sel)
    with pytest.raises(_lib.VsError):
        hg.search(q, 5, 32)
    sel.close()
    hg.close()
    # fresh ones speak of the shifted rows
    xs = x[~mask]
    allowed2 = allowed[~mask]
    sel2 = ix.selector(allowed2)
    Dref, Iref = filtered_reference(xs, q, allowed2, 10, "ip")
    for mode in ("scan", "overfetch", "auto"):
        ix.set_sel_mode(mode)
        D, I = ix.search(q, 10, sel=sel2)
        assert np.array_equal(I, Iref) and np.array_equal(D, Dref), mode
    ix.set_sel_mode("auto")
    radius = np.float32(np.sort(O.canon_scores(xs, q, "ip"), axis=1)[:, -40].min())
    for s, m in ((None, None), (sel2, allowed2)):
        lims, D, I = ix.range_search(q, radius, sel=s)
        lr, Dr, Ir = range_reference(xs, q, radius, "ip", mask=m)
        assert np.array_equal(lims, lr) and np.array_equal(I, Ir) and np.array_equal(D, Dr)
    sel2.close()
    g2 = H.layered_knn_graph(xs, 6, "ip", seed=4)
    hg2 = HNSWGraph(ix, g2)
    S_ref, I_ref = H.search(xs, g2, q, 5, 32, "ip")
    D, I = hg2.search(q, 5, 32)
    assert np.array_equal(I, I_ref) and np.array_equal(D, S_ref.astype(np.float32))
    hg2.close()
    ix.close()


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_range_screen_tier_after_removal(idx, dtype):
    """The range search's MFMA screen tier (bf16 / f16 rows, blocks of 9..256 queries) over compacted rows."""
    n, d = 5000, 128
    rng = np.random.default_rng(59)
    x = rng.standard_normal((n, d)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    q = rng.standard_normal((16, d)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    mask = rng.random(n) < 0.2
    ix = idx.FlatIndex(d, "ip", dtype)
    ix.add(x)
    ix.remove_ids(mask)
    xs = O.round_dtype(x, dtype)[~mask]
    for mode in ("screen", "scan"):
        ix.set_range_mode(mode)
        lims, D, I = ix.range_search(q, 0.15)
        lr, Dr, Ir = range_reference(xs, q, 0.15, "ip")
        assert lr[-1] > 0 and np.array_equal(lims, lr) and np.array_equal(I, Ir) and np.array_equal(D, Dr), mode
    ix.close()


# ---- 6. edges -------------------------------------------------------------------------------------------
def test_edges(idx):
    from photo_search_engine_amd import _lib
    n, d = 1000, 40
    rng = np.random.default_rng(61)
    x = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((3, d)).astype(np.float32)
    ix = idx.FlatIndex(d, "ip", "f32")
    ix.add(x)
    # a short bitmap raises and leaves the index as it was
    with pytest.raises(_lib.VsError):
        ix.remove_bitmap(np.full((n + 7) // 8 - 1, 0xFF, dtype=np.uint8))
    assert ix.ntotal == n
    _check_search(ix, x, q, 10, "ip", "after the refused call")
    # stray bits past ntotal are ignored (n = 1000: a whole number of bytes, so over-long; and a
    # partial last byte after one more removal)
    stray = np.zeros((n + 7) // 8 + 9, dtype=np.uint8)
    stray[n // 8:] = 0xFF
    assert ix.remove_bitmap(stray) == 0 and ix.ntotal == n
    stray[0] = 0x05  # rows 0 and 2
    assert ix.remove_bitmap(stray) == 2 and ix.ntotal == n - 2
    xs = x[np.r_[1, 3:n]]
    _check_search(ix, xs, q, 10, "ip", "stray bits")
    m = n - 2  # 998: six live bits in the last byte
    stray = np.zeros((m + 7) // 8, dtype=np.uint8)
    stray[-1] = 0xFF & ~0x3F | 0x20  # bits 6, 7 (rows 998, 999: past ntotal) and bit 5 (row 997)
    assert ix.remove_bitmap(stray) == 1 and ix.ntotal == m - 1
    xs = xs[:-1]
    assert ix.reconstruct_n(0, m - 1).tobytes() == xs.tobytes()
    # remove all: an empty index, capacity kept, and add works after
    cap = ix.capacity
    assert ix.remove_ids(np.ones(m - 1, dtype=bool)) == m - 1
    assert ix.ntotal == 0 and ix.capacity == cap
    empty = idx.FlatIndex(d, "ip", "f32")
    De, Ie = empty.search(q, 4)
    D, I = ix.search(q, 4)
    assert np.array_equal(I, Ie) and np.array_equal(D, De) and (I == -1).all()
    empty.close()
    assert ix.remove_ids([]) == 0 and ix.remove_bitmap(np.zeros(0, dtype=np.uint8)) == 0
    ix.add(x[:300])
    _check_search(ix, x[:300], q, 10, "ip", "add after remove-all")
    ix.close()


# ---- 7. bookkeeping -------------------------------------------------------------------------------------
def test_bookkeeping(idx, tmp_path):
    from photo_search_engine_amd import _lib
    n, d = 4000, 64
    rng = np.random.default_rng(67)
    x = rng.standard_normal((n, d)).astype(np.float32)
    ix = idx.FlatIndex(d, "l2", "bf16")
    ix.set_screen("int8")
    ix.add(x)
    ix.search(x[:2], 5)
    live = int(_lib.load().vs_device_bytes_live())
    copy = ix.screen_copy_bytes()
    mask = rng.random(n) < 0.5
    assert ix.remove_ids(mask) == int(mask.sum())
    assert int(_lib.load().vs_device_bytes_live()) == live  # the bounce buffer and the id list are gone
    assert ix.screen_copy_bytes() == copy
    xs = O.round_dtype(x, "bf16")[~mask]
    path = str(tmp_path / "rows.bin")
    ix.write_rows(path, 0, 0, xs.shape[0])
    assert open(path, "rb").read() == xs.astype("<f4").tobytes()
    ix.close()


# ---- 8. concurrency -------------------------------------------------------------------------------------
def test_search_while_removing(idx):
    """One thread searches in a loop while another removes once: the exclusive lock puts each search
    wholly before or wholly after the removal."""
    n, d, k = 20000, 64, 10
    rng = np.random.default_rng(71)
    x = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((12, d)).astype(np.float32)
    mask = rng.random(n) < 0.3
    before = _search_ref(x, q, k, "ip")
    after = _search_ref(x[~mask], q, k, "ip")
    assert not np.array_equal(before[1], after[1])
    ix = idx.FlatIndex(d, "ip", "f32")
    ix.add(x)
    results, errors = [], []
    started, removed = threading.Event(), threading.Event()

    def searcher():
        try:
            tail = 0
            while tail < 3:  # (three more searches once the removal has returned)
                if removed.is_set():
                    tail += 1
                results.append(ix.search(q, k))
                started.set()
        except Exception as e:  # pragma: no cover - reported below
            errors.append(e)
            started.set()

    def remover():
        try:
            started.wait(60)
            ix.remove_ids(mask)
        except Exception as e:  # pragma: no cover - reported below
            errors.append(e)
        finally:
            removed.set()

    ts = [threading.Thread(target=searcher), threading.Thread(target=remover)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(120)
    assert not any(t.is_alive() for t in ts) and not errors, errors
    kinds = []
    for D, I in results:
        if np.array_equal(I, before[1]) and np.array_equal(D, before[0]):
            kinds.append(0)
        else:
            assert np.array_equal(I, after[1]) and np.array_equal(D, after[0])
            kinds.append(1)
    assert kinds == sorted(kinds) and kinds[0] == 0 and kinds[-1] == 1
    ix.close()


# ---- 9. VectorStore over the HIP index ----------------------------------------------------------------------
def test_vector_store_remove_items(tmp_path):
    from photo_search_engine_amd.vector_store import VectorStore
    n, d = 600, 64
    rng = np.random.default_rng(73)
    X = rng.standard_normal((n, d)).astype(np.float32)
    kw = dict(index_path=str(tmp_path / "photo_search.index"), metadata_path=str(tmp_path / "metadata.json"))
    store = VectorStore(dimension=d, **kw)
    for i in range(n):
        store.add_item(X[i].tolist(), {"photo_path": f"/photos/{i}.jpg", "i": i})
    xs = store.index.reconstruct_n(0, n)
    gone = sorted(rng.choice(n, size=50, replace=False).tolist())
    assert store.remove_items([f"/photos/{i}.jpg" for i in gone] + ["/photos/none.jpg"]) == 50
    keep = np.setdiff1d(np.arange(n), gone)
    assert store.get_total_items() == n - 50 and [m["i"] for m in store.metadata] == keep.tolist()

    def check(s):
        for j in (0, 17, n - 51):
            vec = xs[keep[j]].tolist()
            qn = s._normalize_query(vec)
            S, I = O.knn_exact(xs[keep], qn, 8, "ip")
            res = s.search(vec, 8)
            assert [r["metadata"]["i"] for r in res] == keep[I[0]].tolist()
            assert [r["distance"] for r in res] == S[0].astype(np.float32).tolist()
            assert res[0]["metadata"]["photo_path"] == f"/photos/{keep[j]}.jpg"
        assert not any(s.has_photo_path(f"/photos/{i}.jpg") for i in gone)
        assert s.get_embedding_by_photo_path(f"/photos/{keep[-1]}.jpg") == xs[keep[-1]].tolist()

    check(store)
    store.save()
    s2 = VectorStore(dimension=d, **kw)
    assert s2.load() and s2.get_total_items() == n - 50
    assert s2.index.reconstruct_n(0, n - 50).tobytes() == xs[keep].tobytes()
    check(s2)
    # update_item: the row is replaced and moves to the end
    v = rng.standard_normal(d).astype(np.float32)
    store.update_item(v.tolist(), {"photo_path": f"/photos/{keep[3]}.jpg", "i": int(keep[3]), "edited": True})
    assert store.get_total_items() == n - 50 and store.metadata[-1]["edited"]
    res = store.search(v.tolist(), 1)
    assert res[0]["metadata"]["i"] == int(keep[3]) and res[0]["metadata"].get("edited")

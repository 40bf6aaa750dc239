"""Exact k-means over stored rows on the GPU (MI355X only): ``vs_kmeans`` through ``FlatIndex.kmeans`` /
``assign_rows``, ``IVFFlatIndex.train_from``, ``VectorStore.cluster_items`` and the multi-device route.

Reference for every case (tests/oracle_kmeans.py): assignment is the oracle's exact top-1 over the
centroids, the update is the segment rule of include/vs.h in explicit loops.  Centroids, labels,
distances, counts, ``changed`` and ``n_iter`` must be bit-equal; ``objective`` may differ by the
worst-case fp64 summation error of any order, ``m * 2^-52 * sum |S_ref|``."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import ivf_oracle as IO
from oracle import oracle as O
from oracle_kmeans import kmeans_reference, oracle_kmeans_factory

pytestmark = pytest.mark.gpu

N = 700  # three row tiles, the last one partial


@pytest.fixture(scope="module")
def idx():
    from photo_search_engine_amd import index
    return index


@functools.lru_cache(maxsize=None)
def _blobs(n, d, k, sigma, seed):
    """Clustered rows, uneven clusters, ids in no cluster order."""
    rng = np.random.default_rng(seed)
    centers = rng.standard_normal((k, d)).astype(np.float32)
    centers /= np.linalg.norm(centers, axis=1, keepdims=True)
    p = np.arange(1, k + 1, dtype=np.float64) ** 1.5
    which = rng.choice(k, size=n, p=p / p.sum())
    x = centers[which] + np.float32(sigma) * rng.standard_normal((n, d)).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _edge_rows():
    """1300 rows in four tight groups of exactly 256, 513, 1 and 530 rows, ids shuffled; returns the
    rows and the four group centres."""
    rng = np.random.default_rng(11)
    d = 40
    centers = np.zeros((4, d), dtype=np.float32)
    for c in range(4):
        centers[c, c] = 4.0
    which = np.repeat(np.arange(4), [256, 513, 1, 530])
    rng.shuffle(which)
    x = centers[which] + np.float32(0.05) * rng.standard_normal((1300, d)).astype(np.float32)
    x.setflags(write=False)
    centers.setflags(write=False)
    return x, centers


def _index(idx, x, dtype, metric="l2"):
    ix = idx.FlatIndex(x.shape[1], metric, dtype)
    ix.add(np.ascontiguousarray(x))
    return ix


def _check(res, ref, what=""):
    m = ref["labels"].shape[0]
    np.testing.assert_array_equal(res.labels, ref["labels"], err_msg=f"{what}: labels")
    np.testing.assert_array_equal(res.counts, ref["counts"], err_msg=f"{what}: counts")
    np.testing.assert_array_equal(res.changed, ref["changed"], err_msg=f"{what}: changed")
    assert res.n_iter == ref["n_iter"], what
    np.testing.assert_array_equal(res.centroids.view(np.uint32), ref["centroids"].view(np.uint32),
                                  err_msg=f"{what}: centroids")
    np.testing.assert_array_equal(res.distances.view(np.uint32), ref["D"].view(np.uint32), err_msg=f"{what}: D")
    assert res.objective.shape == ref["objective"].shape
    tol = m * 2.0 ** -52 * ref["abs_sums"]  # worst-case fp64 summation error of any order, per pass
    assert (np.abs(res.objective - ref["objective"]) <= tol).all(), (what, res.objective, ref["objective"])


def _seed_init(xs, ids, k, seed):
    return np.ascontiguousarray(xs[ids[np.sort(np.random.default_rng(seed).permutation(ids.shape[0])[:k])]])


def _raw(ix, sel, k, niter, metric, c, m, D=True, counts=True, labels=True, centroids=True):
    """``vs_kmeans`` itself, outputs pre-filled with sentinels: (rc, centroids, labels, D, counts,
    objective, changed, iters_done)."""
    lab = np.full((max(m, 1),), -7, dtype=np.int64)
    Dv = np.full((max(m, 1),), -7.0, dtype=np.float32)
    cnt = np.full((max(k, 1),), -7, dtype=np.int64)
    obj = np.full((max(niter, 0) + 1,), -7.0, dtype=np.float64)
    chg = np.full((max(niter, 0) + 1,), -7, dtype=np.int64)
    done = ctypes.c_int32(-7)
    rc = ix._L.vs_kmeans(ix._h, sel._h if sel is not None else None, k, niter, metric,
                         c.ctypes.data if centroids else None, lab.ctypes.data if labels else None,
                         Dv.ctypes.data if D else None, cnt.ctypes.data if counts else None, obj.ctypes.data,
                         chg.ctypes.data, ctypes.byref(done))
    return rc, c, lab, Dv, cnt, obj, chg, int(done.value)


# ---- 1. dtypes and metrics ------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("dtype,d", [("f32", 33), ("bf16", 72), ("f16", 72)])
def test_dtype_metric_sweep(idx, dtype, d, metric):
    x = _blobs(N, d, 5, 0.3, 1)
    xs = O.round_dtype(x, dtype)
    ids = np.arange(N)
    init = _seed_init(xs, ids, 5, 1234)
    ref = kmeans_reference(xs, ids, init, 3, metric)
    assert len(set(ref["counts"].tolist())) > 2  # uneven clusters
    ix = _index(idx, x, dtype, "ip")  # (the assignment metric is the call's, not the index's)
    res = ix.kmeans(5, niter=3, metric=metric)  # init None: the seed recipe, rows fetched with reconstruct
    _check(res, ref, f"{dtype} {metric}")
    if metric == "ip":  # metric None = the index's own
        _check(ix.kmeans(5, niter=3), ref, "index metric")
    ix.close()


# ---- 2. segment edges -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_segment_edges(idx, dtype):
    x, centers = _edge_rows()
    xs = O.round_dtype(x, dtype)
    ids = np.arange(1300)
    first = kmeans_reference(xs, ids, centers, 0, "l2")
    assert first["counts"].tolist() == [256, 513, 1, 530]  # one full segment; two and one row; one row; two and a part
    ref = kmeans_reference(xs, ids, centers, 2, "l2")
    ix = _index(idx, x, dtype)
    _check(ix.kmeans(4, niter=2, init=centers), ref, dtype)
    ix.close()


# ---- 3. more than one sort digit, empty clusters ---------------------------------------------------------
def test_many_clusters_and_empty_ones(idx):
    x, _ = _edge_rows()
    xs = O.round_dtype(x, "bf16")
    ids = np.arange(1300)
    rng = np.random.default_rng(5)
    init = np.empty((300, x.shape[1]), dtype=np.float32)
    near = rng.permutation(300)[:170]
    init[:] = 60.0 + rng.standard_normal(init.shape).astype(np.float32)  # far from every row: empty
    init[near] = xs[np.sort(rng.permutation(1300)[:170])]
    ref = kmeans_reference(xs, ids, init, 2, "l2")
    empty = ref["counts"] == 0
    assert empty.sum() >= 100 and np.median(ref["counts"][~empty]) <= 8 and (np.flatnonzero(~empty) >= 256).any()
    ix = _index(idx, x, "bf16")
    res = ix.kmeans(300, niter=2, init=init)
    _check(res, ref, "k=300")
    np.testing.assert_array_equal(res.centroids[empty].view(np.uint32), init[empty].view(np.uint32))
    ix.close()


# ---- 4. ties --------------------------------------------------------------------------------------------
def test_equal_centroids_go_to_the_lower_id(idx):
    x = _blobs(N, 72, 5, 0.3, 1)
    xs = O.round_dtype(x, "bf16")
    ids = np.arange(N)
    ix = _index(idx, x, "bf16")
    far = np.full((2, 72), 9.0, dtype=np.float32)  # twins far from every row: the lower id takes all
    res = ix.kmeans(2, niter=5, init=far)
    _check(res, kmeans_reference(xs, ids, far, 5, "l2"), "far twins")
    assert res.counts.tolist() == [N, 0] and res.n_iter == 1
    np.testing.assert_array_equal(res.centroids[1], far[1])
    init = np.stack([xs[5], xs[5], xs[400]])  # twins among the rows
    labels, _ = ix.assign_rows(init)
    assert (labels != 1).all() and (labels == 0).any()
    _check(ix.kmeans(3, niter=3, init=init), kmeans_reference(xs, ids, init, 3, "l2"), "twins")
    ix.close()


# ---- 5. k = 1 and k = m ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_one_cluster_and_one_cluster_per_member(idx, dtype):
    x = _blobs(N, 72, 5, 0.3, 1)
    xs = O.round_dtype(x, dtype)
    ids = np.array([3, 100, 255, 256, 257, 300, 511, 600, 699])
    ix = _index(idx, x, dtype)
    sel = ix.selector(ids)
    res = ix.kmeans(1, niter=2, init=xs[[3]], sel=sel)
    mean = np.zeros((72,), dtype=np.float64)
    for i in ids:  # m = 9: a single segment
        mean += xs[i].astype(np.float64)
    np.testing.assert_array_equal(res.centroids[0], (mean / np.float64(9)).astype(np.float32))
    _check(res, kmeans_reference(xs, ids, xs[[3]], 2, "l2"), "k=1")
    assert res.n_iter == 1 and res.changed.tolist() == [9, 0]
    res = ix.kmeans(9, niter=4, init=ids, sel=sel)  # every member its own centroid: a fixed point at once
    np.testing.assert_array_equal(res.centroids, xs[ids])
    assert res.labels.tolist() == list(range(9)) and res.changed.tolist() == [9, 0] and res.n_iter == 1
    _check(res, kmeans_reference(xs, ids, xs[ids], 4, "l2"), "k=m")
    sel.close()
    ix.close()


# ---- 6. selectors, after a removal ----------------------------------------------------------------------
def test_selector_members_after_remove_ids(idx):
    x = _blobs(N, 72, 5, 0.3, 1)
    ix = _index(idx, x, "bf16")
    old = ix.selector(np.arange(0, N, 3))
    gone = np.array([0, 7, 250, 300])
    assert ix.remove_ids(gone) == 4
    xs = np.delete(O.round_dtype(x, "bf16"), gone, axis=0)
    with pytest.raises(Exception):
        ix.kmeans(3, niter=1, sel=old)
    ids = np.union1d(np.arange(0, N - 4, 3), [255, 256])
    sel = ix.selector(ids)
    assert sel.count == ids.shape[0]
    for metric in ("ip", "l2"):
        init = _seed_init(xs, ids, 4, 99)
        res = ix.kmeans(4, niter=3, seed=99, sel=sel, metric=metric)
        assert res.labels.shape[0] == sel.count
        _check(res, kmeans_reference(xs, ids, init, 3, metric), f"sel {metric}")
    res = ix.kmeans(4, niter=3, seed=99, sel=ids, metric="l2")  # ids in place of a selector
    _check(res, kmeans_reference(xs, ids, _seed_init(xs, ids, 4, 99), 3, "l2"), "ids")
    sel.close()
    old.close()
    ix.close()


# ---- 7. early stop --------------------------------------------------------------------------------------
def test_early_stop_leaves_the_tail_untouched(idx):
    x = _blobs(N, 72, 5, 0.05, 2)
    xs = O.round_dtype(x, "bf16")
    ids = np.arange(N)
    init = _seed_init(xs, ids, 5, 1234)
    ref = kmeans_reference(xs, ids, init, 40, "l2")
    assert ref["n_iter"] < 40 and ref["changed"][-1] == 0
    ix = _index(idx, x, "bf16")
    _check(ix.kmeans(5, niter=40), ref, "early stop")
    rc, c, lab, Dv, cnt, obj, chg, done = _raw(ix, None, 5, 40, 1, init.copy(), N)
    n = ref["n_iter"]
    assert rc == 0 and done == n
    np.testing.assert_array_equal(chg[: n + 1], ref["changed"])
    assert (chg[n + 1:] == -7).all() and (obj[n + 1:] == -7.0).all() and (obj[: n + 1] != -7.0).all()
    np.testing.assert_array_equal(c, ref["centroids"])
    np.testing.assert_array_equal(lab, ref["labels"])
    ix.close()


# ---- 8. off unit scale ----------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("log2scale", [20, -20])
def test_off_unit_scale(idx, log2scale, metric):
    x = _blobs(N, 72, 5, 0.3, 1) * np.float32(2.0 ** log2scale)
    xs = O.round_dtype(x, "bf16")
    ids = np.arange(N)
    init = _seed_init(xs, ids, 5, 1234)
    ix = _index(idx, x, "bf16")
    res = ix.kmeans(5, niter=3, metric=metric)
    _check(res, kmeans_reference(xs, ids, init, 3, metric), f"2^{log2scale} {metric}")
    ix.close()


# ---- 9. chunk independence ------------------------------------------------------------------------------
def test_staging_size_and_reruns_change_no_bit(idx):
    x = _blobs(N, 72, 5, 0.3, 1)
    ix = _index(idx, x, "bf16")
    runs = []
    try:
        idx.set_kmeans_staging_bytes(1)  # one 256-row block per chunk: three chunks
        runs.append(ix.kmeans(5, niter=3))
    finally:
        idx.set_kmeans_staging_bytes()
    runs.append(ix.kmeans(5, niter=3))
    runs.append(ix.kmeans(5, niter=3))
    for r in runs[1:]:
        for name in ("centroids", "labels", "distances", "counts", "objective", "changed"):
            a, b = getattr(runs[0], name), getattr(r, name)
            assert a.tobytes() == b.tobytes(), name
        assert r.n_iter == runs[0].n_iter
    with pytest.raises(Exception):
        idx.set_kmeans_staging_bytes(0)
    ix.close()


# ---- 10. niter = 0 --------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_niter_zero_is_assign_rows_is_search(idx, metric):
    x = _blobs(N, 72, 5, 0.3, 1)
    xs = O.round_dtype(x, "f16")
    ix = _index(idx, x, "f16")
    ids = np.arange(1, N, 2)
    init = _seed_init(xs, ids, 6, 3)
    res = ix.kmeans(6, niter=0, init=init, sel=ids, metric=metric)
    labels, dist = ix.assign_rows(init, sel=ids, metric=metric)
    np.testing.assert_array_equal(res.labels, labels)
    np.testing.assert_array_equal(res.distances, dist)
    np.testing.assert_array_equal(res.centroids, init)
    assert res.n_iter == 0 and res.changed.tolist() == [ids.shape[0]]
    cx = idx.FlatIndex(72, metric, "f32")
    cx.add(init)
    D, I = cx.search(xs[ids], 1)
    np.testing.assert_array_equal(labels, I[:, 0])
    np.testing.assert_array_equal(dist, D[:, 0])
    _check(res, kmeans_reference(xs, ids, init, 0, metric), "niter=0")
    cx.close()
    ix.close()


# ---- 11. workspace accounting, argument errors ----------------------------------------------------------
def test_workspace_is_freed_and_argument_errors_touch_nothing(idx):
    x = _blobs(N, 72, 5, 0.3, 1)
    xs = O.round_dtype(x, "bf16")
    ix = _index(idx, x, "bf16")
    L = ix._L
    sel = ix.selector(np.arange(9))
    ix.search(xs[:3], 2)  # (the index's own context and its row-reading buffers exist before the
    ix.reconstruct(0)     #  measurement: the wrapper fetches the initial centroids with reconstruct)
    before = int(L.vs_device_bytes_live())
    ix.kmeans(5, niter=2)
    assert int(L.vs_device_bytes_live()) == before
    init = np.ascontiguousarray(xs[:5]) + np.float32(0.25)
    cases = [dict(k=0), dict(k=-1), dict(k=N + 1), dict(k=10, sel=sel), dict(niter=-1), dict(metric=2), dict(metric=-2),
             dict(centroids=False), dict(labels=False)]
    for case in cases:
        c = init.copy() if case.get("k", 5) <= 5 else np.zeros((case["k"], 72), dtype=np.float32)
        keep = c.copy()
        s = case.get("sel")
        rc = _raw(ix, s, case.get("k", 5), case.get("niter", 2), case.get("metric", 1), c, 9 if s else N,
                  centroids=case.get("centroids", True), labels=case.get("labels", True))[0]
        assert rc == -1, case  # VS_ERR_ARG
        np.testing.assert_array_equal(c, keep)
        assert int(L.vs_device_bytes_live()) == before
    # D and counts may be NULL
    rc, c, lab, *_ = _raw(ix, None, 5, 2, 1, init.copy(), N, D=False, counts=False)
    assert rc == 0
    np.testing.assert_array_equal(lab, kmeans_reference(xs, np.arange(N), init, 2, "l2")["labels"])
    # no members: only k < 1 fails
    empty = idx.FlatIndex(72, "l2", "bf16")
    rc, c, lab, Dv, cnt, obj, chg, done = _raw(empty, None, 3, 2, 1, init[:3].copy(), 0)
    assert rc == 0 and done == 0 and cnt.tolist() == [0, 0, 0] and chg[0] == 0 and obj[0] == 0.0
    assert _raw(empty, None, 0, 2, 1, init[:3].copy(), 0)[0] == -1
    empty.close()
    sel.close()
    ix.close()


# ---- 12. end to end -------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_ivf_train_from(idx, metric):
    from photo_search_engine_amd.ivf import IVFFlatIndex
    x = _blobs(N, 72, 5, 0.3, 1)
    xs = O.round_dtype(x, "bf16")
    ids = np.arange(N)
    flat = _index(idx, x, "bf16")
    ivf = IVFFlatIndex(72, 8, metric, "bf16")
    ivf.train_from(flat, niter=4, seed=21)
    ref = kmeans_reference(xs, ids, _seed_init(xs, ids, 8, 21), 4, metric)
    c = ivf.centroids()
    np.testing.assert_array_equal(c, O.round_dtype(ref["centroids"], "bf16"))  # (an IVF stores them in its dtype)
    ivf.add(x)
    q = np.ascontiguousarray(x[::50]) + np.float32(0.01)
    D, I = ivf.search(q, 5, 3)
    lists = IO.assign(xs, c, metric)
    S, Ie = IO.search(xs, ids, lists, c, q, 5, 3, metric)
    np.testing.assert_array_equal(I, Ie)
    De = S.astype(np.float32)
    De[Ie < 0] = -3.4028235e38 if metric == "ip" else 3.4028235e38
    np.testing.assert_array_equal(D, De)
    ivf.close()
    flat.close()


@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_cluster_items_equals_the_oracle_backed_store(monkeypatch, tmp_path, metric):
    from photo_search_engine_amd import vector_store as vsmod
    x = _blobs(300, 24, 4, 0.2, 3)
    meta = [{"photo_path": f"/p/{i}.jpg", "year": 2020 + i % 5} for i in range(300)]

    def build(tag):
        s = vsmod.VectorStore(dimension=24, index_path=str(tmp_path / f"{tag}.idx"),
                              metadata_path=str(tmp_path / f"{tag}.json"), metric=metric)
        s.add(np.ascontiguousarray(x), meta)
        return s

    gpu = build("gpu")
    monkeypatch.setattr(vsmod, "_index_factory", oracle_kmeans_factory)
    cpu = build("cpu")
    for allowed in (None, lambda m: m["year"] != 2022, np.arange(0, 300, 7)):
        got = gpu.cluster_items(4, allowed=allowed, niter=6)
        assert got == cpu.cluster_items(4, allowed=allowed, niter=6)
        assert sum(g["size"] for g in got) == (300 if allowed is None else len(gpu._allowed_mask(allowed).nonzero()[0]))


def test_multi_device_route_equals_one_device(idx):
    x = _blobs(N, 72, 5, 0.3, 1)
    one = _index(idx, x, "bf16")
    multi = idx.MultiDeviceFlatIndex(72, "l2", "bf16", devices=(0, 0))
    multi.add(np.ascontiguousarray(x))
    mask = np.arange(N) % 4 != 1
    for sel in (None, mask):
        a, b = one.kmeans(5, niter=3, sel=sel), multi.kmeans(5, niter=3, sel=sel)
        for name in ("centroids", "labels", "distances", "counts", "objective", "changed"):
            assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), name
        assert a.n_iter == b.n_iter
    la, da = one.assign_rows(a.centroids, sel=mask)
    lb, db = multi.assign_rows(a.centroids, sel=multi.selector(mask))
    np.testing.assert_array_equal(la, lb)
    np.testing.assert_array_equal(da, db)
    multi.close()
    one.close()

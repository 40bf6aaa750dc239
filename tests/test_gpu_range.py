"""Exact range search on the GPU (MI355X only): every row within a score radius.

Reference for every case (tests/oracle_range_index.py ``range_reference``): the oracle's canonical fp64
scores of the stored values (``O.round_dtype``), members where the fp32 value passes the radius
strictly, restricted to the mask, ordered by (score, then id).  ``lims``, distances and ids must be
bit-equal under the scan tier, the screen tier (where it applies) and the library's own choice.
"""
import threading

import numpy as np
import pytest

from oracle import oracle as O
from oracle_range_index import range_reference

pytestmark = pytest.mark.gpu

RS_SORT_MAX = 4096
K_MAX = 3276  # KP_MAX * 4 / 5


@pytest.fixture(scope="module")
def idx():
    from photo_search_engine_amd import index
    return index


def _modes(dtype, nq, sel):
    screen = sel is None and dtype in ("bf16", "f16") and nq >= 9
    return ("scan", "screen", "auto") if screen else ("scan", "auto")


def _check(ix, xs, q, radius, metric, mask=None, sel=None, modes=None, ref=None):
    """Range-search under every mode, compare each with the reference; returns (reference, stats per mode)."""
    ref = ref if ref is not None else range_reference(xs, q, radius, metric, mask)
    s = sel if sel is not None else mask
    stats = {}
    try:
        for mode in modes or _modes(ix.dtype, q.shape[0], s):
            ix.set_range_mode(mode)
            lims, D, I = ix.range_search(q, radius, sel=s)
            np.testing.assert_array_equal(lims, ref[0], err_msg=f"lims, mode {mode}")
            np.testing.assert_array_equal(I, ref[2], err_msg=f"ids, mode {mode}")
            np.testing.assert_array_equal(D, ref[1], err_msg=f"distances, mode {mode}")
            stats[mode] = ix.range_last_stats()
            assert stats[mode]["total"] == int(ref[0][-1])
    finally:
        ix.set_range_mode("auto")
    if "scan" in stats:
        assert stats["scan"]["tier"] == "scan" and stats["scan"]["rescanned"] == 0
    return ref, stats


def _kth_D(xs, q, metric, rank):
    """fp32 D of each query's rank-th best row (1-based)."""
    S, _ = O.knn_exact(xs, q, rank, metric)
    return S[:, rank - 1].astype(np.float32)


# ---- membership boundary -------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_membership_boundary(idx, metric):
    rng = np.random.default_rng(5)
    N, d, nq = 2000, 64, 6
    x = rng.standard_normal((N, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    ix = idx.FlatIndex(d, metric, "f32")
    ix.add(x)
    D10 = _kth_D(x, q, metric, 10)
    S, I = O.knn_exact(x, q, 10, metric)
    assert (S[:, 8].astype(np.float32) != D10).all()  # (the 9th and the 10th are apart in fp32)
    # the radius is exactly the 10th best row's D: strict, so that row is out and the 9 better are in
    (lims, D, Ir), _ = _check(ix, x, q, D10, metric)
    assert np.diff(lims).tolist() == [9] * nq
    np.testing.assert_array_equal(Ir.reshape(nq, 9), I[:, :9])
    # one fp32 step past it: the row is in
    looser = np.nextafter(D10, np.float32(-np.inf if metric == "ip" else np.inf))
    (lims, D, Ir), _ = _check(ix, x, q, looser, metric)
    assert (np.diff(lims) >= 10).all()
    for i in range(nq):
        assert Ir[lims[i] + 9] == I[i, 9] and D[lims[i] + 9] == D10[i]
    ix.close()


def test_rows_equal_in_fp32_are_both_in_or_both_out(idx):
    """Two rows whose fp64 scores differ (1.5 and 1.5 + 2^-40) and round to the same fp32 value: the
    predicate is on the fp32 value, so no radius separates them."""
    d = 64
    x = np.zeros((40, d), dtype=np.float32)
    x[:, 2] = np.linspace(-1, 1, 40)  # (other rows, scores 0)
    x[7, 0], x[21, 0] = 1.5, 1.5
    x[21, 1] = 2.0 ** -20
    q = np.zeros((1, d), dtype=np.float32)
    q[0, 0], q[0, 1] = 1.0, 2.0 ** -20
    S = O.canon_scores(x, q, "ip")
    assert S[0, 7] != S[0, 21] and np.float32(S[0, 7]) == np.float32(S[0, 21]) == np.float32(1.5)
    ix = idx.FlatIndex(d, "ip", "f32")
    ix.add(x)
    (lims, _, I), _ = _check(ix, x, q, np.float32(1.5), "ip")
    assert lims[1] == 0
    (lims, _, I), _ = _check(ix, x, q, np.nextafter(np.float32(1.5), np.float32(-np.inf)), "ip")
    assert I.tolist() == [21, 7]  # (the larger fp64 score first)
    ix.close()


# ---- ties -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_ties_come_in_id_order(idx, dtype):
    rng = np.random.default_rng(11)
    N, d = 3000, 64
    x = rng.standard_normal((N, d)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    copies = np.sort(rng.choice(N, size=300, replace=False))
    x[copies] = x[copies[0]]
    xs = O.round_dtype(x, dtype)
    q = np.repeat(xs[copies[:1]], 9, axis=0) * 4.0
    score = O.canon_scores(xs[copies[:1]], q, "ip")[:, 0].astype(np.float32)
    ix = idx.FlatIndex(d, "ip", dtype)
    ix.add(x)
    (lims, _, I), _ = _check(ix, xs, q, np.nextafter(score, np.float32(-np.inf)), "ip")
    for i in range(9):
        np.testing.assert_array_equal(I[lims[i]:lims[i + 1]], copies)
    ix.close()


# ---- shapes -------------------------------------------------------------------------------------------
# every N of {1, 255, 256, 257, 3000, 20000}, d of {100, 1536}, dtype, metric and nq of {1, 2, 9, 256, 257}
# occurs, each N with both d and several dtypes (a covering selection, not the 360-case product)
SHAPE_CASES = [
    # metric, dtype, d, N, nq, infinite radii
    ("ip", "f32", 100, 1, 1, False),
    ("l2", "bf16", 1536, 1, 9, False),
    ("ip", "f16", 100, 255, 2, False),
    ("l2", "bf16", 1536, 255, 9, False),
    ("l2", "f32", 1536, 256, 9, False),
    ("ip", "f16", 100, 256, 256, False),
    ("ip", "bf16", 1536, 257, 257, False),
    ("l2", "f16", 100, 257, 256, False),
    ("ip", "f32", 1536, 3000, 2, True),
    ("l2", "bf16", 100, 3000, 9, True),
    ("ip", "f16", 1536, 3000, 257, True),
    ("l2", "f32", 100, 3000, 1, True),
    ("ip", "bf16", 100, 20000, 256, False),
    ("l2", "f16", 1536, 20000, 9, False),
    ("l2", "f32", 100, 20000, 257, False),
    ("ip", "f32", 1536, 20000, 1, False),
    ("l2", "bf16", 1536, 20000, 256, False),
    ("ip", "f16", 100, 20000, 2, False),
]


@pytest.mark.parametrize("metric,dtype,d,N,nq,inf", SHAPE_CASES)
def test_shapes(idx, metric, dtype, d, N, nq, inf):
    """Per-query radii in one batch: query 0 gets no row, query 1 (or the only one) every row, the
    others the D of a rank between 1 and 300 (so that many rows minus one); with ``inf`` the
    every-row radius is -inf / +inf."""
    rng = np.random.default_rng(d * 3 + N + nq)
    x = rng.standard_normal((N, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    xs = O.round_dtype(x, dtype)
    kk = min(N, 300)
    S, _ = O.knn_exact(xs, q, kk, metric)
    ranks = rng.integers(0, kk, size=nq)
    r = S[np.arange(nq), ranks].astype(np.float32)
    big = np.float32(np.inf) if inf else np.float32(1e30)
    none_r, all_r = (big, -big) if metric == "ip" else (-big, big)
    r[0] = none_r
    r[min(1, nq - 1)] = all_r
    ix = idx.FlatIndex(d, metric, dtype)
    ix.add(x)
    (lims, _, _), stats = _check(ix, xs, q, r, metric)
    counts = np.diff(lims)
    assert counts[min(1, nq - 1)] == N and (nq == 1 or counts[0] == 0)
    assert stats["auto"]["host_sorted"] == (1 if N > RS_SORT_MAX else 0)
    if "screen" in stats:
        assert stats["screen"]["tier"] == "screen" and stats["auto"]["tier"] == "screen"
    # one scalar radius for the batch
    _check(ix, xs, q, float(np.median(S[:, kk // 2])), metric, modes=("auto",))
    ix.close()


def test_empty_inputs_and_argument_errors(idx):
    from photo_search_engine_amd import _lib
    d = 48
    ix = idx.FlatIndex(d, "ip", "f32")
    q = np.ones((3, d), dtype=np.float32)
    lims, D, I = ix.range_search(q, 0.0)  # an empty index: all-zero lims
    assert lims.tolist() == [0, 0, 0, 0] and D.shape == (0,) and I.shape == (0,)
    ix.add(np.ones((5, d), dtype=np.float32))
    lims, D, I = ix.range_search(np.zeros((0, d), dtype=np.float32), 0.0)  # nq = 0
    assert lims.tolist() == [0] and D.shape == (0,)
    with pytest.raises(ValueError):
        ix.range_search(q, np.float32(np.nan))
    L = ix._L  # the C ABI rejects NaN itself
    r = np.array([0.0, np.nan, 0.0], dtype=np.float32)
    import ctypes
    h = ctypes.c_void_p()
    rc = L.vs_range_search(ix._h, None, q.ctypes.data, 3, r.ctypes.data, 0, ctypes.byref(h))
    assert rc == _lib.VS_ERR_ARG and "NaN" in _lib.last_error() and not h.value
    with pytest.raises(ValueError):
        ix.set_range_mode("overfetch")
    ix.close()


# ---- sort boundary ------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,host_sorted", [(RS_SORT_MAX - 1, 0), (RS_SORT_MAX, 0), (RS_SORT_MAX + 1, 1)])
def test_sort_boundary(idx, m, host_sorted):
    """Rows x_i = (i, 0, ...) under L2 and the query at the origin: distance i^2, so the radius
    (m - 1/2)^2 returns exactly the m rows 0 .. m - 1, in that order."""
    n, d = 5000, 32
    x = np.zeros((n, d), dtype=np.float32)
    x[:, 0] = np.arange(n)
    q = np.zeros((2, d), dtype=np.float32)
    r = np.array([np.float32((m - 0.5) ** 2), np.float32(2.25)], dtype=np.float32)
    ix = idx.FlatIndex(d, "l2", "f32")
    ix.add(x)
    (lims, _, I), stats = _check(ix, x, q, r, "l2")
    assert lims.tolist() == [0, m, m + 2]
    np.testing.assert_array_equal(I[:m], np.arange(m))
    assert stats["scan"]["host_sorted"] == host_sorted and stats["auto"]["host_sorted"] == host_sorted
    ix.close()


# ---- the screen tier ------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("nq", [9, 256])
def test_screen_without_overflow(idx, nq, metric):
    """79 tiles, one per workgroup: 256 rows never exceed a workgroup's 512 kept slots, so no list is
    cut and no query goes to the scan."""
    rng = np.random.default_rng(13 + nq)
    N, d = 20000, 100
    x = rng.standard_normal((N, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    xs = O.round_dtype(x, "bf16")
    ix = idx.FlatIndex(d, metric, "bf16")
    ix.add(x)
    (lims, _, _), stats = _check(ix, xs, q, _kth_D(xs, q, metric, 40), metric)
    assert np.diff(lims).tolist() == [39] * nq
    for mode in ("screen", "auto"):
        assert stats[mode]["tier"] == "screen" and stats[mode]["rescanned"] == 0, mode
    ix.set_screen("int8")  # the int8 setting does not apply to range searches
    _, stats = _check(ix, xs, q, _kth_D(xs, q, metric, 40), metric, modes=("screen",))
    assert stats["screen"]["tier"] == "screen"
    ix.close()


def test_screen_overflow_goes_to_the_scan(idx):
    """4,000 copies of one vector stored contiguously and a radius just below their score: with at
    most 256 workgroups over 300,000 rows one workgroup spans more than 1,000 rows, above its 768
    slots, so it compacts -- the query's list may be incomplete and the scan answers it."""
    rng = np.random.default_rng(19)
    N, d, nq = 300000, 64, 9
    x = rng.standard_normal((N, d)).astype(np.float32)
    v = x[100000].copy()
    x[100000:104000] = v
    xs = O.round_dtype(x, "bf16")
    q = (v[None, :] * (1.0 + 0.01 * np.arange(nq))[:, None] + 0.01 * rng.standard_normal((nq, d))).astype(np.float32)
    score = O.canon_scores(xs[100000:100001], q, "ip")[:, 0].astype(np.float32)
    ix = idx.FlatIndex(d, "ip", "bf16")
    ix.add(x)
    (lims, _, _), stats = _check(ix, xs, q, np.nextafter(score, np.float32(-np.inf)), "ip")
    assert (np.diff(lims) >= 4000).all()
    for mode in ("screen", "auto"):
        assert stats[mode]["tier"] == "screen" and stats[mode]["rescanned"] >= 1, mode
    ix.close()


def test_screen_overflow_of_some_queries_of_a_block(idx):
    """The construction above with 9 random queries in the same block, each with the radius of its 40th
    best row: their lists are complete and the refine answers them, while the scan answers the 9 whose
    list a workgroup cut -- one block, both tiers, every query through exactly one of them.  The commit
    before the shared tier driver reported 9 re-answered queries under both modes, hence `== 9`."""
    rng = np.random.default_rng(19)
    N, d, nq = 300000, 64, 9
    x = rng.standard_normal((N, d)).astype(np.float32)
    v = x[100000].copy()
    x[100000:104000] = v
    xs = O.round_dtype(x, "bf16")
    q = (v[None, :] * (1.0 + 0.01 * np.arange(nq))[:, None] + 0.01 * rng.standard_normal((nq, d))).astype(np.float32)
    score = O.canon_scores(xs[100000:100001], q, "ip")[:, 0].astype(np.float32)
    q2 = rng.standard_normal((nq, d)).astype(np.float32)
    q = np.concatenate([q, q2])
    radius = np.concatenate([np.nextafter(score, np.float32(-np.inf)), _kth_D(xs, q2, "ip", 40)])
    ix = idx.FlatIndex(d, "ip", "bf16")
    ix.add(x)
    (lims, _, _), stats = _check(ix, xs, q, radius, "ip")
    assert (np.diff(lims)[:nq] >= 4000).all() and np.diff(lims)[nq:].tolist() == [39] * nq
    for mode in ("screen", "auto"):
        assert stats[mode]["tier"] == "screen" and stats[mode]["rescanned"] == 9, mode
    ix.close()


# ---- consistency with top-k ---------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,dtype,nq", [("ip", "f32", 3), ("l2", "bf16", 12), ("ip", "f16", 2)])
def test_range_result_is_a_prefix_of_topk(idx, metric, dtype, nq):
    rng = np.random.default_rng(23 + nq)
    N, d = 9000, 96
    x = rng.standard_normal((N, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    xs = O.round_dtype(x, dtype)
    ranks = rng.integers(2, K_MAX, size=nq)
    S, _ = O.knn_exact(xs, q, K_MAX, metric)
    r = S[np.arange(nq), ranks].astype(np.float32)
    ix = idx.FlatIndex(d, metric, dtype)
    ix.add(x)
    lims, D, I = ix.range_search(q, r)
    for i in range(nq):
        count = int(lims[i + 1] - lims[i])
        assert 0 < count <= K_MAX
        Dk, Ik = ix.search(q[i:i + 1], count)
        np.testing.assert_array_equal(I[lims[i]:lims[i + 1]], Ik[0])
        np.testing.assert_array_equal(D[lims[i]:lims[i + 1]], Dk[0])
    ix.close()


# ---- selector ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [37, 5000])
@pytest.mark.parametrize("metric,dtype,nq", [("ip", "bf16", 12), ("l2", "f32", 2)])
def test_selector(idx, m, metric, dtype, nq):
    from photo_search_engine_amd import _lib
    rng = np.random.default_rng(29 + m)
    N, d = 20000, 64
    x = rng.standard_normal((N, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    xs = O.round_dtype(x, dtype)
    mask = np.zeros(N, dtype=bool)
    mask[rng.choice(N, size=m, replace=False)] = True
    r = _kth_D(xs, q, metric, 200)
    r[0] = np.float32(-np.inf if metric == "ip" else np.inf)  # every allowed row
    ix = idx.FlatIndex(d, metric, dtype)
    ix.add(x)
    (lims, _, _), stats = _check(ix, xs, q, r, metric, mask=mask)
    assert lims[1] == m and stats["auto"]["tier"] == "scan"
    _check(ix, xs, q, r, metric, mask=mask, sel=np.flatnonzero(mask), modes=("auto",))
    sel = ix.selector(mask)
    ix.add(np.concatenate([q, q]))  # the nearest rows of every query, added after the selector
    xs2 = np.concatenate([xs, O.round_dtype(np.concatenate([q, q]), dtype)])
    later = np.concatenate([mask, np.zeros(2 * nq, dtype=bool)])
    (_, _, I), _ = _check(ix, xs2, q, r, metric, mask=later, sel=sel)
    assert I.max() < N
    ix.reset()
    ix.add(x)
    with pytest.raises(_lib.VsError) as e:
        ix.range_search(q, r, sel=sel)  # stale after reset
    assert e.value.code == _lib.VS_ERR_ARG
    sel.close()
    ix.close()


# ---- max_total ---------------------------------------------------------------------------------------------
def test_max_total(idx):
    from photo_search_engine_amd import _lib
    rng = np.random.default_rng(31)
    N, d, nq = 4000, 64, 300  # (two query blocks: the count goes on past the cap)
    x = rng.standard_normal((N, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    ix = idx.FlatIndex(d, "ip", "f32")
    ix.add(x)
    r = _kth_D(x, q, "ip", 30)
    ref = range_reference(x, q, r, "ip")
    total = int(ref[0][-1])
    assert total == 29 * nq
    lims, D, I = ix.range_search(q, r, max_total=total)
    np.testing.assert_array_equal(I, ref[2])
    for cap in (total - 1, 100):
        with pytest.raises(_lib.VsError) as e:
            ix.range_search(q, r, max_total=cap)
        assert e.value.code == _lib.VS_ERR_ARG and str(total) in str(e.value)
    _check(ix, x, q, r, "ip", ref=ref)  # the handle works after the error
    ix.close()


# ---- multi-device -------------------------------------------------------------------------------------------
def test_multi_device_range_search(idx):
    rng = np.random.default_rng(37)
    N, d, nq = 200000, 32, 5  # 4 chunks of 2^16 ids over 3 shards
    x = rng.standard_normal((N, d)).astype(np.float32)
    x[70000:70040] = x[5]  # equal scores across shards: the merge orders them by global id
    q = rng.standard_normal((nq, d)).astype(np.float32)
    q[0] = x[5]
    r = _kth_D(x, q, "ip", 120)
    r[1] = _kth_D(x, q[1:2], "ip", 6000)[0]  # (a segment past the LDS sort)
    mi = idx.MultiDeviceFlatIndex(d, "ip", "f32", devices=(0, 0, 0))
    mi.add(x)
    single = idx.FlatIndex(d, "ip", "f32")
    single.add(x)
    for mask in (None, rng.random(N) < 0.3):
        ref = range_reference(x, q, r, "ip", mask)
        lims, D, I = mi.range_search(q, r, sel=mask)
        np.testing.assert_array_equal(lims, ref[0])
        np.testing.assert_array_equal(I, ref[2])
        np.testing.assert_array_equal(D, ref[1])
        ls, Ds, Is = single.range_search(q, r, sel=mask)
        np.testing.assert_array_equal(ls, lims)
        np.testing.assert_array_equal(Is, I)
        np.testing.assert_array_equal(Ds, D)
    ms = mi.selector(np.arange(N) % 7 == 0)
    ref = range_reference(x, q, r, "ip", np.arange(N) % 7 == 0)
    lims, D, I = mi.range_search(q, r, sel=ms)
    np.testing.assert_array_equal(I, ref[2])
    from photo_search_engine_amd import _lib
    with pytest.raises(_lib.VsError) as e:
        mi.range_search(q, r, max_total=10)
    assert e.value.code == _lib.VS_ERR_ARG
    mi.close()
    single.close()


# ---- concurrency ---------------------------------------------------------------------------------------------
def test_four_threads_range_and_topk(idx):
    rng = np.random.default_rng(41)
    N, d, k = 6000, 96, 10
    x = rng.standard_normal((N, d)).astype(np.float32)
    xs = O.round_dtype(x, "bf16")
    ix = idx.FlatIndex(d, "ip", "bf16")
    ix.add(x)
    qs = [rng.standard_normal((nq, d)).astype(np.float32) for nq in (2, 24, 2, 24)]
    rads = [_kth_D(xs, qv, "ip", 50) for qv in qs]
    range_refs = [range_reference(xs, qs[t], rads[t], "ip") for t in range(4)]
    topk_refs = []
    for t in range(4):
        S, I = O.knn_exact(xs, qs[t], k, "ip")
        topk_refs.append((S.astype(np.float32), I))
    errors = []

    def work(t):
        try:
            for _ in range(10):
                if t < 2:  # (the scan under AUTO for 2 queries, the screen for 24)
                    lims, D, I = ix.range_search(qs[t], rads[t])
                    np.testing.assert_array_equal(lims, range_refs[t][0])
                    np.testing.assert_array_equal(I, range_refs[t][2])
                    np.testing.assert_array_equal(D, range_refs[t][1])
                else:
                    D, I = ix.search(qs[t], k)
                    np.testing.assert_array_equal(I, topk_refs[t][1])
                    np.testing.assert_array_equal(D, topk_refs[t][0])
        except BaseException as exc:  # noqa: BLE001 - reported by the main thread
            errors.append(exc)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    ix.close()
    assert not errors, errors[0]


# ---- VectorStore ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index_type,metric", [("flat", "cosine"), ("flat", "l2"), ("hnsw", "cosine")])
def test_vector_store_search_range(tmp_path, index_type, metric):
    from photo_search_engine_amd.vector_store import VectorStore
    rng = np.random.default_rng(43)
    n, d = 2000, 64
    X = rng.standard_normal((n, d)).astype(np.float32)
    store = VectorStore(dimension=d, index_path=str(tmp_path / "idx"), metadata_path=str(tmp_path / "meta.json"),
                        metric=metric, index_type=index_type)
    store.add(X, [{"photo_path": f"/p/{i}.jpg", "year": 2019 + i % 6} for i in range(n)])
    qv = rng.standard_normal((d,)).astype(np.float32)
    m = "ip" if metric == "cosine" else "l2"
    rows = store.index.reconstruct_n(0, n)
    qn = store._normalize_query(qv.tolist())
    radius = float(_kth_D(rows, qn, m, 25)[0])

    def expected(mask):
        _, D, I = range_reference(rows, qn, radius, m, mask)
        return [{"metadata": store.metadata[i], "distance": float(dist)} for dist, i in zip(D.tolist(), I.tolist())]

    want = expected(None)
    assert len(want) == 24
    assert store.search_range(qv.tolist(), radius) == want
    assert store.search_range(qv.tolist(), radius, max_results=5) == want[:5]
    # the floor cut of the searcher: search(top_k) cut at the radius
    cut = [r for r in store.search(qv.tolist(), 100)
           if (r["distance"] > np.float32(radius) if m == "ip" else r["distance"] < np.float32(radius))]
    assert [r["metadata"]["photo_path"] for r in cut] == [r["metadata"]["photo_path"] for r in want]
    mask = np.array([md["year"] == 2023 for md in store.metadata])
    loose = float(_kth_D(rows, qn, m, 400)[0])
    _, D, I = range_reference(rows, qn, loose, m, mask)
    got = store.search_range(qv.tolist(), loose, allowed=lambda md: md["year"] == 2023)
    assert [r["metadata"]["photo_path"] for r in got] == [f"/p/{i}.jpg" for i in I.tolist()]
    assert [r["distance"] for r in got] == D.tolist()
    assert store.search_range(qv.tolist(), loose, allowed=[]) == []

"""Exact score selectors on the GPU (MI355X only): selectors built on the device from a range predicate.

Reference for every case (tests/oracle_scoresel_index.py ``scoresel_reference``): the union (ANY) or the
intersection (ALL) of ``range_reference``'s lists, complemented within the members under ``negate``.  The
selector's ``bitmap`` and ``count`` must be bit-equal under the scan tier, the screen tier (where it applies)
and the library's own choice.
"""
import threading

import numpy as np
import pytest

from oracle import oracle as O
from oracle_scoresel_index import oracle_scoresel_factory, scoresel_reference

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def idx():
    from photo_search_engine_amd import index
    return index


def _tiers(dtype, nq, sel):
    screen = sel is None and dtype in ("bf16", "f16") and nq >= 9
    return ("scan", "screen", "auto") if screen else ("scan", "auto")


def _bits(mask):
    return np.packbits(np.asarray(mask, dtype=bool), bitorder="little")


def _assert_selector(s, want, what=""):
    """``s`` is exactly the boolean mask ``want`` over the rows it covers: count, bitmap (tail zero), mask."""
    n = want.shape[0]
    assert s.count == int(want.sum()), what
    bm = s.bitmap
    assert bm.dtype == np.uint8 and bm.shape == ((n + 7) // 8,), what
    np.testing.assert_array_equal(bm, _bits(want), err_msg=what)  # (packbits pads with zero: the tail is zero)
    np.testing.assert_array_equal(s.to_mask(), want, err_msg=what)


def _check(ix, xs, q, radius, metric, mode="any", negate=False, mask=None, sel=None, tiers=None, want=None):
    """``selector_from_range`` under every applicable tier against the reference; returns (the reference
    mask, stats per tier)."""
    if want is None:
        want = scoresel_reference(xs, q, radius, metric, mode, negate, mask)
    s_arg = sel if sel is not None else mask
    stats = {}
    try:
        for tier in tiers or _tiers(ix.dtype, q.shape[0], s_arg):
            ix.set_range_mode(tier)
            s = ix.selector_from_range(q, radius, mode=mode, negate=negate, sel=s_arg)
            try:
                _assert_selector(s, want, f"{tier} / {mode} / negate={negate}")
            finally:
                s.close()
            st = stats[tier] = ix.scoresel_last_stats()
            assert st["m"] == int(want.sum())
            if tier == "scan":
                assert st["tier"] in ("scan", "none") and st["rescanned"] == 0
    finally:
        ix.set_range_mode("auto")
    return want, stats


def _kth_D(xs, q, metric, rank):
    """fp32 D of each query's rank-th best row (1-based)."""
    S, _ = O.knn_exact(xs, q, rank, metric)
    return S[:, rank - 1].astype(np.float32)


# ---- parity ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def parity_corpus():
    rng = np.random.default_rng(3)
    N, d = 3000, 64  # 47 workgroups of the scan, a last partial wave-step, a last word of 56 bits
    x = rng.standard_normal((N, d)).astype(np.float32)
    q = rng.standard_normal((20, d)).astype(np.float32)
    return x, q


@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_parity(idx, parity_corpus, dtype, metric):
    x, q = parity_corpus
    N = x.shape[0]
    xs = O.round_dtype(x, dtype)
    ix = idx.FlatIndex(x.shape[1], metric, dtype)
    ix.add(x)
    for nq in (1, 6, 20):  # (20 reaches the screen for bf16 / f16)
        for rank in (10, 500):
            r = _kth_D(xs, q[:nq], metric, rank)
            for mode in ("any", "all"):
                for negate in (False, True):
                    want, stats = _check(ix, xs, q[:nq], r, metric, mode, negate)
                    if nq == 1:
                        assert int(want.sum()) == (N - (rank - 1) if negate else rank - 1)
                    if "screen" in stats:
                        assert stats["screen"]["tier"] == "screen" and stats["auto"]["tier"] == "screen"
    ix.close()


# ---- word boundaries ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [63, 64, 65, 2049])
def test_word_boundaries(idx, N):
    rng = np.random.default_rng(5)
    d = 32
    x = rng.standard_normal((N, d)).astype(np.float32)
    q = rng.standard_normal((3, d)).astype(np.float32)
    ix = idx.FlatIndex(d, "ip", "f32")
    ix.add(x)
    every = np.float32(-np.inf)
    for mode in ("any", "all"):
        want, _ = _check(ix, x, q, every, "ip", mode)
        assert want.all()
        s = ix.selector_from_range(q, every, mode=mode)
        bm = s.bitmap
        assert s.count == N and bm.shape[0] == (N + 7) // 8
        assert np.unpackbits(bm, bitorder="little")[:N].all() and not np.unpackbits(bm, bitorder="little")[N:].any()
        s.close()
        want, _ = _check(ix, x, q, every, "ip", mode, negate=True)
        assert not want.any()
        s = ix.selector_from_range(q, every, mode=mode, negate=True)
        assert s.count == 0 and not s.bitmap.any()  # the tail is still zero
        s.close()
    ix.close()


# ---- membership boundary -----------------------------------------------------------------------------------
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
    looser = np.nextafter(D10, np.float32(-np.inf if metric == "ip" else np.inf))
    for j in range(nq):
        # the radius is exactly the 10th best row's D: strict, so that row is out and the 9 better are in
        want, _ = _check(ix, x, q[j:j + 1], D10[j:j + 1], metric)
        assert int(want.sum()) == 9 and not want[I[j, 9]] and want[I[j, :9]].all()
        # one fp32 step past it: the row is in
        want, _ = _check(ix, x, q[j:j + 1], looser[j:j + 1], metric)
        assert int(want.sum()) >= 10 and want[I[j, 9]]
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
    want, _ = _check(ix, x, q, np.float32(1.5), "ip")
    assert not want.any()
    want, _ = _check(ix, x, q, np.nextafter(np.float32(1.5), np.float32(-np.inf)), "ip")
    assert np.flatnonzero(want).tolist() == [7, 21]
    ix.close()


# ---- contention --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["any", "all"])
def test_every_row_passes_every_query(idx, mode):
    """Maximal contention: 20 queries, every row passing -- under ANY every thread hits the same words."""
    rng = np.random.default_rng(15)
    N, d, nq = 5000, 48, 20
    x = rng.standard_normal((N, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    xs = O.round_dtype(x, "bf16")
    ix = idx.FlatIndex(d, "ip", "bf16")
    ix.add(x)
    want, _ = _check(ix, xs, q, np.float32(-np.inf), "ip", mode)
    assert want.all()
    want, _ = _check(ix, xs, q, np.float32(-np.inf), "ip", mode, negate=True)
    assert not want.any()
    ix.close()


# ---- ALL staging -------------------------------------------------------------------------------------------
def test_all_staging_blocks(idx):
    rng = np.random.default_rng(21)
    N, d, nq = 2000, 64, 20
    x = rng.standard_normal((N, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    xs = O.round_dtype(x, "bf16")
    ix = idx.FlatIndex(d, "ip", "bf16")
    ix.add(x)
    r = _kth_D(xs, q, "ip", 1800)
    want, stats = _check(ix, xs, q, r, "ip", "all")
    assert 0 < int(want.sum()) < N
    assert all(st["blocks"] == 1 for st in stats.values()) and stats["auto"]["tier"] == "screen"
    nwords = (N + 63) // 64
    try:
        idx.set_scoresel_staging_bytes(1)  # below one query's bitmap: one query per block
        _, stats = _check(ix, xs, q, r, "ip", "all", want=want)
        assert all(st["blocks"] == 20 and st["tier"] == "scan" for st in stats.values())
        idx.set_scoresel_staging_bytes(8 * nwords * 7 + 5)  # 7 queries per block: 7 + 7 + 6
        _, stats = _check(ix, xs, q, r, "ip", "all", want=want)
        assert all(st["blocks"] == 3 for st in stats.values())
        _, stats = _check(ix, xs, q, r, "ip", "any")  # ANY takes whole blocks whatever the setting
        assert all(st["blocks"] == 1 for st in stats.values())
    finally:
        idx.set_scoresel_staging_bytes()
    ix.close()


# ---- base selector -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,nq", [("f32", 3), ("bf16", 12)])
def test_base_selector(idx, dtype, nq):
    rng = np.random.default_rng(9)
    N, n0, d = 3000, 2500, 64
    x = rng.standard_normal((N, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    xs = O.round_dtype(x, dtype)
    ix = idx.FlatIndex(d, "ip", dtype)
    ix.add(x[:n0])
    early_mask = rng.random(n0) < 0.5
    early = ix.selector(early_mask)  # a base made before rows were added
    ix.add(x[n0:])
    r = _kth_D(xs, q, "ip", 300)
    some = rng.random(N) < 0.3
    for mode in ("any", "all"):
        for negate in (False, True):
            want, _ = _check(ix, xs, q, r, "ip", mode, negate, mask=some)
            assert not (want & ~some).any()  # a subset of the base, under negate too
            want, _ = _check(ix, xs, q, r, "ip", mode, negate, mask=early_mask, sel=early)
            assert want.shape == (N,) and not want[n0:].any()  # the rows added later are never selected
            assert not (want[:n0] & ~early_mask).any()
            want, _ = _check(ix, xs, q, r, "ip", mode, negate, mask=np.zeros(N, dtype=bool))  # an empty base
            assert not want.any()
    # a stale base
    assert ix.remove_ids([5]) == 1
    with pytest.raises(RuntimeError, match="stale"):
        ix.selector_from_range(q, r, sel=early)
    early.close()
    ix.close()


# ---- the screen tier ---------------------------------------------------------------------------------------
def test_screen_overflow_goes_to_the_scan(idx):
    """The construction of test_gpu_range.py: 4,000 copies of one vector stored contiguously and a radius
    just below their score, so a workgroup of the screen compacts its list.  The scan answers the query over
    the bits its refine set: none lost, and a bit set twice is a bit set."""
    rng = np.random.default_rng(19)
    N, d, nq = 300000, 64, 9
    x = rng.standard_normal((N, d)).astype(np.float32)
    v = x[100000].copy()
    x[100000:104000] = v
    xs = O.round_dtype(x, "bf16")
    q = (v[None, :] * (1.0 + 0.01 * np.arange(nq))[:, None] + 0.01 * rng.standard_normal((nq, d))).astype(np.float32)
    score = O.canon_scores(xs[100000:100001], q, "ip")[:, 0].astype(np.float32)
    r = np.nextafter(score, np.float32(-np.inf))
    ix = idx.FlatIndex(d, "ip", "bf16")
    ix.add(x)
    for mode in ("any", "all"):
        want, stats = _check(ix, xs, q, r, "ip", mode)
        assert want[100000:104000].all()
        for tier in ("screen", "auto"):
            assert stats[tier]["tier"] == "screen" and stats[tier]["rescanned"] >= 1, (tier, mode)
    ix.close()


def test_query_outside_lds(idx):
    """d = 6400: the fp64 query (50 KiB) is not staged in LDS (the QLDS = false instantiations)."""
    rng = np.random.default_rng(17)
    N, d, nq = 300, 6400, 2
    x = rng.standard_normal((N, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    mask = rng.random(N) < 0.5
    for dtype, metric in (("f32", "ip"), ("bf16", "l2")):
        xs = O.round_dtype(x, dtype)
        ix = idx.FlatIndex(d, metric, dtype)
        ix.add(x)
        r = _kth_D(xs, q, metric, 100)
        for mode in ("any", "all"):
            _check(ix, xs, q, r, metric, mode)
            _check(ix, xs, q, r, metric, mode, mask=mask)
        ix.close()


def test_query_blocks(idx):
    rng = np.random.default_rng(22)
    N, d = 2000, 64
    x = rng.standard_normal((N, d)).astype(np.float32)
    q = rng.standard_normal((300, d)).astype(np.float32)  # 256 + 44 queries
    xs = O.round_dtype(x, "bf16")
    ix = idx.FlatIndex(d, "ip", "bf16")
    ix.add(x)
    for mode, rank in (("any", 5), ("all", 1990)):
        want, stats = _check(ix, xs, q, _kth_D(xs, q, "ip", rank), "ip", mode)
        assert 0 < int(want.sum()) < N and all(st["blocks"] == 2 for st in stats.values())
    ix.close()


# ---- queries from stored rows ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,metric", [("f32", "l2"), ("bf16", "ip")])
def test_from_range_rows(idx, dtype, metric):
    rng = np.random.default_rng(31)
    N, d = 1500, 64
    x = rng.standard_normal((N, d)).astype(np.float32)
    xs = O.round_dtype(x, dtype)
    ix = idx.FlatIndex(d, metric, dtype)
    ix.add(x)
    ids = np.array([7, 1499, 0, 640, 7, 33, 901, 77, 1200, 5, 64, 63], dtype=np.int64)  # (a repeat; 12 reach the screen)
    rows = np.stack([ix.reconstruct(int(i)) for i in ids])
    np.testing.assert_array_equal(rows, xs[ids])
    r = _kth_D(xs, rows, metric, 40)
    mask = rng.random(N) < 0.6
    for n in (1, 12):
        for mode in ("any", "all"):
            for negate in (False, True):
                for m in (None, mask):
                    want = scoresel_reference(xs, rows[:n], r[:n], metric, mode, negate, m)
                    for tier in _tiers(dtype, n, m):
                        ix.set_range_mode(tier)
                        s = ix.selector_from_range_rows(ids[:n], r[:n], mode=mode, negate=negate, sel=m)
                        t = ix.selector_from_range(rows[:n], r[:n], mode=mode, negate=negate, sel=m)
                        _assert_selector(s, want, f"{tier} rows")
                        np.testing.assert_array_equal(s.bitmap, t.bitmap)
                        s.close()
                        t.close()
    ix.set_range_mode("auto")
    # the row itself passes its own predicate: in, and out under negate
    s = ix.selector_from_range_rows(ids[:1], r[:1])
    assert s.to_mask()[7] and s.count == 39
    s.close()
    s = ix.selector_from_range_rows(ids[:1], r[:1], negate=True)
    assert not s.to_mask()[7] and s.count == N - 39
    s.close()
    s = ix.selector_from_range_rows(np.zeros((0,), dtype=np.int64), np.zeros((0,), dtype=np.float32), mode="all")
    assert s.count == N  # no query: ALL passes everything
    s.close()
    for bad in ([N], [-1], [3, N + 5]):
        with pytest.raises(RuntimeError, match="outside"):
            ix.selector_from_range_rows(bad, 0.0)
    ix.close()


# ---- set operators -----------------------------------------------------------------------------------------
def test_combine(idx):
    rng = np.random.default_rng(33)
    n0, N, d = 1000, 1100, 32  # (1000 rows: a last word of 40 bits; 1100: of 12)
    x = rng.standard_normal((N, d)).astype(np.float32)
    q = rng.standard_normal((2, d)).astype(np.float32)
    ix = idx.FlatIndex(d, "ip", "f32")
    ix.add(x[:n0])
    ma = rng.random(n0) < 0.5
    # a host bitmap whose last byte carries bits past n_sel: they are ignored by every operator
    raw = _bits(ma).copy()
    a = idx.Selector.from_bitmap(ix, raw)
    b0 = ix.selector_from_range(q[:1], _kth_D(x[:n0], q[:1], "ip", 400))
    mb0 = scoresel_reference(x[:n0], q[:1], _kth_D(x[:n0], q[:1], "ip", 400), "ip")
    for s, want in ((a & b0, ma & mb0), (a | b0, ma | mb0), (a - b0, ma & ~mb0), (b0 - a, mb0 & ~ma), (~a, ~ma),
                    (~b0, ~mb0), (~(a | b0), ~(ma | mb0))):
        _assert_selector(s, want)
        s.close()
    ix.add(x[n0:])
    # operands of different n_sel: the result covers the larger, the shorter reads as zero past its end
    r = _kth_D(x, q[1:], "ip", 600)
    b = ix.selector_from_range(q[1:], r)
    mb = scoresel_reference(x, q[1:], r, "ip")
    assert mb[n0:].any()
    pad = np.concatenate([ma, np.zeros(N - n0, dtype=bool)])
    for s, want in ((a & b, pad & mb), (b & a, pad & mb), (a | b, pad | mb), (a - b, pad & ~mb), (b - a, mb & ~pad),
                    (~b, ~mb)):
        _assert_selector(s, want)
        s.close()
    s = ~a  # NOT covers a's rows only
    _assert_selector(s, ~ma)
    # a combined selector is an ordinary selector
    both = a | b
    D, I = ix.search(q, 10, sel=both)
    D2, I2 = ix.search(q, 10, sel=pad | mb)
    np.testing.assert_array_equal(I, I2)
    np.testing.assert_array_equal(D, D2)
    both.close()
    s.close()
    # errors: another index's operand, a closed operand, a non-selector
    other = idx.FlatIndex(d, "ip", "f32")
    other.add(x)
    foreign = other.selector(mb)
    with pytest.raises(RuntimeError, match="another index"):
        a & foreign
    with pytest.raises(RuntimeError, match="another index"):
        foreign | b
    with pytest.raises(TypeError):
        a & [1, 2]
    foreign.close()
    other.close()
    b.close()
    with pytest.raises(RuntimeError, match="closed"):
        a & b
    assert ix.remove_ids([0]) == 1
    with pytest.raises(RuntimeError, match="stale"):
        ~a
    a.close()
    b0.close()
    ix.close()


# ---- composition -------------------------------------------------------------------------------------------
def test_composition(idx):
    rng = np.random.default_rng(35)
    N, d, nq = 3000, 64, 12
    x = rng.standard_normal((N, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    xs = O.round_dtype(x, "bf16")
    ix = idx.FlatIndex(d, "ip", "bf16")
    ix.add(x)
    s = ix.selector_from_range(q[:3], _kth_D(xs, q[:3], "ip", 400), negate=True)  # "not like these"
    host = ix.selector(s.to_mask())  # the same rows through the host road
    assert host.count == s.count and 0 < s.count < N
    D, I = ix.search(q, 10, sel=s)
    D2, I2 = ix.search(q, 10, sel=host)
    np.testing.assert_array_equal(I, I2)
    np.testing.assert_array_equal(D, D2)
    r = _kth_D(xs, q, "ip", 200)
    np.testing.assert_array_equal(ix.range_count(q, r, sel=s)[0], ix.range_count(q, r, sel=host)[0])
    for got, want in zip(ix.range_search(q, r, sel=s), ix.range_search(q, r, sel=host)):
        np.testing.assert_array_equal(got, want)
    ka, kb = ix.kmeans(5, niter=3, seed=7, sel=s), ix.kmeans(5, niter=3, seed=7, sel=host)  # (member ids from the bitmap)
    np.testing.assert_array_equal(ka.labels, kb.labels)
    np.testing.assert_array_equal(ka.centroids, kb.centroids)
    assert ka.labels.shape == (s.count,)
    # a device-built selector as the base of another: "near q3 AND near q4" as a filter
    r34 = _kth_D(xs, q[3:5], "ip", 900)
    first = ix.selector_from_range(q[3:4], r34[:1])
    second = ix.selector_from_range(q[4:5], r34[1:], sel=first)
    _assert_selector(second, scoresel_reference(xs, q[3:5], r34, "ip", "all"))
    for h in (s, host, first, second):
        h.close()
    ix.close()


# ---- errors and empty cases --------------------------------------------------------------------------------
def test_errors_and_empty_inputs(idx):
    from photo_search_engine_amd import _lib
    import ctypes
    d = 48
    rng = np.random.default_rng(23)
    ix = idx.FlatIndex(d, "ip", "f32")
    q = np.ones((3, d), dtype=np.float32)
    s = ix.selector_from_range(q, 0.0)  # an empty index
    assert s.count == 0 and s.bitmap.shape == (0,)
    e = ~s
    assert e.count == 0
    e.close()
    s.close()
    x = rng.standard_normal((200, d)).astype(np.float32)
    ix.add(x)
    none = np.zeros((0, d), dtype=np.float32)
    mask = rng.random(200) < 0.5
    for mode, negate, want in (("any", False, np.zeros(200, dtype=bool)), ("all", False, mask),
                               ("any", True, mask), ("all", True, np.zeros(200, dtype=bool))):
        s = ix.selector_from_range(none, np.zeros((0,), dtype=np.float32), mode=mode, negate=negate, sel=mask)  # nq = 0
        _assert_selector(s, want)
        assert ix.scoresel_last_stats()["tier"] == "none" and ix.scoresel_last_stats()["blocks"] == 0
        s.close()
    with pytest.raises(ValueError):
        ix.selector_from_range(q, np.float32(np.nan))
    L = ix._L  # the C ABI's own checks
    r = np.array([0.0, np.nan, 0.0], dtype=np.float32)
    h = ctypes.c_void_p()
    rc = L.vs_sel_from_range(ix._h, None, q.ctypes.data, 3, r.ctypes.data, 0, 0, ctypes.byref(h))
    assert rc == _lib.VS_ERR_ARG and "NaN" in _lib.last_error() and not h.value
    r[1] = 0.0
    assert L.vs_sel_from_range(ix._h, None, q.ctypes.data, 3, r.ctypes.data, 2, 0, ctypes.byref(h)) == _lib.VS_ERR_ARG
    assert L.vs_sel_from_range(ix._h, None, None, 3, r.ctypes.data, 0, 0, ctypes.byref(h)) == _lib.VS_ERR_ARG
    assert L.vs_sel_from_range(ix._h, None, q.ctypes.data, 3, None, 0, 0, ctypes.byref(h)) == _lib.VS_ERR_ARG
    assert L.vs_sel_from_range(ix._h, None, q.ctypes.data, -1, r.ctypes.data, 0, 0, ctypes.byref(h)) == _lib.VS_ERR_ARG
    assert L.vs_sel_from_range(ix._h, None, q.ctypes.data, 3, r.ctypes.data, 0, 0, None) == _lib.VS_ERR_ARG
    assert L.vs_set_scoresel_staging_bytes(0) == _lib.VS_ERR_ARG
    s = ix.selector_from_range(q, 0.0)
    assert L.vs_sel_combine(ix._h, s._h, None, _lib.SEL_AND, ctypes.byref(h)) == _lib.VS_ERR_ARG
    assert L.vs_sel_combine(ix._h, s._h, s._h, _lib.SEL_NOT, ctypes.byref(h)) == _lib.VS_ERR_ARG
    assert L.vs_sel_combine(ix._h, s._h, s._h, 9, ctypes.byref(h)) == _lib.VS_ERR_ARG
    short = np.zeros((24,), dtype=np.uint8)
    assert L.vs_sel_bitmap(s._h, short.ctypes.data, 24) == _lib.VS_ERR_ARG  # 25 bytes cover 200 rows
    # infinite radii
    for mode in ("any", "all"):
        _check(ix, x, q, np.float32(-np.inf), "ip", mode)
        _check(ix, x, q, np.float32(np.inf), "ip", mode, negate=True)
    s.close()
    with pytest.raises(RuntimeError, match="closed"):
        s.bitmap
    ix.close()


# ---- device memory -----------------------------------------------------------------------------------------
def test_device_memory_is_returned(idx):
    rng = np.random.default_rng(25)
    N, d, nq = 2000, 64, 12
    x = rng.standard_normal((N, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    ix = idx.FlatIndex(d, "ip", "bf16")
    ix.add(x)
    L = ix._L
    base = ix.selector(rng.random(N) < 0.5)
    ids = np.arange(nq, dtype=np.int64)
    try:
        for tier in ("scan", "screen"):
            ix.set_range_mode(tier)
            for mode in ("any", "all"):  # (the context's workspaces grow once)
                ix.selector_from_range(q, 0.0, mode=mode).close()
            ix.selector_from_range_rows(ids, 0.0).close()
            before = int(L.vs_device_bytes_live())
            made = [ix.selector_from_range(q, 0.0, mode="any"), ix.selector_from_range(q, 0.0, mode="all", negate=True),
                    ix.selector_from_range(q, 0.0, mode="all", sel=base), ix.selector_from_range_rows(ids, 0.0)]
            made.append(made[0] | made[1])
            made.append(~made[2])
            for s in made:
                s.bitmap
                s.close()
            assert int(L.vs_device_bytes_live()) == before, tier
    finally:
        ix.set_range_mode("auto")
    base.close()
    ix.close()


# ---- concurrency -------------------------------------------------------------------------------------------
def test_four_threads_on_one_handle(idx):
    rng = np.random.default_rng(27)
    N, d = 6000, 96
    x = rng.standard_normal((N, d)).astype(np.float32)
    xs = O.round_dtype(x, "bf16")
    ix = idx.FlatIndex(d, "ip", "bf16")
    ix.add(x)
    qs = [rng.standard_normal((nq, d)).astype(np.float32) for nq in (2, 24, 2, 24)]  # (scan, screen under AUTO)
    modes = ["any", "any", "all", "all"]
    rads = [_kth_D(xs, qs[t], "ip", 50 if modes[t] == "any" else 5000) for t in range(4)]
    wants = [_bits(scoresel_reference(xs, qs[t], rads[t], "ip", modes[t])) for t in range(4)]
    errors = []

    def work(t):
        try:
            for _ in range(10):
                s = ix.selector_from_range(qs[t], rads[t], mode=modes[t])
                try:
                    np.testing.assert_array_equal(s.bitmap, wants[t])
                finally:
                    s.close()
        except BaseException as exc:  # noqa: BLE001 - reported by the main thread
            errors.append(exc)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    ix.close()
    assert not errors, errors[0]


# ---- multi-device and the product --------------------------------------------------------------------------
def test_multi_device_selector_from_range(idx):
    rng = np.random.default_rng(29)
    N, d, nq = 1200, 64, 3
    x = rng.standard_normal((N, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    mi = idx.MultiDeviceFlatIndex(d, "ip", "f32", devices=[0, 0])
    mi.add(x)
    r = _kth_D(x, q, "ip", 200)
    mask = rng.random(N) < 0.5
    for m in (None, mask, mi.selector(mask)):
        mm = None if m is None else mask
        for mode in ("any", "all"):
            s = mi.selector_from_range(q, r, mode=mode, negate=True, sel=m)
            assert isinstance(s, idx.MaskSelector) and s.n == N
            want = scoresel_reference(x, q, r, "ip", mode, True, mm)
            np.testing.assert_array_equal(s.to_mask(), want)
            D, I = mi.search(q, 5, sel=s)
            D2, I2 = mi.search(q, 5, sel=want)
            np.testing.assert_array_equal(I, I2)
    ids = np.array([3, 700], dtype=np.int64)
    s = mi.selector_from_range_rows(ids, _kth_D(x, x[ids], "ip", 30))
    np.testing.assert_array_equal(s.to_mask(), scoresel_reference(x, x[ids], _kth_D(x, x[ids], "ip", 30), "ip"))
    with pytest.raises(RuntimeError):
        mi.selector_from_range_rows([N], 0.0)
    mi.close()


@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_vector_store_similar_to(tmp_path, monkeypatch, metric):
    from photo_search_engine_amd import vector_store as vsmod
    rng = np.random.default_rng(31)
    n, d = 2000, 64
    X = rng.standard_normal((n, d)).astype(np.float32)
    meta = [{"photo_path": f"/p/{i}.jpg", "year": 2019 + i % 6} for i in range(n)]

    def make(name):
        store = vsmod.VectorStore(dimension=d, index_path=str(tmp_path / f"{name}.idx"),
                                  metadata_path=str(tmp_path / f"{name}.json"), metric=metric, index_type="flat")
        store.add(X, [dict(m) for m in meta])
        return store

    gpu = make("gpu")
    monkeypatch.setattr(vsmod, "_index_factory", oracle_scoresel_factory)
    ref = make("ref")
    ref.index._x = gpu.index.reconstruct_n(0, n)  # (the values as stored)
    qa = rng.standard_normal((d,)).astype(np.float32).tolist()
    qb = rng.standard_normal((d,)).astype(np.float32).tolist()
    threshold = gpu.search(qb, 400)[399]["distance"]
    pred = lambda m: m["year"] != 2020  # noqa: E731
    for negate in (False, True):
        for allowed in (None, pred):
            g = gpu.similar_to(qb, threshold, allowed=allowed, negate=negate)
            w = ref.similar_to(qb, threshold, allowed=allowed, negate=negate)
            np.testing.assert_array_equal(g.to_mask(), w.to_mask())
            assert gpu.search(qa, 20, allowed=g) == ref.search(qa, 20, allowed=w)
            assert gpu.facet_counts(qa, gpu.search(qa, 300)[299]["distance"], "year", allowed=g) == \
                ref.facet_counts(qa, gpu.search(qa, 300)[299]["distance"], "year", allowed=w)
            g.close()
    assert gpu.similar_to(qb, threshold).count == 399
    paths = ["/p/3.jpg", "/p/1777.jpg"]
    t_items = gpu.search_similar(paths[0], 50)[-1]["distance"]
    for mode in ("any", "all"):
        g = gpu.similar_to_items(paths, t_items, negate=True, mode=mode)
        w = ref.similar_to_items(paths, t_items, negate=True, mode=mode)
        np.testing.assert_array_equal(g.to_mask(), w.to_mask())
        clusters = gpu.cluster_items(4, allowed=g, niter=2)  # a selector as `allowed` of a mask-taking method
        assert clusters == gpu.cluster_items(4, allowed=g.to_mask(), niter=2)
        assert sorted(i for c in clusters for i in c["items"]) == np.flatnonzero(g.to_mask()).tolist()
        g.close()

"""Exact facet counts on the GPU (MI355X only): matching rows per group within a radius.

Reference for every case (tests/oracle_facet_index.py ``facet_reference``): ``range_reference`` over the
members -- the covered rows, restricted to the mask -- and one bincount of their ``np.unique`` key codes per
query, the negative keys in the last column.  ``totals`` and ``counts`` must be bit-equal under the scan
tier, the screen tier (where it applies) and the library's own choice, and under each histogram form.
"""
import ctypes
import threading

import numpy as np
import pytest

from oracle import oracle as O
from oracle_facet_index import facet_reference, oracle_facet_factory
from oracle_range_index import range_reference

pytestmark = pytest.mark.gpu

LDS_BINS = 8192  # VS_FACET_LDS_BINS


@pytest.fixture(scope="module")
def idx():
    from photo_search_engine_amd import index
    return index


def _tiers(dtype, nq, sel):
    screen = sel is None and dtype in ("bf16", "f16") and nq >= 9
    return ("scan", "screen", "auto") if screen else ("scan", "auto")


def _check(ix, xs, q, radius, metric, keys=None, groups=None, mask=None, sel=None, tiers=None, ref=None):
    """``range_count`` under every applicable tier x histogram form against the reference; returns
    (totals, counts of the reference, stats per (tier, form))."""
    if ref is None:
        ref = facet_reference(xs, q, radius, metric, keys, None if groups is None else groups.rows, mask)[:2]
    s = sel if sel is not None else mask
    bins = 1 if groups is None else groups.count + 1
    forms = ("auto", "lds", "global") if bins <= LDS_BINS else ("auto", "global")
    stats = {}
    # (no scan runs over an empty member set)
    s_members = (groups is None or groups.rows > 0) and ix.ntotal > 0 and (mask is None or bool(np.asarray(mask).any()))
    try:
        for tier in tiers or _tiers(ix.dtype, q.shape[0], s):
            ix.set_range_mode(tier)
            for form in forms:
                ix.set_facet_hist(form)
                totals, counts = ix.range_count(q, radius, groups=groups, sel=s)
                np.testing.assert_array_equal(totals, ref[0], err_msg=f"totals, {tier} / {form}")
                if groups is None:
                    assert counts is None
                else:
                    np.testing.assert_array_equal(counts, ref[1], err_msg=f"counts, {tier} / {form}")
                st = stats[tier, form] = ix.facet_last_stats()
                assert st["total"] == int(ref[0].sum())
                if tier == "scan":
                    assert st["tier"] == "scan" and st["rescanned"] == 0
                if not s_members:
                    assert st["hist"] == "none"
                elif st["tier"] == "scan" or st["rescanned"]:
                    assert st["hist"] != "none"
                if form != "auto" and st["hist"] != "none":  # (a block too small for the screen scans too)
                    assert st["hist"] == form
    finally:
        ix.set_range_mode("auto")
        ix.set_facet_hist("auto")
    return ref, stats


def _kth_D(xs, q, metric, rank):
    """fp32 D of each query's rank-th best row (1-based)."""
    S, _ = O.knn_exact(xs, q, rank, metric)
    return S[:, rank - 1].astype(np.float32)


def _keys12(n, rng):
    """12 groups with keys far beyond 32 bits, about 5 % of the rows ungrouped."""
    keys = (2 ** 40 + 7 * rng.integers(0, 12, n)).astype(np.int64)
    keys[rng.random(n) < 0.05] = -5
    return keys


# ---- parity ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def parity_corpus():
    rng = np.random.default_rng(3)
    N, d = 3000, 64  # 47 workgroups of the scan, query slices (qy > 1), a last partial wave-step
    x = rng.standard_normal((N, d)).astype(np.float32)
    q = rng.standard_normal((20, d)).astype(np.float32)
    return x, q, _keys12(N, rng)


@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_parity(idx, parity_corpus, dtype, metric):
    x, q, keys = parity_corpus
    xs = O.round_dtype(x, dtype)
    ix = idx.FlatIndex(x.shape[1], metric, dtype)
    ix.add(x)
    groups = ix.group_keys(keys)
    np.testing.assert_array_equal(groups.keys, np.unique(keys[keys >= 0]))
    for nq in (1, 6, 20):  # (20 reaches the screen for bf16 / f16)
        for rank in (10, 500):
            (totals, counts), stats = _check(ix, xs, q[:nq], _kth_D(xs, q[:nq], metric, rank), metric, keys, groups)
            assert totals.tolist() == [rank - 1] * nq and counts.shape == (nq, 13)
            if ("screen", "auto") in stats:
                assert stats["screen", "auto"]["tier"] == "screen"
    groups.close()
    ix.close()


# ---- membership boundary -----------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_membership_boundary(idx, metric):
    rng = np.random.default_rng(5)
    N, d, nq = 2000, 64, 6
    x = rng.standard_normal((N, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    keys = _keys12(N, rng)
    ix = idx.FlatIndex(d, metric, "f32")
    ix.add(x)
    groups = ix.group_keys(keys)
    D10 = _kth_D(x, q, metric, 10)
    S, _ = O.knn_exact(x, q, 10, metric)
    assert (S[:, 8].astype(np.float32) != D10).all()  # (the 9th and the 10th are apart in fp32)
    # the radius is exactly the 10th best row's D: strict, so that row is out and the 9 better are in
    (totals, _), _ = _check(ix, x, q, D10, metric, keys, groups)
    assert totals.tolist() == [9] * nq
    # one fp32 step past it: the row is in
    looser = np.nextafter(D10, np.float32(-np.inf if metric == "ip" else np.inf))
    (totals, _), _ = _check(ix, x, q, looser, metric, keys, groups)
    assert (totals >= 10).all()
    groups.close()
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
    keys = np.arange(40, dtype=np.int64) % 4  # rows 7 and 21 in groups 3 and 1
    ix = idx.FlatIndex(d, "ip", "f32")
    ix.add(x)
    groups = ix.group_keys(keys)
    (totals, counts), _ = _check(ix, x, q, np.float32(1.5), "ip", keys, groups)
    assert totals.tolist() == [0] and not counts.any()
    (totals, counts), _ = _check(ix, x, q, np.nextafter(np.float32(1.5), np.float32(-np.inf)), "ip", keys, groups)
    assert totals.tolist() == [2] and counts[0].tolist() == [0, 1, 0, 1, 0]
    groups.close()
    ix.close()


# ---- infinite radii ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,dtype", [("ip", "bf16"), ("l2", "f32")])
def test_infinite_radii_are_the_group_sizes(idx, metric, dtype):
    rng = np.random.default_rng(7)
    N, d, nq = 1500, 40, 12
    x = rng.standard_normal((N, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    xs = O.round_dtype(x, dtype)
    keys = _keys12(N, rng)
    mask = rng.random(N) < 0.4
    ix = idx.FlatIndex(d, metric, dtype)
    ix.add(x)
    groups = ix.group_keys(keys)
    gkeys = groups.keys
    every = np.float32(-np.inf if metric == "ip" else np.inf)
    for m in (None, mask):
        member = np.ones(N, dtype=bool) if m is None else m
        (totals, counts), _ = _check(ix, xs, q, every, metric, keys, groups, mask=m)
        assert (totals == int(member.sum())).all()
        for g, key in enumerate(gkeys.tolist()):
            assert (counts[:, g] == int(((keys == key) & member).sum())).all()
        assert (counts[:, 12] == int(((keys < 0) & member).sum())).all()
        # the sizes search_groups reports for the groups it returns
        res = ix.search_groups(q, 30, groups, group_size=1, sel=m)
        for i in range(nq):
            for slot in range(30):
                if res.keys[i, slot] >= 0:
                    assert res.sizes[i, slot] == counts[i, int(np.searchsorted(gkeys, res.keys[i, slot]))]
        (totals, counts), _ = _check(ix, xs, q, -every, metric, keys, groups, mask=m)
        assert not totals.any() and not counts.any()
    groups.close()
    ix.close()


# ---- members -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,nq", [("f32", 3), ("bf16", 12)])
def test_members(idx, dtype, nq):
    rng = np.random.default_rng(9)
    N, n_cov, d = 3000, 2500, 64
    x = rng.standard_normal((N, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    xs = O.round_dtype(x, dtype)
    keys = _keys12(n_cov, rng)
    ix = idx.FlatIndex(d, "ip", dtype)
    ix.add(x[:n_cov])
    groups = ix.group_keys(keys)
    ix.add(x[n_cov:])  # rows behind the groups
    r = _kth_D(xs, q, "ip", 300)
    # without a selector (the screen lists rows behind the groups; they are not counted)
    (totals, _), _ = _check(ix, xs, q, r, "ip", keys, groups)
    lims, _, I = range_reference(xs, q, r, "ip")
    assert (totals < np.diff(lims)).all()
    np.testing.assert_array_equal(totals, [int((I[lims[i]:lims[i + 1]] < n_cov).sum()) for i in range(nq)])
    # a selector made after the rows were added allows them; they are no members all the same
    everything = np.ones(N, dtype=bool)
    (with_sel, _), _ = _check(ix, xs, q, r, "ip", keys, groups, mask=everything)
    np.testing.assert_array_equal(with_sel, totals)
    some = rng.random(N) < 0.3
    _check(ix, xs, q, r, "ip", keys, groups, mask=some)
    # a selector allowing nothing
    (totals, counts), _ = _check(ix, xs, q, r, "ip", keys, groups, mask=np.zeros(N, dtype=bool))
    assert not totals.any() and not counts.any()
    # no groups: every stored row, np.diff(lims) of range_search
    for m in (None, some):
        lims, _, _ = ix.range_search(q, r, sel=m)
        (totals, counts), _ = _check(ix, xs, q, r, "ip", mask=m)
        assert counts is None
        np.testing.assert_array_equal(totals, np.diff(lims))
    groups.close()
    ix.close()


# ---- histogram forms ---------------------------------------------------------------------------------------
def test_lds_form_at_the_full_bin_count(idx):
    rng = np.random.default_rng(11)
    N, d, nq = 9000, 32, 4
    x = rng.standard_normal((N, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    keys = (np.arange(N, dtype=np.int64) * 3) % (LDS_BINS - 1)  # every one of 8191 keys, then ungrouped rows
    keys[-50:] = -1
    ix = idx.FlatIndex(d, "l2", "f32")
    ix.add(x)
    groups = ix.group_keys(keys)
    assert groups.count + 1 == LDS_BINS
    _, stats = _check(ix, x, q, _kth_D(x, q, "l2", 3000), "l2", keys, groups)
    assert stats["auto", "auto"]["hist"] == "lds"
    groups.close()
    ix.close()


def test_global_form_past_the_lds_bins(idx):
    rng = np.random.default_rng(13)
    N, d, nq = 10000, 32, 4
    x = rng.standard_normal((N, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    keys = rng.permutation(N).astype(np.int64) * 5  # all distinct: G + 1 > VS_FACET_LDS_BINS
    ix = idx.FlatIndex(d, "ip", "f32")
    ix.add(x)
    groups = ix.group_keys(keys)
    r = _kth_D(x, q, "ip", 2000)
    (totals, counts), stats = _check(ix, x, q, r, "ip", keys, groups)
    assert counts.max() == 1 and stats["auto", "auto"]["hist"] == "global"
    ix.set_facet_hist("lds")
    try:
        with pytest.raises(RuntimeError, match="bins"):
            ix.range_count(q, r, groups=groups)
    finally:
        ix.set_facet_hist("auto")
    groups.close()
    ix.close()


@pytest.mark.parametrize("dtype,nq", [("f32", 5), ("bf16", 16)])
def test_every_row_in_one_group(idx, dtype, nq):
    """Maximal contention on one bin, under both forms and both tiers."""
    rng = np.random.default_rng(15)
    N, d = 5000, 48
    x = rng.standard_normal((N, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    xs = O.round_dtype(x, dtype)
    keys = np.full(N, 77, dtype=np.int64)
    ix = idx.FlatIndex(d, "ip", dtype)
    ix.add(x)
    groups = ix.group_keys(keys)
    (totals, counts), _ = _check(ix, xs, q, np.float32(-np.inf), "ip", keys, groups)
    assert counts.tolist() == [[N, 0]] * nq
    _check(ix, xs, q, _kth_D(xs, q, "ip", 2500), "ip", keys, groups)
    groups.close()
    ix.close()


def test_query_outside_lds(idx):
    """d = 6400: the fp64 query (50 KiB) is not staged in LDS (the QLDS = false instantiations); the LDS
    form's bins then start the workgroup's LDS."""
    rng = np.random.default_rng(17)
    N, d, nq = 300, 6400, 2
    x = rng.standard_normal((N, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    keys = _keys12(N, rng)
    for dtype, metric in (("f32", "ip"), ("bf16", "l2")):
        xs = O.round_dtype(x, dtype)
        ix = idx.FlatIndex(d, metric, dtype)
        ix.add(x)
        groups = ix.group_keys(keys)
        _check(ix, xs, q, _kth_D(xs, q, metric, 100), metric, keys, groups)
        groups.close()
        ix.close()


# ---- the screen tier ---------------------------------------------------------------------------------------
def test_screen_overflow_goes_to_the_scan(idx):
    """The construction of test_gpu_range.py: 4,000 copies of one vector stored contiguously and a radius
    just below their score, so a workgroup of the screen compacts its list.  The scan answers the query
    and the refine leaves it alone: no row counted twice, none lost."""
    rng = np.random.default_rng(19)
    N, d, nq = 300000, 64, 9
    x = rng.standard_normal((N, d)).astype(np.float32)
    v = x[100000].copy()
    x[100000:104000] = v
    xs = O.round_dtype(x, "bf16")
    q = (v[None, :] * (1.0 + 0.01 * np.arange(nq))[:, None] + 0.01 * rng.standard_normal((nq, d))).astype(np.float32)
    score = O.canon_scores(xs[100000:100001], q, "ip")[:, 0].astype(np.float32)
    keys = _keys12(N, rng)
    ix = idx.FlatIndex(d, "ip", "bf16")
    ix.add(x)
    groups = ix.group_keys(keys)
    (totals, _), stats = _check(ix, xs, q, np.nextafter(score, np.float32(-np.inf)), "ip", keys, groups)
    assert (totals >= 4000).all()
    for form in ("auto", "lds", "global"):
        for tier in ("screen", "auto"):
            assert stats[tier, form]["tier"] == "screen" and stats[tier, form]["rescanned"] >= 1, (tier, form)
    groups.close()
    ix.close()


def test_screen_overflow_of_some_queries_of_a_block(idx):
    """The construction above with 9 random queries in the same block, each with the radius of its 40th
    best row: their lists are complete and the refine counts them, while the scan counts the 9 whose
    list a workgroup cut -- one block, both tiers, every query through exactly one of them.  The commit
    before the shared tier driver reported 9 re-answered queries under every tier and form, hence `== 9`."""
    rng = np.random.default_rng(19)
    N, d, nq = 300000, 64, 9
    x = rng.standard_normal((N, d)).astype(np.float32)
    v = x[100000].copy()
    x[100000:104000] = v
    xs = O.round_dtype(x, "bf16")
    q = (v[None, :] * (1.0 + 0.01 * np.arange(nq))[:, None] + 0.01 * rng.standard_normal((nq, d))).astype(np.float32)
    score = O.canon_scores(xs[100000:100001], q, "ip")[:, 0].astype(np.float32)
    keys = _keys12(N, rng)
    q2 = rng.standard_normal((nq, d)).astype(np.float32)
    q = np.concatenate([q, q2])
    radius = np.concatenate([np.nextafter(score, np.float32(-np.inf)), _kth_D(xs, q2, "ip", 40)])
    ix = idx.FlatIndex(d, "ip", "bf16")
    ix.add(x)
    groups = ix.group_keys(keys)
    (totals, _), stats = _check(ix, xs, q, radius, "ip", keys, groups)
    assert (totals[:nq] >= 4000).all() and totals[nq:].tolist() == [39] * nq
    for form in ("auto", "lds", "global"):
        for tier in ("screen", "auto"):
            assert stats[tier, form]["tier"] == "screen" and stats[tier, form]["rescanned"] == 9, (tier, form)
    groups.close()
    ix.close()


# ---- query blocks ------------------------------------------------------------------------------------------
def test_query_blocks(idx):
    rng = np.random.default_rng(21)
    N, d = 2000, 64
    x = rng.standard_normal((N, d)).astype(np.float32)
    q = rng.standard_normal((300, d)).astype(np.float32)
    xs = O.round_dtype(x, "bf16")
    keys = _keys12(N, rng)
    ix = idx.FlatIndex(d, "ip", "bf16")
    ix.add(x)
    groups = ix.group_keys(keys)
    r = _kth_D(xs, q, "ip", 60)
    ref, stats = _check(ix, xs, q, r, "ip", keys, groups)  # 256 + 44 queries
    assert all(st["blocks"] == 2 for st in stats.values())
    assert stats["auto", "auto"]["tier"] == "screen"
    try:
        idx.set_facet_staging_bytes(1)  # below one query's row of counters: one query per block
        ref20 = (ref[0][:20], ref[1][:20])
        _, stats = _check(ix, xs, q[:20], r[:20], "ip", keys, groups, ref=ref20)
        assert all(st["blocks"] == 20 and st["tier"] == "scan" for st in stats.values())
        # 8 (G + 1) * 12 bytes: 12 queries per block, enough for the screen
        idx.set_facet_staging_bytes(8 * 13 * 12)
        _, stats = _check(ix, xs, q[:20], r[:20], "ip", keys, groups, ref=ref20)
        assert all(st["blocks"] == 2 for st in stats.values())
    finally:
        idx.set_facet_staging_bytes()
    groups.close()
    ix.close()


# ---- errors and empty cases --------------------------------------------------------------------------------
def test_errors_and_empty_inputs(idx):
    from photo_search_engine_amd import _lib
    d = 48
    rng = np.random.default_rng(23)
    ix = idx.FlatIndex(d, "ip", "f32")
    q = np.ones((3, d), dtype=np.float32)
    totals, counts = ix.range_count(q, 0.0)  # an empty index
    assert totals.tolist() == [0, 0, 0] and counts is None
    empty_groups = ix.group_keys(np.zeros((0,), dtype=np.int64))
    totals, counts = ix.range_count(q, 0.0, groups=empty_groups)
    assert totals.tolist() == [0, 0, 0] and counts.shape == (3, 1) and not counts.any()
    assert empty_groups.keys.shape == (0,)
    x = rng.standard_normal((200, d)).astype(np.float32)
    ix.add(x)
    totals, counts = ix.range_count(q, -1e30, groups=empty_groups)  # groups that cover none of the rows
    assert totals.tolist() == [0, 0, 0] and not counts.any()
    empty_groups.close()
    keys = np.arange(200, dtype=np.int64) % 7
    groups = ix.group_keys(keys)
    totals, counts = ix.range_count(np.zeros((0, d), dtype=np.float32), 0.0, groups=groups)  # nq = 0
    assert totals.shape == (0,) and counts.shape == (0, 8)
    with pytest.raises(ValueError):
        ix.range_count(q, np.float32(np.nan), groups=groups)
    L = ix._L  # the C ABI's own checks
    r = np.array([0.0, np.nan, 0.0], dtype=np.float32)
    c = np.zeros((3, 8), dtype=np.int64)
    t = np.zeros((3,), dtype=np.int64)
    rc = L.vs_range_count(ix._h, groups._h, None, q.ctypes.data, 3, r.ctypes.data, c.ctypes.data, t.ctypes.data)
    assert rc == _lib.VS_ERR_ARG and "NaN" in _lib.last_error()
    r[1] = 0.0
    assert L.vs_range_count(ix._h, groups._h, None, q.ctypes.data, 3, r.ctypes.data, None, t.ctypes.data) == _lib.VS_ERR_ARG
    assert L.vs_range_count(ix._h, None, None, q.ctypes.data, 3, r.ctypes.data, None, None) == _lib.VS_ERR_ARG
    assert L.vs_range_count(ix._h, None, None, q.ctypes.data, 3, r.ctypes.data, c.ctypes.data, t.ctypes.data) == _lib.VS_ERR_ARG
    assert L.vs_range_count(ix._h, groups._h, None, None, 3, r.ctypes.data, c.ctypes.data, t.ctypes.data) == _lib.VS_ERR_ARG
    assert L.vs_range_count(ix._h, groups._h, None, q.ctypes.data, 3, None, c.ctypes.data, t.ctypes.data) == _lib.VS_ERR_ARG
    assert L.vs_range_count(ix._h, groups._h, None, q.ctypes.data, 3, r.ctypes.data, c.ctypes.data, None) == 0  # totals may be null
    np.testing.assert_array_equal(c, facet_reference(x, q, r, "ip", keys)[1])
    # groups of another index
    other = idx.FlatIndex(d, "ip", "f32")
    other.add(x)
    with pytest.raises(RuntimeError, match="another index"):
        other.range_count(q, 0.0, groups=groups)
    other.close()
    # a stale selector, stale groups
    sel = ix.selector(np.ones(200, dtype=bool))
    assert ix.remove_ids([5]) == 1
    with pytest.raises(RuntimeError, match="stale"):
        ix.range_count(q, 0.0, groups=groups)
    with pytest.raises(RuntimeError, match="stale"):
        ix.range_count(q, 0.0, sel=sel)
    sel.close()
    groups.close()
    with pytest.raises(RuntimeError, match="closed"):
        ix.range_count(q, 0.0, groups=groups)
    with pytest.raises(ValueError):
        ix.set_facet_hist("shared")
    ix.close()


# ---- device memory -----------------------------------------------------------------------------------------
def test_device_memory_is_returned(idx):
    rng = np.random.default_rng(25)
    N, d, nq = 2000, 64, 12
    x = rng.standard_normal((N, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    keys = _keys12(N, rng)
    ix = idx.FlatIndex(d, "ip", "bf16")
    ix.add(x)
    groups = ix.group_keys(keys)
    L = ix._L
    try:
        for tier in ("scan", "screen"):
            ix.set_range_mode(tier)
            ix.range_count(q, 0.0, groups=groups)  # (the context's workspaces grow once)
            before = int(L.vs_device_bytes_live())
            ix.range_count(q, 0.0, groups=groups)
            ix.range_count(q, 0.0)
            assert int(L.vs_device_bytes_live()) == before, tier
    finally:
        ix.set_range_mode("auto")
    groups.close()
    ix.close()


# ---- concurrency -------------------------------------------------------------------------------------------
def test_four_threads_on_one_handle(idx):
    rng = np.random.default_rng(27)
    N, d = 6000, 96
    x = rng.standard_normal((N, d)).astype(np.float32)
    xs = O.round_dtype(x, "bf16")
    keys = _keys12(N, rng)
    ix = idx.FlatIndex(d, "ip", "bf16")
    ix.add(x)
    groups = ix.group_keys(keys)
    qs = [rng.standard_normal((nq, d)).astype(np.float32) for nq in (2, 24, 2, 24)]  # (scan, screen under AUTO)
    rads = [_kth_D(xs, qv, "ip", 50) for qv in qs]
    serial = [ix.range_count(qs[t], rads[t], groups=groups) for t in range(4)]
    for t in range(4):
        ref = facet_reference(xs, qs[t], rads[t], "ip", keys)
        np.testing.assert_array_equal(serial[t][0], ref[0])
        np.testing.assert_array_equal(serial[t][1], ref[1])
    errors = []

    def work(t):
        try:
            for _ in range(10):
                totals, counts = ix.range_count(qs[t], rads[t], groups=groups)
                np.testing.assert_array_equal(totals, serial[t][0])
                np.testing.assert_array_equal(counts, serial[t][1])
        except BaseException as exc:  # noqa: BLE001 - reported by the main thread
            errors.append(exc)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    groups.close()
    ix.close()
    assert not errors, errors[0]


# ---- multi-device and the product --------------------------------------------------------------------------
def test_multi_device_range_count(idx):
    rng = np.random.default_rng(29)
    N, n_cov, d, nq = 1200, 1000, 64, 3
    x = rng.standard_normal((N, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    keys = _keys12(n_cov, rng)
    mi = idx.MultiDeviceFlatIndex(d, "ip", "f32", devices=[0, 0])
    mi.add(x[:n_cov])
    groups = mi.group_keys(keys)
    mi.add(x[n_cov:])
    r = _kth_D(x, q, "ip", 200)
    mask = rng.random(N) < 0.5
    for m in (None, mask):
        want = facet_reference(x, q, r, "ip", keys, n_cov, m)
        totals, counts = mi.range_count(q, r, groups=groups, sel=m)
        np.testing.assert_array_equal(totals, want[0])
        np.testing.assert_array_equal(counts, want[1])
        totals, counts = mi.range_count(q, r, sel=m)
        assert counts is None
        np.testing.assert_array_equal(totals, facet_reference(x, q, r, "ip", mask=m)[0])
    groups.close()
    mi.close()


@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_vector_store_facet_counts(tmp_path, monkeypatch, metric):
    from photo_search_engine_amd import vector_store as vsmod
    rng = np.random.default_rng(31)
    n, d = 2000, 64
    X = rng.standard_normal((n, d)).astype(np.float32)
    meta = [{"photo_path": f"/p/{i}.jpg", "year": 2019 + i % 6, **({} if i % 9 == 0 else {"camera": f"cam-{i % 5}"})}
            for i in range(n)]

    def make(name):
        store = vsmod.VectorStore(dimension=d, index_path=str(tmp_path / f"{name}.idx"),
                                  metadata_path=str(tmp_path / f"{name}.json"), metric=metric, index_type="flat")
        store.add(X, [dict(m) for m in meta])
        return store

    gpu = make("gpu")
    monkeypatch.setattr(vsmod, "_index_factory", oracle_facet_factory)
    ref = make("ref")
    ref.index._x = gpu.index.reconstruct_n(0, n)  # (the values as stored)
    qv = rng.standard_normal((d,)).astype(np.float32).tolist()
    ranked = gpu.search(qv, 400)
    pred = lambda m: m["year"] != 2020  # noqa: E731
    for threshold in (ranked[25]["distance"], ranked[399]["distance"]):
        assert gpu.count_matches(qv, threshold) == ref.count_matches(qv, threshold) == len(gpu.search_range(qv, threshold))
        assert gpu.count_matches(qv, threshold, allowed=pred) == ref.count_matches(qv, threshold, allowed=pred)
        for by in ("camera", "year", lambda m: m["year"] % 2 or None, [i % 11 - 1 for i in range(n)]):
            got = gpu.facet_counts(qv, threshold, by)
            assert got == ref.facet_counts(qv, threshold, by) and got["total"] > 0
            assert list(got["counts"].items()) == list(ref.facet_counts(qv, threshold, by)["counts"].items())
            assert gpu.facet_counts(qv, threshold, by, allowed=pred) == ref.facet_counts(qv, threshold, by, allowed=pred)
    got = gpu.facet_counts(qv, ranked[399]["distance"], "camera")
    assert got["total"] == 399 and got["ungrouped"] > 0 and sum(got["counts"].values()) + got["ungrouped"] == 399

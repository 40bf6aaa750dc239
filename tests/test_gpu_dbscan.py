"""Exact density clusters on the GPU (MI355X only): neighbour counts and DBSCAN over the stored rows.

Reference for every case (tests/oracle_dbscan_index.py): the pair list of ``rows_range_reference(...,
self_mode="above")`` over the members, the bincount of its ends, the components of its core - core pairs and
the best core neighbour of every other member.  Labels, kinds, degrees, counts and ``n_edges`` must be
bit-equal under the scan tier, the screen tier (where it applies) and the library's own choice.
"""
import ctypes
import threading

import numpy as np
import pytest

from oracle import oracle as O
from oracle_dbscan_index import (BORDER, CORE, NOISE, NONE, dbscan_pairs, dbscan_reference, degrees_of_pairs,
                                 oracle_dbscan_factory)

pytestmark = pytest.mark.gpu

COS = 0.95  # a chain's step: cos(theta); rows are near iff their angle is below arccos(0.9) = 1.42 theta
THETA = np.arccos(COS)
RADIUS = {"ip": np.float32(0.9), "l2": np.float32(0.2)}  # (unit rows: squared L2 = 2 - 2 cos)


@pytest.fixture(scope="module")
def idx():
    from photo_search_engine_amd import index
    return index


def _tiers(dtype, members, sel):
    screen = sel is None and dtype in ("bf16", "f16") and members >= 9
    return ("scan", "screen", "auto") if screen else ("scan", "auto")


def _skipped(pairs):
    """Members without a neighbour above: the queries pass 2 leaves out."""
    member, first, _, _ = pairs
    return int(member.sum()) - int(np.unique(first).shape[0])


def _check(ix, ref, radius, min_samples, sel=None, members=None, tiers=None, skipped=None):
    """``range_dbscan`` and ``range_degrees`` under every applicable tier against ``ref`` = (labels, kinds,
    degrees, counts); returns the stats of the ``range_dbscan`` call per tier."""
    members = ix.ntotal if members is None else members
    stats = {}
    try:
        for tier in tiers or _tiers(ix.dtype, members, sel):
            ix.set_range_mode(tier)
            deg, ne = ix.range_degrees(radius, sel=sel)
            assert deg.dtype == np.int64 and deg.shape == (ix.ntotal,)
            np.testing.assert_array_equal(deg, ref[2], err_msg=f"range_degrees, {tier}")
            assert ne == ref[3]["edges"] and int(deg[deg >= 0].sum()) == 2 * ne, tier
            st = ix.dbscan_last_stats()
            assert (st["members"], st["edges"], st["clusters"], st["blocks2"]) == (members, ne, 0, 0), tier
            labels, kinds, degrees, counts = ix.range_dbscan(radius, min_samples, sel=sel)
            assert labels.dtype == np.int64 and labels.shape == (ix.ntotal,)
            assert kinds.dtype == np.uint8 and kinds.shape == (ix.ntotal,)
            np.testing.assert_array_equal(degrees, ref[2], err_msg=f"degrees, {tier}")
            np.testing.assert_array_equal(kinds, ref[1], err_msg=f"kinds, {tier}")
            np.testing.assert_array_equal(labels, ref[0], err_msg=f"labels, {tier}")
            assert counts == ref[3], tier
            st = stats[tier] = ix.dbscan_last_stats()
            assert {k: st[k] for k in ("clusters", "core", "border", "noise", "edges")} == counts, tier
            assert st["members"] == members and st["blocks"] == (members + 255) // 256, tier
            assert st["blocks2"] <= st["blocks"] and st["skipped"] <= members, tier
            if skipped is not None:
                assert st["skipped"] == skipped, tier
            if tier == "scan":
                assert st["tier"] == "scan" and st["rescanned"] == 0 and st["rescanned2"] == 0
            if tier == "screen":
                assert st["tier"] == "screen"
    finally:
        ix.set_range_mode("auto")
    return stats


def _unit(x):
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def _plane_rows(rng, d, angles):
    """Unit rows at the given multiples of theta in a random plane."""
    u, v = np.linalg.qr(rng.standard_normal((d, 2)))[0].T
    return np.stack([np.cos(a * THETA) * u + np.sin(a * THETA) * v for a in angles]).astype(np.float32)


def _tie_rows(d):
    """x = e0, a = (c, s), b = (c, -s), then four copies at 1.9 theta beside a and beside b: 11 rows in the plane
    of the first two axes.  <x, a> = <x, b> = c and |x - a|^2 = |x - b|^2 bit for bit, in every dtype."""
    rows = np.zeros((11, d), dtype=np.float32)
    rows[0, 0] = 1.0
    rows[1, :2] = (np.cos(THETA), np.sin(THETA))
    rows[2, :2] = (np.cos(THETA), -np.sin(THETA))
    rows[3:7, :2] = (np.cos(1.9 * THETA), np.sin(1.9 * THETA))
    rows[7:11, :2] = (np.cos(1.9 * THETA), -np.sin(1.9 * THETA))
    return rows


# ---- parity ------------------------------------------------------------------------------------------------
CHAIN = (10, 1500, 2300, 700, 2990)          # angles 0 .. 4 theta: degrees 1, 2, 2, 2, 1
SPAN = (6, 300, 301, 2900, 2901, 1200)       # one dense group, its rows in query blocks 0, 1, 4 and 11
BR_A, BR_A0, BR_X, BR_B0, BR_B = (400, 401, 402, 403, 404), 2500, 1000, 50, (2600, 2601, 2602, 2603, 2604)
TIE_X, TIE_A, TIE_B, TIE_AC, TIE_BC = 5, 2100, 900, (2101, 2102, 2103, 2104), (901, 902, 903, 904)
MIN_SAMPLES = (1, 3, 6)


@pytest.fixture(scope="module")
def parity_corpus():
    rng = np.random.default_rng(61)
    N, d = 3000, 64  # 12 query blocks, 47 workgroups of the scan, query slices, a last partial wave-step
    x = _unit(rng.standard_normal((N, d)))
    planted = CHAIN + SPAN + BR_A + (BR_A0, BR_X, BR_B0) + BR_B + (TIE_X, TIE_A, TIE_B) + TIE_AC + TIE_BC
    assert len(set(planted)) == len(planted)
    free = np.setdiff1d(np.arange(N), np.array(planted))
    rng.shuffle(free)
    pos = 0
    # groups of noisy copies, scattered over the blocks: tight ones (cliques), then loose ones (two copies meet
    # at cos = 1 / (1 + 64 noise^2) = 0.88 or 0.86 on average, so a minority of a group's pairs pass: core,
    # border and noise rows in one group)
    loose = [(12, 0.046), (20, 0.05), (30, 0.05), (30, 0.046)]
    for size, noise in [(s, 0.02) for s in (2, 3, 5, 8, 13, 21, 40, 2, 2, 4, 7, 30)] + loose:
        ids = free[pos:pos + size]
        pos += size
        x[ids] = _unit(x[ids[0]] + noise * rng.standard_normal((size, d)))
    x[list(CHAIN)] = _plane_rows(rng, d, [0, 1, 2, 3, 4])
    x[list(SPAN)] = _unit(x[SPAN[0]] + 0.02 * rng.standard_normal((len(SPAN), d)))
    # two dense groups and a row near one row of each (test_dbscan_host.py has the angles' reasoning)
    x[list(BR_A) + [BR_A0, BR_X, BR_B0] + list(BR_B)] = _plane_rows(rng, d, [-0.9] * 5 + [0, 0.95, 2] + [2.9] * 5)
    x[[TIE_X, TIE_A, TIE_B] + list(TIE_AC) + list(TIE_BC)] = _tie_rows(d)
    x.setflags(write=False)
    return x


_parity_pairs = {}


def _parity_ref(x, dtype, metric, min_samples):
    if (dtype, metric) not in _parity_pairs:
        _parity_pairs[dtype, metric] = dbscan_pairs(O.round_dtype(x, dtype), RADIUS[metric], metric)
    pairs = _parity_pairs[dtype, metric]
    return pairs, dbscan_reference(None, RADIUS[metric], metric, min_samples, pairs=pairs)


def _assert_planted(xs, metric, min_samples, ref):
    """The planted features are in the reference."""
    labels, kinds, degrees, counts = ref
    assert degrees[list(CHAIN)].tolist() == [1, 2, 2, 2, 1]
    assert len({i // 256 for i in SPAN}) >= 3 and (degrees[list(SPAN)] == len(SPAN) - 1).all()
    assert degrees[[BR_A0, BR_X, BR_B0]].tolist() == [6, 2, 6] and (degrees[list(BR_A + BR_B)] == 5).all()
    assert degrees[[TIE_X, TIE_A, TIE_B]].tolist() == [2, 5, 5] and (degrees[list(TIE_AC + TIE_BC)] == 4).all()
    S = O.canon_scores(xs[[TIE_A, TIE_B]], xs[[TIE_X]], metric)
    assert np.float32(S[0, 0]) == np.float32(S[0, 1])
    assert degrees.max() == 39 and counts["edges"] > 1500
    assert (kinds[list(SPAN)] == CORE).all() and (labels[list(SPAN)] == SPAN[0]).all()
    if min_samples == 1:
        assert (kinds == CORE).all() and counts["border"] == counts["noise"] == 0
    if min_samples == 3:
        # the chain: a border row below its one core neighbour, one above its own
        assert kinds[list(CHAIN)].tolist() == [BORDER, CORE, CORE, CORE, BORDER]
        assert (labels[list(CHAIN)] == 700).all() and CHAIN[0] < CHAIN[1] and CHAIN[4] > CHAIN[3]
        # the row between the two dense groups is core: they are one cluster
        assert kinds[BR_X] == CORE and labels[BR_A0] == labels[BR_B0] == BR_B0
        assert kinds[TIE_X] == CORE and labels[TIE_A] == labels[TIE_B] == TIE_X
    if min_samples == 6:
        assert (kinds[list(CHAIN)] == NOISE).all()
        # the non-core bridge joins nothing and goes with its better-scoring core neighbour, the higher id
        assert kinds[BR_X] == BORDER and (kinds[list(BR_A + BR_B) + [BR_A0, BR_B0]] == CORE).all()
        assert labels[BR_A0] == BR_A[0] and labels[BR_B0] == BR_B0 and labels[BR_X] == BR_A[0]
        # the exact tie goes to the lower core id; the copies are border rows of their own side
        assert kinds[[TIE_X, TIE_A, TIE_B]].tolist() == [BORDER, CORE, CORE] and TIE_B < TIE_A
        assert labels[TIE_X] == TIE_B and (labels[list(TIE_AC)] == TIE_A).all() and (labels[list(TIE_BC)] == TIE_B).all()
        assert (kinds[list(TIE_AC + TIE_BC)] == BORDER).all()
    if min_samples > 1:
        assert counts["border"] >= 5 and counts["noise"] > 2000 and counts["clusters"] >= 8
        assert counts["core"] + counts["border"] + counts["noise"] == xs.shape[0]


@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_parity(idx, parity_corpus, dtype, metric):
    x = parity_corpus
    xs = O.round_dtype(x, dtype)
    ix = idx.FlatIndex(x.shape[1], metric, dtype)
    ix.add(x)
    for ms in MIN_SAMPLES:
        pairs, ref = _parity_ref(x, dtype, metric, ms)
        _assert_planted(xs, metric, ms, ref)
        stats = _check(ix, ref, RADIUS[metric], ms, skipped=_skipped(pairs))
        assert stats["scan"]["blocks"] == 12
    ix.close()


# ---- contention --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_every_row_identical(idx, dtype):
    N, d = 2000, 32
    x = np.tile(_unit(np.random.default_rng(45).standard_normal((1, d))), (N, 1))
    deg = np.full((N,), N - 1, dtype=np.int64)
    ne = N * (N - 1) // 2
    ix = idx.FlatIndex(d, "ip", dtype)
    ix.add(x)
    one = (np.zeros((N,), dtype=np.int64), np.full((N,), CORE, dtype=np.uint8), deg,
           {"clusters": 1, "core": N, "border": 0, "noise": 0, "edges": ne})
    stats = _check(ix, one, np.float32(0.5), N, skipped=1)
    assert ("screen" in stats) == (dtype == "bf16")
    none = (np.full((N,), -1, dtype=np.int64), np.full((N,), NOISE, dtype=np.uint8), deg,
            {"clusters": 0, "core": 0, "border": 0, "noise": N, "edges": ne})
    _check(ix, none, np.float32(0.5), N + 1, skipped=1)
    ix.close()


def test_exactly_once_under_the_screens_rescan(idx):
    """The construction of test_gpu_range.py: 4,000 copies of one vector stored contiguously, so a workgroup of
    the screen compacts the lists of the queries that are those copies.  Those queries are counted by the scan
    and by the scan alone: a degree of 3999, not more.  Random unit rows at d = 64 are nowhere near 0.95 of
    each other, so the answer is known without a join."""
    rng = np.random.default_rng(57)
    N, d, c0, nc = 300000, 64, 100000, 4000
    x = _unit(rng.standard_normal((N, d)))
    x[c0:c0 + nc] = x[c0]
    labels = np.full((N,), -1, dtype=np.int64)
    labels[c0:c0 + nc] = c0
    kinds = np.full((N,), NOISE, dtype=np.uint8)
    kinds[c0:c0 + nc] = CORE
    deg = np.zeros((N,), dtype=np.int64)
    deg[c0:c0 + nc] = nc - 1
    counts = {"clusters": 1, "core": nc, "border": 0, "noise": N - nc, "edges": nc * (nc - 1) // 2}
    ix = idx.FlatIndex(d, "ip", "bf16")
    ix.add(x)
    try:
        ix.set_range_mode("screen")  # (the scan of 1172 blocks takes seconds)
        got = ix.range_dbscan(np.float32(0.95), nc)
        st = ix.dbscan_last_stats()
    finally:
        ix.set_range_mode("auto")
    np.testing.assert_array_equal(got[2], deg)
    np.testing.assert_array_equal(got[1], kinds)
    np.testing.assert_array_equal(got[0], labels)
    assert got[3] == counts
    assert st["tier"] == "screen" and st["rescanned"] >= 1 and st["skipped"] == N - nc + 1
    assert st["blocks"] == (N + 255) // 256 and st["blocks2"] == len({i // 256 for i in range(c0, c0 + nc - 1)})
    ix.close()


# ---- pass-2 skipping ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_pass_two_skips_queries_without_an_edge_above(idx, dtype):
    """Ten triples of copies in 2000 random rows: the two lower rows of a triple have a neighbour above, nobody
    else has.  Pass 2 answers those 20 queries, in the blocks that hold them, and skips 1980."""
    rng = np.random.default_rng(63)
    N, d = 2000, 32
    x = _unit(rng.standard_normal((N, d)))
    triples = rng.choice(N, 30, replace=False).reshape(10, 3)
    for t in triples:
        x[t] = x[t[0]]
    xs = O.round_dtype(x, dtype)
    pairs = dbscan_pairs(xs, RADIUS["ip"], "ip")
    assert pairs[1].shape[0] == 30  # (no pair but the triples')
    lower = np.sort(triples, axis=1)[:, :2].reshape(-1)
    assert sorted(set(pairs[1].tolist())) == sorted(lower.tolist())
    ix = idx.FlatIndex(d, "ip", dtype)
    ix.add(x)
    for ms in (2, 3, 4):
        ref = dbscan_reference(xs, RADIUS["ip"], "ip", ms, pairs=pairs)
        assert ref[3]["clusters"] == (10 if ms <= 3 else 0) and ref[3]["noise"] == (N - 30 if ms <= 3 else N)
        stats = _check(ix, ref, RADIUS["ip"], ms, skipped=N - 20)
        for st in stats.values():
            assert st["blocks2"] == len({int(i) // 256 for i in lower}) and st["blocks"] == 8
    ix.close()


# ---- selector ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_selector_members(idx, dtype):
    rng = np.random.default_rng(47)
    N, extra, d = 1000, 40, 32
    x = _unit(rng.standard_normal((N + extra, d)))
    for g in range(20):  # groups of copies, about a third of their rows disallowed below
        ids = rng.choice(N, 6, replace=False)
        x[ids] = _unit(x[ids[0]] + 0.02 * rng.standard_normal((6, d)))
    chain = (100, 400, 800, 900, 950)
    x[list(chain)] = _plane_rows(rng, d, [0, 1, 2, 3, 4])
    x[N:N + 5] = x[3]  # copies of an allowed row, added after the selector was made
    mask = rng.random(N) < 0.7
    mask[[100, 400, 900, 950, 3]] = True
    mask[800] = False  # the chain's middle, core when it is a member
    xs = O.round_dtype(x, dtype)
    ix = idx.FlatIndex(d, "ip", dtype)
    ix.add(x[:N])
    sel = ix.selector(mask)
    ix.add(x[N:])
    pairs = dbscan_pairs(xs, RADIUS["ip"], "ip", mask)  # (a mask over the first N rows only)
    ref = dbscan_reference(xs, RADIUS["ip"], "ip", 3, pairs=pairs)
    labels, kinds, degrees, counts = ref
    assert (kinds[N:] == NONE).all() and (degrees[N:] == -1).all() and (labels[N:] == -1).all()
    assert (kinds[:N][~mask] == NONE).all() and (kinds[:N][mask] != NONE).all()
    # without its middle the chain is two pairs: nobody core, nobody attached
    assert degrees[list(chain)].tolist() == [1, 1, -1, 1, 1] and (kinds[[100, 400, 900, 950]] == NOISE).all()
    assert counts["clusters"] >= 5
    full_pairs = dbscan_pairs(xs, RADIUS["ip"], "ip")
    full = dbscan_reference(xs, RADIUS["ip"], "ip", 3, pairs=full_pairs)
    assert full[1][list(chain)].tolist() == [BORDER, CORE, CORE, CORE, BORDER] and full[2][3] >= 5 and full[1][N] == CORE
    m = int(mask.sum())
    _check(ix, ref, RADIUS["ip"], 3, sel=sel, members=m, skipped=_skipped(pairs))
    _check(ix, full, RADIUS["ip"], 3, skipped=_skipped(full_pairs))
    # a mask: the same members as the selector object when nothing was added since
    sel.close()
    mask2 = np.concatenate([mask, np.zeros(extra, dtype=bool)])
    got = ix.range_dbscan(RADIUS["ip"], 3, sel=mask2)
    for a, b in zip(got[:3], ref[:3]):
        np.testing.assert_array_equal(a, b)
    assert got[3] == counts
    # nothing allowed
    got = ix.range_dbscan(RADIUS["ip"], 3, sel=np.zeros(N + extra, dtype=bool))
    assert (got[0] == -1).all() and (got[1] == NONE).all() and (got[2] == -1).all()
    assert got[3] == {"clusters": 0, "core": 0, "border": 0, "noise": 0, "edges": 0}
    assert ix.dbscan_last_stats()["members"] == 0
    deg, ne = ix.range_degrees(RADIUS["ip"], sel=np.zeros(N + extra, dtype=bool))
    assert (deg == -1).all() and ne == 0
    ix.close()


# ---- identities on the device ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,metric", [("bf16", "ip"), ("f32", "l2")])
def test_identities_on_the_device(idx, parity_corpus, dtype, metric):
    x = parity_corpus[:1500]
    ix = idx.FlatIndex(x.shape[1], metric, dtype)
    ix.add(x)
    n = ix.ntotal
    lims, _, I = ix.range_search_rows(RADIUS[metric], self_mode="above")
    first = np.repeat(np.arange(n), np.diff(lims))
    deg, ne = ix.range_degrees(RADIUS[metric])
    np.testing.assert_array_equal(deg, np.bincount(first, minlength=n) + np.bincount(I, minlength=n))
    assert ne == int(lims[-1]) > 0
    comp, nc, _ = ix.range_components(RADIUS[metric])
    labels, kinds, degrees, counts = ix.range_dbscan(RADIUS[metric], 1)
    np.testing.assert_array_equal(labels, comp)
    assert (kinds == CORE).all() and counts["clusters"] == nc and counts["edges"] == ne
    # min_samples = 2: the components of two or more
    labels, kinds, _, counts = ix.range_dbscan(RADIUS[metric], 2)
    big = np.bincount(comp, minlength=n)[comp] >= 2
    np.testing.assert_array_equal(labels, np.where(big, comp, -1))
    assert counts["border"] == 0 and counts["noise"] == int((~big).sum())
    labels, kinds, _, counts = ix.range_dbscan(RADIUS[metric], 3)
    groups = ix.group_keys(labels)
    assert groups.count == counts["clusters"] == len(set(labels[labels >= 0].tolist())) > 3
    groups.close()
    ix.close()


# ---- edges of the domain -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_small_indexes_and_infinities(idx, dtype):
    rng = np.random.default_rng(49)
    d = 24
    x = _unit(rng.standard_normal((257, d)))
    x[1::2] = _unit(x[0::2][:128] + 0.02 * rng.standard_normal((128, d)))  # pairs (2 i, 2 i + 1)
    for metric in ("ip", "l2"):
        ix = idx.FlatIndex(d, metric, dtype)
        got = ix.range_dbscan(RADIUS[metric], 2)  # an empty index
        assert [a.shape for a in got[:3]] == [(0,)] * 3 and got[3]["clusters"] == 0
        deg, ne = ix.range_degrees(RADIUS[metric])
        assert deg.shape == (0,) and ne == 0
        every = np.float32(-np.inf if metric == "ip" else np.inf)
        done = 0
        for n in (1, 8, 9, 257):
            ix.add(x[done:n])
            done = n
            xs = O.round_dtype(x[:n], dtype)
            ref = dbscan_reference(xs, RADIUS[metric], metric, 2)
            assert ref[3]["clusters"] == n // 2 and ref[3]["noise"] == n % 2 and ref[3]["edges"] == n // 2
            _check(ix, ref, RADIUS[metric], 2, skipped=n - n // 2)
            all_deg = np.full((n,), n - 1, dtype=np.int64)
            ne = n * (n - 1) // 2
            _check(ix, (np.zeros((n,), dtype=np.int64), np.full((n,), CORE, dtype=np.uint8), all_deg,
                        {"clusters": 1, "core": n, "border": 0, "noise": 0, "edges": ne}), every, n, skipped=1)
            _check(ix, (np.full((n,), -1, dtype=np.int64), np.full((n,), NOISE, dtype=np.uint8), all_deg,
                        {"clusters": 0, "core": 0, "border": 0, "noise": n, "edges": ne}), every, n + 1, skipped=1)
            zero = np.zeros((n,), dtype=np.int64)
            _check(ix, (np.arange(n, dtype=np.int64), np.full((n,), CORE, dtype=np.uint8), zero,
                        {"clusters": n, "core": n, "border": 0, "noise": 0, "edges": 0}), -every, 1, skipped=n)
            _check(ix, (np.full((n,), -1, dtype=np.int64), np.full((n,), NOISE, dtype=np.uint8), zero,
                        {"clusters": 0, "core": 0, "border": 0, "noise": n, "edges": 0}), -every, 2, skipped=n)
        ix.close()


def test_query_too_long_for_lds(idx):
    """d = 6152: the fp64 query no longer fits the 48 KiB staged in LDS."""
    rng = np.random.default_rng(53)
    N, d = 300, 6152
    x = _unit(rng.standard_normal((N, d)))
    x[[7, 150, 299, 20]] = _unit(x[7] + (0.02 / np.sqrt(d / 64)) * rng.standard_normal((4, d)))
    x[[30, 40, 250]] = _plane_rows(rng, d, [0, 1, 2])
    xs = O.round_dtype(x, "bf16")
    pairs = dbscan_pairs(xs, RADIUS["ip"], "ip")
    ref = dbscan_reference(xs, RADIUS["ip"], "ip", 3, pairs=pairs)
    assert ref[0][[7, 150, 299, 20, 30, 40, 250]].tolist() == [7, 7, 7, 7, 40, 40, 40]
    assert ref[1][[30, 40, 250]].tolist() == [BORDER, CORE, BORDER] and ref[3]["edges"] == 8
    ix = idx.FlatIndex(d, "ip", "bf16")
    ix.add(x)
    _check(ix, ref, RADIUS["ip"], 3, skipped=_skipped(pairs))
    ix.close()


# ---- arguments, concurrency, memory ------------------------------------------------------------------------
def test_argument_errors(idx):
    from photo_search_engine_amd import _lib
    rng = np.random.default_rng(51)
    N, d = 300, 16
    ix = idx.FlatIndex(d, "ip", "bf16")
    ix.add(rng.standard_normal((N, d)).astype(np.float32))
    with pytest.raises(ValueError):
        ix.range_dbscan(np.nan, 3)
    with pytest.raises(ValueError):
        ix.range_dbscan(0.5, 0)
    L = ix._L  # the C ABI's own checks
    labels = np.zeros((N,), dtype=np.int64)
    degrees = np.zeros((N,), dtype=np.int64)
    ne = ctypes.c_int64(7)
    nan = float("nan")
    assert L.vs_range_degrees(ix._h, None, nan, degrees.ctypes.data, ctypes.byref(ne)) == _lib.VS_ERR_ARG
    assert "NaN" in _lib.last_error()
    assert L.vs_range_degrees(ix._h, None, 0.5, None, ctypes.byref(ne)) == _lib.VS_ERR_ARG
    assert L.vs_range_degrees(ix._h, None, 0.5, degrees.ctypes.data, None) == 0  # (the count is optional)
    assert L.vs_range_dbscan(ix._h, None, nan, 3, labels.ctypes.data, None, None, None, None) == _lib.VS_ERR_ARG
    for bad in (0, -5):
        assert L.vs_range_dbscan(ix._h, None, 0.5, bad, labels.ctypes.data, None, None, None, None) == _lib.VS_ERR_ARG
        assert "min_samples" in _lib.last_error()
    assert L.vs_range_dbscan(ix._h, None, 0.5, 3, None, None, None, None, None) == _lib.VS_ERR_ARG
    # kinds, degrees, counts and n_edges are optional: the labels are the full call's
    assert L.vs_range_dbscan(ix._h, None, 0.5, 3, labels.ctypes.data, None, None, None, None) == 0
    want = ix.range_dbscan(0.5, 3)
    np.testing.assert_array_equal(labels, want[0])
    np.testing.assert_array_equal(degrees, want[2])
    assert want[3]["edges"] > 0
    assert L.vs_dbscan_last_stats(ix._h, None, 12) == _lib.VS_ERR_ARG
    assert L.vs_dbscan_last_times(ix._h, None, 5) == _lib.VS_ERR_ARG
    # a stale selector
    sel = ix.selector(np.ones(N, dtype=bool))
    assert ix.remove_ids([5]) == 1
    with pytest.raises(RuntimeError, match="stale"):
        ix.range_dbscan(0.5, 3, sel=sel)
    with pytest.raises(RuntimeError, match="stale"):
        ix.range_degrees(0.5, sel=sel)
    sel.close()
    ix.close()


def test_two_threads_on_one_handle(idx, parity_corpus):
    x = parity_corpus[:1200]
    ref = dbscan_reference(O.round_dtype(x, "bf16"), RADIUS["ip"], "ip", 3)
    assert ref[3]["border"] >= 1 and ref[3]["clusters"] >= 3
    ix = idx.FlatIndex(x.shape[1], "ip", "bf16")
    ix.add(x)
    out, errors = [None, None], []

    def work(t):
        try:
            out[t] = ix.range_dbscan(RADIUS["ip"], 3)
        except BaseException as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    ix.close()
    assert not errors, errors[0]
    for got in out:
        for a, b in zip(got[:3], ref[:3]):
            np.testing.assert_array_equal(a, b)
        assert got[3] == ref[3]


def test_device_memory_is_returned(idx, parity_corpus):
    x = parity_corpus[:2000]
    ix = idx.FlatIndex(x.shape[1], "ip", "bf16")
    ix.add(x)
    mask = np.arange(2000) % 3 != 0
    L = ix._L
    try:
        for tier in ("scan", "screen"):
            ix.set_range_mode(tier)
            ix.range_dbscan(RADIUS["ip"], 3)  # (the context's workspaces grow once)
            before = int(L.vs_device_bytes_live())
            ix.range_dbscan(RADIUS["ip"], 3)
            ix.range_degrees(RADIUS["ip"])
            ix.range_dbscan(RADIUS["ip"], 3, sel=mask)
            assert int(L.vs_device_bytes_live()) == before, tier
    finally:
        ix.set_range_mode("auto")
    ix.close()


def test_stats_and_times(idx, parity_corpus):
    x = parity_corpus[:1000]
    ix = idx.FlatIndex(x.shape[1], "ip", "bf16")
    ix.add(x)
    ix.set_range_mode("scan")
    labels, kinds, degrees, counts = ix.range_dbscan(RADIUS["ip"], 3)
    st = ix.dbscan_last_stats()
    assert set(st) == {"members", "edges", "clusters", "core", "border", "noise", "tier", "rescanned", "blocks",
                       "rescanned2", "blocks2", "skipped"}
    assert st["members"] == 1000 and st["tier"] == "scan" and st["blocks"] == 4 and 1 <= st["blocks2"] <= 4
    t = ix.dbscan_last_times()
    assert set(t) == {"pass1_screen_ms", "pass1_scan_ms", "pass2_screen_ms", "pass2_scan_ms", "labels_ms"}
    assert t["pass1_scan_ms"] > 0 and t["pass2_scan_ms"] > 0 and t["labels_ms"] > 0
    ix.set_range_mode("auto")
    assert ix.range_dbscan(RADIUS["ip"], 3)[3] == counts
    assert ix.dbscan_last_stats()["tier"] == "screen"
    ix.close()


# ---- multi-device and the product --------------------------------------------------------------------------
def test_multi_device_density_clusters(idx, parity_corpus):
    x = parity_corpus[:1200]
    mi = idx.MultiDeviceFlatIndex(x.shape[1], "ip", "f32", devices=[0, 0])
    got = mi.range_dbscan(RADIUS["ip"], 3)
    assert got[0].shape == (0,) and got[3]["clusters"] == 0
    assert mi.range_degrees(RADIUS["ip"])[0].shape == (0,)
    mi.add(x)
    mask = np.arange(1200) % 4 != 1
    for m in (None, mask):
        pairs = dbscan_pairs(x, RADIUS["ip"], "ip", m)
        want = dbscan_reference(x, RADIUS["ip"], "ip", 3, pairs=pairs)
        got = mi.range_dbscan(RADIUS["ip"], 3, sel=m)
        for a, b in zip(got[:3], want[:3]):
            np.testing.assert_array_equal(a, b)
        assert got[3] == want[3]
        deg, ne = mi.range_degrees(RADIUS["ip"], sel=m)
        np.testing.assert_array_equal(deg, degrees_of_pairs(*pairs[:3]))
        assert ne == want[3]["edges"]
    mi.close()


@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_vector_store_density_clusters(tmp_path, monkeypatch, metric):
    """The store on the device against the store over the oracle index."""
    from photo_search_engine_amd import vector_store as vsmod
    rng = np.random.default_rng(55)
    n, d = 1500, 64
    X = _unit(rng.standard_normal((n, d)))
    # bursts: tight ones (cliques) and loose ones (a minority of their pairs pass: core, border and noise rows)
    for size, noise in ((2, 0.02), (3, 0.02), (9, 0.02), (30, 0.046), (2, 0.02), (17, 0.046), (12, 0.02), (30, 0.05)):
        ids = rng.choice(n, size, replace=False)
        X[ids] = _unit(X[ids[0]] + noise * rng.standard_normal((size, d)))
    meta = [{"photo_path": f"/p/{i}.jpg", "year": 2019 + i % 6} for i in range(n)]
    threshold = float(RADIUS["ip" if metric == "cosine" else "l2"])
    pred = lambda m: m["year"] != 2020  # noqa: E731

    def answers(tag):
        store = vsmod.VectorStore(dimension=d, index_path=str(tmp_path / f"{tag}.idx"),
                                  metadata_path=str(tmp_path / f"{tag}.json"), metric=metric, index_type="flat")
        store.add(X, meta)
        out = []
        for allowed in (None, pred):
            labels, kinds = store.density_labels(threshold, min_samples=4, allowed=allowed)
            out.append((store.neighbor_counts(threshold, allowed=allowed).tolist(), labels.tolist(), kinds.tolist(),
                        store.density_clusters(threshold, min_samples=4, allowed=allowed)))
        return out

    got = answers("gpu")
    monkeypatch.setattr(vsmod, "_index_factory", oracle_dbscan_factory)
    want = answers("cpu")
    kinds = np.array(want[0][2])
    assert (kinds == BORDER).any() and (kinds == NOISE).any() and len(want[0][3]) >= 3 and want[1] != want[0]
    assert got == want

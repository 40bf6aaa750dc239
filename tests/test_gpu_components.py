"""Exact duplicate groups on the GPU (MI355X only): connected components within a radius.

Reference for every case (tests/oracle_components_index.py ``components_reference``): the pair list of
``rows_range_reference(..., self_mode="above")`` over the members and a union-find over it whose roots are the
smallest ids.  ``labels``, ``n_components`` and ``n_edges`` must be bit-equal under the scan tier, the screen
tier (where it applies) and the library's own choice.
"""
import ctypes
import threading

import numpy as np
import pytest

from oracle import oracle as O
from oracle_components_index import components_of_pairs, components_reference

pytestmark = pytest.mark.gpu

COS = 0.95  # a chain's step; its ends meet at cos(2 theta) = 0.805
RADIUS = {"ip": np.float32(0.9), "l2": np.float32(0.2)}  # (unit rows: squared L2 = 2 - 2 cos)


@pytest.fixture(scope="module")
def idx():
    from photo_search_engine_amd import index
    return index


def _tiers(dtype, members, sel):
    screen = sel is None and dtype in ("bf16", "f16") and members >= 9
    return ("scan", "screen", "auto") if screen else ("scan", "auto")


def _check(ix, ref, radius, sel=None, members=None, tiers=None):
    """``range_components`` under every applicable tier against ``ref`` = (labels, n_components, n_edges);
    returns the stats per tier."""
    members = ix.ntotal if members is None else members
    stats = {}
    try:
        for tier in tiers or _tiers(ix.dtype, members, sel):
            ix.set_range_mode(tier)
            labels, nc, ne = ix.range_components(radius, sel=sel)
            assert labels.dtype == np.int64 and labels.shape == (ix.ntotal,)
            np.testing.assert_array_equal(labels, ref[0], err_msg=f"labels, {tier}")
            assert (nc, ne) == (ref[1], ref[2]), tier
            st = stats[tier] = ix.components_last_stats()
            assert (st["members"], st["edges"], st["components"]) == (members, ne, nc), tier
            assert st["blocks"] == (members + 255) // 256
            if tier == "scan":
                assert st["tier"] == "scan" and st["rescanned"] == 0
            if tier == "screen":
                assert st["tier"] == "screen"
    finally:
        ix.set_range_mode("auto")
    return stats


def _unit(x):
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def _chain_rows(rng, d, steps):
    """Unit rows at angles 0, theta, ..., (steps - 1) theta in a random plane, cos(theta) = COS."""
    u, v = np.linalg.qr(rng.standard_normal((d, 2)))[0].T
    t = np.arccos(COS)
    return np.stack([np.cos(i * t) * u + np.sin(i * t) * v for i in range(steps)]).astype(np.float32)


def _near(xs, a, b, metric):
    D = np.float32(O.canon_scores(xs[[b]], xs[[a]], metric)[0, 0])
    return bool(D > RADIUS[metric]) if metric == "ip" else bool(D < RADIUS[metric])


# ---- parity ------------------------------------------------------------------------------------------------
CHAIN = (700, 1500, 2300)
SPAN = (5, 300, 2900)


@pytest.fixture(scope="module")
def parity_corpus():
    rng = np.random.default_rng(41)
    N, d = 3000, 64  # 12 query blocks, 47 workgroups of the scan, query slices, a last partial wave-step
    x = _unit(rng.standard_normal((N, d)))
    free = np.setdiff1d(np.arange(N), np.array(CHAIN + SPAN))
    rng.shuffle(free)
    pos = 0
    for size in (2, 3, 5, 8, 13, 21, 40, 2, 2, 4, 7, 30):  # groups of noisy copies, scattered over the blocks
        ids = free[pos:pos + size]
        pos += size
        x[ids] = _unit(x[ids[0]] + 0.02 * rng.standard_normal((size, d)))
    x[list(CHAIN)] = _chain_rows(rng, d, 3)
    x[list(SPAN)] = _unit(x[SPAN[0]] + 0.02 * rng.standard_normal((3, d)))
    x.setflags(write=False)
    return x


_parity_refs = {}


def _parity_ref(x, dtype, metric):
    if (dtype, metric) not in _parity_refs:
        _parity_refs[dtype, metric] = components_reference(O.round_dtype(x, dtype), RADIUS[metric], metric)
    return _parity_refs[dtype, metric]


@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_parity(idx, parity_corpus, dtype, metric):
    x = parity_corpus
    xs = O.round_dtype(x, dtype)
    ref = _parity_ref(x, dtype, metric)
    labels = ref[0]
    # the planted features are in the reference: a component with a pair inside that is not near, ...
    a, b, c = CHAIN
    assert labels[a] == labels[b] == labels[c] == a and int((labels == a).sum()) >= 3
    assert _near(xs, a, b, metric) and _near(xs, b, c, metric) and not _near(xs, a, c, metric)
    # ... one whose members lie in three query blocks, and groups of many sizes
    assert labels[list(SPAN)].tolist() == [SPAN[0]] * 3 and len({i // 256 for i in SPAN}) == 3
    sizes = np.bincount(labels)
    assert sizes.max() == 40 and int((sizes >= 2).sum()) >= 14 and ref[2] > 1000
    ix = idx.FlatIndex(x.shape[1], metric, dtype)
    ix.add(x)
    stats = _check(ix, ref, RADIUS[metric])
    assert stats["scan"]["blocks"] == 12
    ix.close()


# ---- re-rooting --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_a_root_is_hooked_under_a_smaller_one(idx, dtype):
    """{10, 2000} and {5, 2500} meet only through 2000 - 2500: the root 10 ends under 5."""
    rng = np.random.default_rng(43)
    N, d = 2600, 32
    x = _unit(rng.standard_normal((N, d)))
    x[[10, 2000, 2500, 5]] = _chain_rows(rng, d, 4)
    xs = O.round_dtype(x, dtype)
    assert _near(xs, 10, 2000, "ip") and _near(xs, 2000, 2500, "ip") and _near(xs, 5, 2500, "ip")
    assert not (_near(xs, 5, 10, "ip") or _near(xs, 5, 2000, "ip") or _near(xs, 10, 2500, "ip"))
    ref = components_reference(xs, RADIUS["ip"], "ip")
    assert ref[0][[5, 10, 2000, 2500]].tolist() == [5, 5, 5, 5] and ref[1] == N - 3 and ref[2] == 3
    ix = idx.FlatIndex(d, "ip", dtype)
    ix.add(x)
    _check(ix, ref, RADIUS["ip"])
    ix.close()


# ---- contention --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_every_row_identical(idx, dtype):
    N, d = 2000, 32
    x = np.tile(_unit(np.random.default_rng(45).standard_normal((1, d))), (N, 1))
    ref = (np.zeros((N,), dtype=np.int64), 1, N * (N - 1) // 2)
    ix = idx.FlatIndex(d, "ip", dtype)
    ix.add(x)
    stats = _check(ix, ref, np.float32(0.5))
    assert ("screen" in stats) == (dtype == "bf16")
    ix.close()


def test_screen_overflow_goes_to_the_scan(idx):
    """The construction of test_gpu_range.py: 4,000 copies of one vector stored contiguously, so a workgroup
    of the screen compacts the lists of the queries that are those copies.  Their edge counters start again
    from zero and the scan answers them; the unions their refine made stay, and uniting again changes nothing.
    Random unit rows at d = 64 are nowhere near 0.95 of each other, so the answer is known without a join."""
    rng = np.random.default_rng(57)
    N, d, c0, nc = 300000, 64, 100000, 4000
    x = _unit(rng.standard_normal((N, d)))
    x[c0:c0 + nc] = x[c0]
    labels = np.arange(N, dtype=np.int64)
    labels[c0:c0 + nc] = c0
    ref = (labels, N - nc + 1, nc * (nc - 1) // 2)
    ix = idx.FlatIndex(d, "ip", "bf16")
    ix.add(x)
    stats = _check(ix, ref, np.float32(0.95), tiers=("screen",))  # (the scan of 1172 blocks takes seconds)
    assert stats["screen"]["tier"] == "screen" and stats["screen"]["rescanned"] >= 1
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
    bridge = (100, 400, 800)
    x[list(bridge)] = _chain_rows(rng, d, 3)
    x[N:N + 5] = x[3]  # copies of an allowed row, added after the selector was made
    mask = rng.random(N) < 0.7
    mask[[100, 800, 3]] = True
    mask[400] = False  # the chain's middle: its ends must not join
    xs = O.round_dtype(x, dtype)
    ix = idx.FlatIndex(d, "ip", dtype)
    ix.add(x[:N])
    sel = ix.selector(mask)
    ix.add(x[N:])
    ref = components_reference(xs, RADIUS["ip"], "ip", mask)  # (a mask over the first N rows only)
    assert (ref[0][N:] == -1).all() and (ref[0][:N][~mask] == -1).all() and (ref[0][:N][mask] >= 0).all()
    assert ref[0][100] == 100 and ref[0][800] == 800 and ref[2] > 20
    full = components_reference(xs, RADIUS["ip"], "ip")
    assert full[0][800] == 100 and full[0][N] == 3  # (unfiltered, the bridge joins and the late copies belong)
    m = int(mask.sum())
    _check(ix, ref, RADIUS["ip"], sel=sel, members=m)
    _check(ix, full, RADIUS["ip"])
    # n_edges is the filtered self-join's total
    lims, _, _ = ix.range_search_rows(RADIUS["ip"], ids=np.flatnonzero(mask), sel=sel, self_mode="above")
    assert int(lims[-1]) == ref[2]
    # a mask, ids: the same members as the selector object when nothing was added since
    sel.close()
    mask2 = np.concatenate([mask, np.zeros(extra, dtype=bool)])
    labels, nc, ne = ix.range_components(RADIUS["ip"], sel=mask2)
    np.testing.assert_array_equal(labels, ref[0])
    assert (nc, ne) == ref[1:]
    # nothing allowed
    labels, nc, ne = ix.range_components(RADIUS["ip"], sel=np.zeros(N + extra, dtype=bool))
    assert (labels == -1).all() and (nc, ne) == (0, 0)
    assert ix.components_last_stats()["members"] == 0
    ix.close()


# ---- identity on the device --------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,metric", [("bf16", "ip"), ("f32", "l2")])
def test_identities_on_the_device(idx, parity_corpus, dtype, metric):
    x = parity_corpus[:1500]
    ix = idx.FlatIndex(x.shape[1], metric, dtype)
    ix.add(x)
    lims, _, I = ix.range_search_rows(RADIUS[metric], self_mode="above")
    want = components_of_pairs(ix.ntotal, np.repeat(np.arange(ix.ntotal), np.diff(lims)), I)
    labels, nc, ne = ix.range_components(RADIUS[metric])
    np.testing.assert_array_equal(labels, want)
    assert ne == int(lims[-1]) > 0
    groups = ix.group_keys(labels)
    assert groups.count == nc == int((labels == np.arange(ix.ntotal)).sum())
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
        labels, nc, ne = ix.range_components(RADIUS[metric])  # an empty index
        assert labels.shape == (0,) and (nc, ne) == (0, 0)
        every = np.float32(-np.inf if metric == "ip" else np.inf)
        done = 0
        for n in (1, 8, 9, 257):
            ix.add(x[done:n])
            done = n
            xs = O.round_dtype(x[:n], dtype)
            ref = components_reference(xs, RADIUS[metric], metric)
            assert ref[1] == (n + 1) // 2 and ref[2] == n // 2
            _check(ix, ref, RADIUS[metric])
            _check(ix, (np.zeros((n,), dtype=np.int64), 1, n * (n - 1) // 2), every)
            _check(ix, (np.arange(n, dtype=np.int64), n, 0), -every)
        ix.close()


def test_argument_errors(idx):
    from photo_search_engine_amd import _lib
    rng = np.random.default_rng(51)
    N, d = 300, 16
    ix = idx.FlatIndex(d, "ip", "bf16")
    ix.add(rng.standard_normal((N, d)).astype(np.float32))
    with pytest.raises(ValueError):
        ix.range_components(np.nan)
    L = ix._L  # the C ABI's own checks
    labels = np.zeros((N,), dtype=np.int64)
    nc, ne = ctypes.c_int64(7), ctypes.c_int64(7)
    rc = L.vs_range_components(ix._h, None, float("nan"), labels.ctypes.data, ctypes.byref(nc), ctypes.byref(ne))
    assert rc == _lib.VS_ERR_ARG and "NaN" in _lib.last_error()
    assert L.vs_range_components(ix._h, None, 0.5, None, ctypes.byref(nc), ctypes.byref(ne)) == _lib.VS_ERR_ARG
    assert L.vs_range_components(ix._h, None, 0.5, labels.ctypes.data, None, None) == 0  # (the counts are optional)
    assert L.vs_components_last_stats(ix._h, None, 6) == _lib.VS_ERR_ARG
    # a stale selector
    sel = ix.selector(np.ones(N, dtype=bool))
    assert ix.remove_ids([5]) == 1
    with pytest.raises(RuntimeError, match="stale"):
        ix.range_components(0.5, sel=sel)
    sel.close()
    ix.close()


def test_query_too_long_for_lds(idx):
    """d = 6152: the fp64 query no longer fits the 48 KiB staged in LDS."""
    rng = np.random.default_rng(53)
    N, d = 300, 6152
    x = _unit(rng.standard_normal((N, d)))
    x[[7, 150, 299]] = _unit(x[7] + (0.02 / np.sqrt(d / 64)) * rng.standard_normal((3, d)))
    x[[20, 40]] = _unit(x[20] + (0.02 / np.sqrt(d / 64)) * rng.standard_normal((2, d)))
    xs = O.round_dtype(x, "bf16")
    ref = components_reference(xs, RADIUS["ip"], "ip")
    assert ref[0][[7, 150, 299, 20, 40]].tolist() == [7, 7, 7, 20, 20] and ref[2] == 4
    ix = idx.FlatIndex(d, "ip", "bf16")
    ix.add(x)
    _check(ix, ref, RADIUS["ip"])
    ix.close()


# ---- concurrency, memory -----------------------------------------------------------------------------------
def test_two_threads_on_one_handle(idx, parity_corpus):
    x = parity_corpus[:1200]
    ref = components_reference(O.round_dtype(x, "bf16"), RADIUS["ip"], "ip")
    ix = idx.FlatIndex(x.shape[1], "ip", "bf16")
    ix.add(x)
    out, errors = [None, None], []

    def work(t):
        try:
            out[t] = ix.range_components(RADIUS["ip"])
        except BaseException as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    ix.close()
    assert not errors, errors[0]
    for labels, nc, ne in out:
        np.testing.assert_array_equal(labels, ref[0])
        assert (nc, ne) == ref[1:]


def test_device_memory_is_returned(idx, parity_corpus):
    x = parity_corpus[:2000]
    ix = idx.FlatIndex(x.shape[1], "ip", "bf16")
    ix.add(x)
    mask = np.arange(2000) % 3 != 0
    L = ix._L
    try:
        for tier in ("scan", "screen"):
            ix.set_range_mode(tier)
            ix.range_components(RADIUS["ip"])  # (the context's workspaces grow once)
            before = int(L.vs_device_bytes_live())
            ix.range_components(RADIUS["ip"])
            ix.range_components(RADIUS["ip"], sel=mask)
            assert int(L.vs_device_bytes_live()) == before, tier
    finally:
        ix.set_range_mode("auto")
    ix.close()


def test_stats_and_times(idx, parity_corpus):
    x = parity_corpus[:1000]
    ix = idx.FlatIndex(x.shape[1], "ip", "bf16")
    ix.add(x)
    ix.set_range_mode("scan")
    labels, nc, ne = ix.range_components(RADIUS["ip"])
    st = ix.components_last_stats()
    assert st == {"members": 1000, "edges": ne, "components": nc, "tier": "scan", "rescanned": 0, "blocks": 4}
    t = ix.components_last_times()
    assert set(t) == {"screen_ms", "scan_ms", "readback_ms"} and t["scan_ms"] > 0 and t["readback_ms"] > 0
    ix.set_range_mode("auto")
    assert ix.range_components(RADIUS["ip"])[1:] == (nc, ne)
    assert ix.components_last_stats()["tier"] == "screen"
    ix.close()


# ---- multi-device and the product --------------------------------------------------------------------------
def test_multi_device_range_components(idx, parity_corpus):
    x = parity_corpus[:1200]
    mi = idx.MultiDeviceFlatIndex(x.shape[1], "ip", "f32", devices=[0, 0])
    labels, nc, ne = mi.range_components(RADIUS["ip"])
    assert labels.shape == (0,) and (nc, ne) == (0, 0)
    mi.add(x)
    mask = np.arange(1200) % 4 != 1
    for m in (None, mask):
        want = components_reference(x, RADIUS["ip"], "ip", m)
        labels, nc, ne = mi.range_components(RADIUS["ip"], sel=m)
        np.testing.assert_array_equal(labels, want[0])
        assert (nc, ne) == want[1:]
    mi.close()


@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_vector_store_duplicate_groups(tmp_path, metric):
    from photo_search_engine_amd import vector_store as vsmod
    rng = np.random.default_rng(55)
    n, d = 1500, 64
    X = _unit(rng.standard_normal((n, d)))
    for size in (2, 3, 9, 30, 2, 17):  # bursts
        ids = rng.choice(n, size, replace=False)
        X[ids] = _unit(X[ids[0]] + 0.02 * rng.standard_normal((size, d)))
    meta = [{"photo_path": f"/p/{i}.jpg", "year": 2019 + i % 6} for i in range(n)]
    store = vsmod.VectorStore(dimension=d, index_path=str(tmp_path / "s.idx"), metadata_path=str(tmp_path / "s.json"),
                              metric=metric, index_type="flat")
    store.add(X, meta)
    threshold = float(RADIUS["ip" if metric == "cosine" else "l2"])
    pred = lambda m: m["year"] != 2020  # noqa: E731
    want = store.find_duplicates(threshold)
    assert len(want) >= 5 and max(len(g) for g in want) >= 25
    assert store.duplicate_groups(threshold) == want
    want_f = store.find_duplicates(threshold, allowed=pred)
    assert want_f and want_f != want
    assert store.duplicate_groups(threshold, allowed=pred) == want_f
    labels = store.duplicate_labels(threshold)
    for g in want:
        assert (labels[g] == g[0]).all()
    assert int((labels == np.arange(n)).sum()) == n - sum(len(g) - 1 for g in want)

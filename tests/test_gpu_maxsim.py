"""Exact multi-vector search on the GPU (MI355X only): ``vs_search_maxsim`` through ``FlatIndex.search_maxsim``.

Reference for every case (tests/oracle_maxsim_index.py ``maxsim_reference``): the members scored with the
oracle's canonical fp64 score against every sub-query, per group the best score of each sub-query and the
lowest id that attains it, F their fp64 sum left to right, the groups ordered by (F, code).  All five outputs
must be equal -- ``scores`` as fp64 bits, ``sub_scores`` as fp32 bits -- under every setting of ``SETTINGS``:
the scan, lists of every depth with the fall-through, a row cap that sends everything on, and one query per
table block."""
import contextlib
import functools
import threading

import numpy as np
import pytest

from oracle import oracle as O
from oracle_maxsim_index import KEY_PAD, maxsim_need, maxsim_reference, resolve_depth

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "bf16", "f16"]
METRICS = ["ip", "l2"]
NAMES = ("keys", "scores", "sub_scores", "sub_ids", "sizes")


@pytest.fixture(scope="module")
def idx():
    from photo_search_engine_amd import index
    return index


def settings(k):
    """(tier, first, limit, walk_rows, staging bytes) of every run of a case; 0 = the default."""
    out = [("scan", 0, 0, 0, 0)]
    for first in (1, k, 64):
        for limit in (first, 0):
            out.append(("lists", first, limit, 0, 0))
    out += [("auto", 0, 0, 0, 0), ("auto", 0, 0, 1, 0), ("scan", 0, 0, 0, 1)]
    return list(dict.fromkeys(out))


@contextlib.contextmanager
def setting(idx, ix, s):
    tier, first, limit, walk_rows, staging = s
    try:
        ix.set_maxsim_mode(tier)
        ix.set_maxsim_depth(first, limit, walk_rows)
        if staging:
            idx.set_maxsim_staging_bytes(staging)
        yield
    finally:
        ix.set_maxsim_mode("auto")
        ix.set_maxsim_depth(0, 0, 0)
        idx.set_maxsim_staging_bytes()


def _index(idx, x, dtype, metric):
    ix = idx.FlatIndex(x.shape[1], metric, dtype)
    ix.add(np.ascontiguousarray(x))
    return ix


def _eq(res, ref, what=""):
    for g, w, name in zip(res, ref, NAMES):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, f"{what}: {name} {g.shape} {g.dtype}"
        view = {np.dtype(np.float32): np.uint32, np.dtype(np.float64): np.uint64}.get(g.dtype)
        if view is not None:
            np.testing.assert_array_equal(g.view(view), w.view(view), err_msg=f"{what}: {name}")
        else:
            np.testing.assert_array_equal(g, w, err_msg=f"{what}: {name}")


def _cut(ref, nq, k):
    """A reference at (nq', k') cut to its first nq queries and k groups (the ranking's prefix)."""
    return tuple(a[:nq, :k] for a in ref)


def _check_all(idx, ix, groups, q3, k, ref, what, sel=None, need=None):
    """``need``: (xs, metric, keys) -- the stats of every setting are then held to ``maxsim_need`` too."""
    for s in settings(k):
        with setting(idx, ix, s):
            res = ix.search_maxsim(q3, k, groups, sel=sel)
            st = ix.maxsim_last_stats()
        _eq(res, ref, f"{what} {s}")
        assert st["queries"] == q3.shape[0] and st["first"] + st["deeper"] + st["scan"] == q3.shape[0], (what, s, st)
        assert st["tier"] == ("scan" if s[0] == "scan" else "lists"), (what, s, st)
        if s[0] == "scan":
            assert st["scan"] == q3.shape[0], (what, s, st)
        if need is not None:
            xs, metric, keys = need
            want, _ = maxsim_need(xs, q3, k, metric, keys, *resolve_depth(k, q3.shape[1], s[1], s[2]), walk_rows=s[3], tier=s[0])
            assert {n: st[n] for n in want} == want, (what, s, st, want)


# ---- 1. parity: N = 3000, d = 64 --------------------------------------------------------------------------
PN, PD = 3000, 64


@functools.lru_cache(maxsize=None)
def _parity_keys():
    """About 300 groups of 1..40 rows with keys beyond 2^40, about 5 % of the rows ungrouped (a repeated
    negative key), the members of a group scattered over the rows."""
    rng = np.random.default_rng(41)
    n_un = PN // 20
    sizes = []
    while sum(sizes) < PN - n_un:
        sizes.append(int(min(40, 1 + rng.exponential(9.0))))
    sizes[-1] -= sum(sizes) - (PN - n_un)
    keys = np.concatenate([np.full((s,), (1 << 40) + 7919 * g, dtype=np.int64) for g, s in enumerate(sizes)]
                          + [np.full((n_un,), -5, dtype=np.int64)])
    rng.shuffle(keys)
    assert 250 <= len(sizes) <= 400 and max(sizes) == 40 and min(sizes) >= 1
    keys.setflags(write=False)
    return keys


@functools.lru_cache(maxsize=None)
def _parity(dtype):
    rng = np.random.default_rng(17)
    x = rng.standard_normal((PN, PD)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    q = rng.standard_normal((20, 8, PD)).astype(np.float32)
    q /= np.linalg.norm(q, axis=2, keepdims=True)
    xs = O.round_dtype(x, dtype)
    for a in (x, xs, q):
        a.setflags(write=False)
    return x, xs, q


@functools.lru_cache(maxsize=None)
def _parity_ref(dtype, metric, m, k=100, masked=False):
    _, xs, q = _parity(dtype)
    return maxsim_reference(xs, q[:, :m], k, metric, _parity_keys(), mask=_parity_mask() if masked else None)


@functools.lru_cache(maxsize=None)
def _parity_mask():
    """Empties the groups whose key is 0 mod 3 and thins the others."""
    keys = _parity_keys()
    mask = ((keys - (1 << 40)) // 7919 % 3 != 0) & ((np.arange(PN) % 4 != 1) | (keys < 0))
    mask.setflags(write=False)
    return mask


@pytest.mark.parametrize("m", [1, 3, 8])
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_parity(idx, dtype, metric, m):
    x, xs, q = _parity(dtype)
    ix = _index(idx, x, dtype, metric)
    groups = ix.group_keys(_parity_keys())
    ref = _parity_ref(dtype, metric, m)
    try:
        for nq in (1, 6, 20):
            for k in (1, 10, 100):
                _check_all(idx, ix, groups, q[:nq, :m], k, _cut(ref, nq, k), f"{dtype} {metric} m={m} nq={nq} k={k}")
    finally:
        groups.close()
        ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_k_above_the_groups_that_exist_is_padded(idx, metric):
    x, xs, q = _parity("bf16")
    ix = _index(idx, x, "bf16", metric)
    groups = ix.group_keys(_parity_keys())
    k = 600
    ref = maxsim_reference(xs, q[:3, :3], k, metric, _parity_keys())
    ngroups = int((ref[0][0] != KEY_PAD).sum())
    assert ngroups < k and (ref[4][:, ngroups:] == 0).all() and (ref[3][:, ngroups:] == -1).all()
    assert np.isinf(ref[1][:, ngroups:]).all()
    try:
        _check_all(idx, ix, groups, q[:3, :3], k, ref, f"padding {metric}")
    finally:
        groups.close()
        ix.close()


# ---- 2. sub-queries outside LDS: d = 2560 -----------------------------------------------------------------
@pytest.mark.parametrize("m", [8, 2])
def test_wide_rows_sub_queries_in_global_memory(idx, m):
    """m = 8: 8 fp64 sub-queries of d = 2560 are 160 KiB, more than the scan stages in LDS; m = 2: they fit."""
    n, d, k = 600, 2560, 10
    rng = np.random.default_rng(5)
    x = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((3, m, d)).astype(np.float32)
    keys = rng.integers(0, 60, size=n).astype(np.int64)
    keys[::17] = -1
    for dtype, metric in (("bf16", "ip"), ("f32", "l2")):
        xs = O.round_dtype(x, dtype)
        ix = _index(idx, x, dtype, metric)
        groups = ix.group_keys(keys)
        try:
            _check_all(idx, ix, groups, q, k, maxsim_reference(xs, q, k, metric, keys), f"d=2560 m={m} {dtype} {metric}")
        finally:
            groups.close()
            ix.close()


# ---- 3. a winner outside every list -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _outside():
    d = 8
    rows, keys = [], []
    for j in range(3):  # 50 single-row groups per axis at 0.9 e_j plus small distinct noise
        for i in range(50):
            v = np.zeros((d,), np.float32)
            v[j] = 0.9 + 0.0005 * (i + 1)
            rows.append(v)
            keys.append(1000 + 50 * j + i)
    for j in range(3):  # W: mediocre on every axis
        v = np.zeros((d,), np.float32)
        v[j] = 0.5
        rows.append(v)
        keys.append(7)
    for j, s in ((0, 0.95), (1, 0.4)):  # V: the best row of axis 0, and a row no list holds
        v = np.zeros((d,), np.float32)
        v[j] = s
        rows.append(v)
        keys.append(8)
    rng = np.random.default_rng(3)
    for _ in range(300):
        rows.append((1e-4 * rng.standard_normal(d)).astype(np.float32))
        keys.append(-1)
    x, keys = np.stack(rows), np.asarray(keys, dtype=np.int64)
    perm = rng.permutation(x.shape[0])
    q = np.eye(d, dtype=np.float32)[None, :3, :].copy()
    return x[perm], keys[perm], q


def test_a_winner_outside_every_list(idx):
    x, keys, q = _outside()
    k = 3
    ref = maxsim_reference(x, q, k, "ip", keys)
    assert ref[0][0, 0] == 7 and ref[0][0, 1] == 8  # W wins, then V
    w04 = int(np.flatnonzero((keys == 8) & (x[:, 1] > 0.3))[0])
    assert ref[3][0, 1, 1] == w04 and ref[2][0, 1, 1] == np.float32(0.4)
    # W and the 0.4 row are in no list of 16
    S = O.canon_scores(x, q[0], "ip")
    top16 = {int(i) for j in range(3) for i in np.lexsort((np.arange(x.shape[0]), -S[j]))[:16]}
    assert not top16 & set(np.flatnonzero(keys == 7).tolist()) and w04 not in top16
    ix = _index(idx, x, "f32", "ip")
    groups = ix.group_keys(keys)
    try:
        for limit, where in ((0, 1), (16, 2)):
            first, lim = resolve_depth(k, 3, 16, limit)
            want, at = maxsim_need(x, q, k, "ip", keys, first, lim)
            assert at == [where]
            with setting(idx, ix, ("auto", 16, limit, 0, 0)):
                res = ix.search_maxsim(q, k, groups)
                st = ix.maxsim_last_stats()
            _eq(res, ref, f"outside limit={limit}")
            assert {n: st[n] for n in want} == want, (limit, st, want)
            assert (st["deeper"], st["scan"]) == ((1, 0) if where == 1 else (0, 1))
        _check_all(idx, ix, groups, q, k, ref, "outside", need=(x, "ip", keys))
    finally:
        groups.close()
        ix.close()


# ---- 4. a first-list case ---------------------------------------------------------------------------------
def test_tight_clusters_complete_in_the_first_list(idx):
    rng = np.random.default_rng(11)
    nc, per, d, k = 40, 10, 64, 3
    c = rng.standard_normal((nc, d))
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    x = (np.repeat(c, per, axis=0) + 0.01 * rng.standard_normal((nc * per, d))).astype(np.float32)
    keys = np.repeat(np.arange(nc, dtype=np.int64), per)
    perm = rng.permutation(nc * per)
    x, keys = x[perm], keys[perm]
    q = np.stack([np.stack([c[(3 * a + j) % nc] for j in range(3)]) for a in range(6)]).astype(np.float32)
    for dtype, metric in (("f32", "ip"), ("bf16", "l2")):
        xs = O.round_dtype(x, dtype)
        first, lim = resolve_depth(k, 3)
        want, at = maxsim_need(xs, q, k, metric, keys, first, lim)
        assert at == [0] * 6, (dtype, metric, at)
        ix = _index(idx, x, dtype, metric)
        groups = ix.group_keys(keys)
        try:
            ref = maxsim_reference(xs, q, k, metric, keys)
            res = ix.search_maxsim(q, k, groups)
            st = ix.maxsim_last_stats()
            _eq(res, ref, f"clusters {dtype} {metric}")
            assert {n: st[n] for n in want} == want and st["first"] == 6 and st["walked"] > 0, (st, want)
            _check_all(idx, ix, groups, q, k, ref, f"clusters {dtype} {metric}", need=(xs, metric, keys))
        finally:
            groups.close()
            ix.close()


# ---- 5. ties ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ties():
    """20 distinct vectors of small integers (exact in f16); 10 templates of 2-3 of them, each template the
    member set of 6 groups, with a vector repeated inside some groups: F ties in blocks of 6 and more."""
    rng = np.random.default_rng(29)
    d = 16
    vecs = set()
    while len(vecs) < 20:
        vecs.add(tuple(rng.integers(-3, 4, size=d).tolist()))
    vecs = np.asarray(sorted(vecs), dtype=np.float32)
    rows, keys = [], []
    for t in range(10):
        members = [(2 * t + u) % 20 for u in range(2 + t % 2)]
        for g in range(6):
            for v in members + members[: g % 2]:  # (a duplicate inside every other group)
                rows.append(vecs[v])
                keys.append(100 * t + g)
    x, keys = np.stack(rows), np.asarray(keys, dtype=np.int64)
    perm = rng.permutation(x.shape[0])
    q = rng.integers(-2, 3, size=(4, 3, d)).astype(np.float32)
    return x[perm], keys[perm], q


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_ties_go_to_the_lower_code_and_the_lowest_id(idx, dtype, metric):
    x, keys, q = _ties()
    np.testing.assert_array_equal(O.round_dtype(x, dtype), x)
    ref = maxsim_reference(x, q, 100, metric, keys)
    F = ref[1][:, :60]
    assert all(np.unique(F[a]).shape[0] <= 10 for a in range(4))  # blocks of 6 equal F at the least
    assert (F[:, 9] == F[:, 10]).any()                             # a tie across the k = 10 boundary
    ix = _index(idx, x, dtype, metric)
    groups = ix.group_keys(keys)
    try:
        for k in (1, 10, 100):
            _check_all(idx, ix, groups, q, k, _cut(ref, 4, k), f"ties {dtype} {metric} k={k}")
    finally:
        groups.close()
        ix.close()


# ---- 6. identities ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_identities(idx, dtype, metric):
    x, xs, q = _parity(dtype)
    k = 10
    ref = _parity_ref(dtype, metric, 1)
    F = ref[1][:, : k + 1]
    assert all(np.unique(F[a]).shape[0] == k + 1 for a in range(F.shape[0]))  # the best scores are distinct
    ix = _index(idx, x, dtype, metric)
    groups = ix.group_keys(_parity_keys())
    each = ix.group_keys(5 * np.arange(PN, dtype=np.int64))
    try:
        for tier in ("auto", "scan"):
            with setting(idx, ix, (tier, 0, 0, 0, 0)):
                res = ix.search_maxsim(q[:, :1], k, groups)
                one = ix.search_maxsim(q[:, :1], k, each)
            gr = ix.search_groups(q[:, 0], k, groups, group_size=1)
            np.testing.assert_array_equal(res.keys, gr.keys)
            np.testing.assert_array_equal(res.scores.astype(np.float32).view(np.uint32), gr.D[:, :, 0].view(np.uint32))
            np.testing.assert_array_equal(res.sub_ids[:, :, 0], gr.I[:, :, 0])
            D, I = ix.search(q[:, 0], k)  # every key distinct: vs_search (keys[i] = 5 i)
            np.testing.assert_array_equal(one.sub_ids[:, :, 0], I)
            np.testing.assert_array_equal(one.keys, 5 * I)
            np.testing.assert_array_equal(one.scores.astype(np.float32).view(np.uint32), D.view(np.uint32))
            np.testing.assert_array_equal(one.sub_scores[:, :, 0].view(np.uint32), D.view(np.uint32))
            assert (one.sizes == 1).all()
    finally:
        each.close()
        groups.close()
        ix.close()


# ---- 7. selector and coverage -----------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_selector_and_coverage(idx, metric):
    dtype, m, k, nq = "bf16", 3, 10, 6
    x, xs, q = _parity(dtype)
    q3 = q[:nq, :m]
    ix = _index(idx, x, dtype, metric)
    groups = ix.group_keys(_parity_keys())
    try:
        # a mask that empties some groups and thins others: sizes follow it
        mask = _parity_mask()
        ref = _cut(_parity_ref(dtype, metric, m, masked=True), nq, k)
        plain = _cut(_parity_ref(dtype, metric, m), nq, k)
        assert not np.array_equal(ref[4], plain[4]) and not np.array_equal(ref[0], plain[0])
        sel = ix.selector(mask)
        _check_all(idx, ix, groups, q3, k, ref, f"mask {metric}", sel=sel)
        _eq(ix.search_maxsim(q3, k, groups, sel=mask), ref, "a mask as sel")
        # a score selector as sel
        radius = 0.1 if metric == "ip" else 1.8
        ssel = ix.selector_from_range(q[:2, 0], radius)
        smask = ssel.to_mask()
        assert 0 < smask.sum() < PN
        _check_all(idx, ix, groups, q3, k, maxsim_reference(xs, q3, k, metric, _parity_keys(), mask=smask),
                   f"score selector {metric}", sel=ssel)
        # rows added after group_keys are no members, whatever a later selector allows
        extra = np.ascontiguousarray(x[:200][::-1])
        ix.add(extra)
        xs2 = np.concatenate([xs, O.round_dtype(extra, dtype)])
        _check_all(idx, ix, groups, q3, k, plain, f"rows added {metric}")
        late = np.ones((PN + 200,), dtype=bool)
        late[::3] = False
        lsel = ix.selector(late)
        _check_all(idx, ix, groups, q3, k, maxsim_reference(xs2, q3, k, metric, _parity_keys(), mask=late),
                   f"rows added, a later selector {metric}", sel=lsel)
        _check_all(idx, ix, groups, q3, k, ref, f"rows added, an earlier selector {metric}", sel=sel)
        for s in (sel, ssel, lsel):
            s.close()
    finally:
        groups.close()
        ix.close()


# ---- 8. lifetime and errors -------------------------------------------------------------------------------
def test_member_lists_live_with_the_groups_object(idx):
    from photo_search_engine_amd import _lib
    L = _lib.load()
    x, xs, q = _parity("bf16")
    ix = _index(idx, x, "bf16", "ip")
    q3 = q[:2, :3]
    warm = ix.group_keys(_parity_keys())  # (the context's own buffers grow on the first call)
    for tier in ("auto", "scan"):
        with setting(idx, ix, (tier, 0, 0, 0, 0)):
            ix.search_maxsim(q3, 10, warm)
    warm.close()
    base = int(L.vs_device_bytes_live())
    groups = ix.group_keys(_parity_keys())
    made = int(L.vs_device_bytes_live())
    assert made > base
    ref = _cut(_parity_ref("bf16", "ip", 3), 2, 10)
    _eq(ix.search_maxsim(q3, 10, groups), ref, "first call")
    first = int(L.vs_device_bytes_live())
    ncodes = int(np.unique(_parity_keys()[_parity_keys() >= 0]).shape[0] + (_parity_keys() < 0).sum())
    assert first == made + 4 * PN + 8 * (ncodes + 1)  # the rows by (code, id) and the offsets, nothing else
    for tier in ("auto", "scan"):
        with setting(idx, ix, (tier, 0, 0, 0, 0)):
            _eq(ix.search_maxsim(q3, 10, groups), ref, "second call")
        assert int(L.vs_device_bytes_live()) == first, tier
    groups.close()
    assert int(L.vs_device_bytes_live()) == base
    ix.close()


def test_argument_errors(idx):
    from photo_search_engine_amd import _lib
    x, xs, q = _parity("bf16")
    ix = _index(idx, x[:500], "bf16", "ip")
    other = _index(idx, x[:500], "bf16", "ip")
    keys = np.arange(500, dtype=np.int64) % 50
    groups, foreign = ix.group_keys(keys), other.group_keys(keys)
    sel = ix.selector(np.arange(500) % 2 == 0)
    ix.search_maxsim(q[:1, :2], 5, groups, sel=sel)
    with pytest.raises(_lib.VsError):
        ix.search_maxsim(q[:1, :2], 5, foreign)
    for bad in (np.zeros((1, 0, PD), np.float32), np.zeros((1, 9, PD), np.float32), q[:1, 0], q[:1, :2, :-1]):
        with pytest.raises(ValueError):
            ix.search_maxsim(bad, 5, groups)
    for m, k in ((2, 0), (1, 3277), (8, 1025), (3, 2731)):
        with pytest.raises(_lib.VsError):
            ix.search_maxsim(q[:1, :m], k, groups)
    L = _lib.load()
    out = np.zeros((1, 5), np.int64)
    F = np.zeros((1, 5), np.float64)
    q1 = np.ascontiguousarray(q[:1, :1])
    args = lambda m, k: (ix._h, groups._h, None, q1.ctypes.data, 1, m, k, out.ctypes.data, F.ctypes.data, None, None, None)  # noqa: E731
    assert L.vs_search_maxsim(*args(1, 5)) == 0
    for m, k in ((0, 5), (9, 5), (1, 0), (1, 3277)):
        assert L.vs_search_maxsim(*args(m, k)) == _lib.VS_ERR_ARG, (m, k)
    assert L.vs_search_maxsim(ix._h, groups._h, None, q1.ctypes.data, 1, 1, 5, None, F.ctypes.data, None, None, None) == _lib.VS_ERR_ARG
    assert L.vs_search_maxsim(ix._h, groups._h, None, None, 0, 1, 5, None, None, None, None, None) == 0  # nq = 0
    with pytest.raises(ValueError):
        ix.set_maxsim_mode("most")
    with pytest.raises(_lib.VsError):
        ix.set_maxsim_depth(10, 5)
    with pytest.raises(_lib.VsError):
        ix.set_maxsim_depth(0, 0, -1)
    with pytest.raises(ValueError):
        idx.set_maxsim_staging_bytes(0)
    # stale: a removal, then a reset
    ix.remove_ids([3])
    with pytest.raises(_lib.VsError):
        ix.search_maxsim(q[:1, :2], 5, groups)
    fresh = ix.group_keys(np.arange(499, dtype=np.int64) % 50)
    with pytest.raises(_lib.VsError):
        ix.search_maxsim(q[:1, :2], 5, fresh, sel=sel)  # a stale selector
    ix.search_maxsim(q[:1, :2], 5, fresh)
    ix.reset()
    with pytest.raises(_lib.VsError):
        ix.search_maxsim(q[:1, :2], 5, fresh)
    for o in (sel, groups, fresh, foreign):
        o.close()
    with pytest.raises(_lib.VsError):
        ix.search_maxsim(q[:1, :2], 5, groups)  # closed
    other.close()
    ix.close()


def test_an_empty_member_set_is_all_padding(idx):
    x, xs, q = _parity("bf16")
    ix = _index(idx, x[:100], "bf16", "l2")
    groups = ix.group_keys(np.arange(100, dtype=np.int64) // 7)
    res = ix.search_maxsim(q[:2, :3], 4, groups, sel=np.zeros((100,), dtype=bool))
    _eq(res, maxsim_reference(xs[:100], q[:2, :3], 4, "l2", np.arange(100) // 7, mask=np.zeros((100,), bool)), "empty")
    assert (res.keys == KEY_PAD).all() and np.isposinf(res.scores).all() and (res.sizes == 0).all()
    groups.close()
    ix.close()


# ---- 9. two threads ---------------------------------------------------------------------------------------
def test_two_threads_make_their_first_call_at_once(idx):
    x, xs, q = _parity("bf16")
    ix = _index(idx, x, "bf16", "ip")
    groups = ix.group_keys(_parity_keys())
    ref = _cut(_parity_ref("bf16", "ip", 3), 6, 10)
    out, gate = [None, None], threading.Barrier(2)

    def run(t):
        gate.wait()
        out[t] = ix.search_maxsim(q[:6, :3], 10, groups)

    threads = [threading.Thread(target=run, args=(t,)) for t in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    try:
        for t in range(2):
            assert out[t] is not None
            _eq(out[t], ref, f"thread {t}")
    finally:
        groups.close()
        ix.close()

"""Exact grouped search on the GPU (MI355X only): ``vs_search_groups`` through
``FlatIndex.search_groups``, ``VectorStore.search_grouped`` and the multi-device route.

Reference for every case (tests/oracle_group_index.py ``group_reference``): the members ranked by the
oracle's canonical fp64 score and walked to the end in explicit loops.  ``keys``, ``I``, ``D`` (as
bits), ``found`` and ``sizes`` must be equal, whichever tier answered the query.  The tier a query must
end in follows from the reference alone (``need``: the rank at which its answer became complete), the
number of restricted rounds from the contract's scheme replayed on the reference ranking
(``expected_rounds``).

The burst corpus (256 rows, d = 72: the last 64-element chunk is partial) with four key schemes is the
smallest shape that reaches every tier: under the depths (16, 64) and (k g, k g) its eight queries end
in the first list, in a deeper list and in restricted rounds, some of which take more than one."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import oracle as O
from oracle_diverse_index import burst_corpus, staged_chunk
from oracle_group_index import KEY_PAD, burst_keys, expected_rounds, group_reference, oracle_group_factory

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "bf16", "f16"]
METRICS = ["ip", "l2"]
N, D_ = 256, 72
FLT_MAX = np.float32(3.4028235e38)
BASE = 2 ** 40  # keys far beyond 32 bits: a truncated key would collide or come back wrong
KG = [(2, 1), (10, 1), (10, 3), (4, 8)]
SCHEMES = ["burst", "mod7", "giant", "mixed"]
KMAX = 3276


@pytest.fixture(scope="module")
def idx():
    from photo_search_engine_amd import index
    return index


@functools.lru_cache(maxsize=None)
def _stored(dtype):
    x, q = burst_corpus()
    xs = O.round_dtype(x, dtype)
    xs.setflags(write=False)
    return x, xs, q


@functools.lru_cache(maxsize=None)
def _keys(scheme):
    burst = burst_keys()
    assert burst.shape == (N,) and np.bincount(burst, minlength=40).tolist() == [1 + (5 * b) % 12 for b in range(40)]
    if scheme == "burst":  # 40 small groups
        keys = burst + BASE
    elif scheme == "mod7":  # fewer groups than k = 10: the target clamp, sizes near 37
        keys = np.arange(N, dtype=np.int64) % 7 + BASE
    elif scheme == "giant":  # the large bursts merged: one group floods the top of every ranking
        big = (1 + (5 * burst) % 12) >= 7
        keys = np.where(big, BASE + 1000, burst + BASE)
    else:  # mixed: every fifth burst ungrouped (its rows share one negative key and still stand alone)
        keys = np.where(burst % 5 == 0, -1 - burst, burst + BASE)
    keys = np.ascontiguousarray(keys, dtype=np.int64)
    keys.setflags(write=False)
    return keys


def _depths(k, g):
    """(set_group_depth arguments, (first, limit) as the contract resolves them)."""
    return [((0, 0), (max(4 * k * g, 64), KMAX)), ((16, 64), (16, 64)), ((k * g, k * g), (k * g, k * g))]


@functools.lru_cache(maxsize=None)
def _ref(dtype, metric, scheme, k, g):
    _, xs, q = _stored(dtype)
    out = group_reference(xs, q, _keys(scheme), k, g, metric)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _want_stats(dtype, metric, scheme, k, g, first, limit):
    """(first, deeper, finished, rounds) the call must report: the tiers from ``need`` alone, the
    rounds from the replayed scheme (whose own tiers must agree with ``need``)."""
    _, xs, q = _stored(dtype)
    need = _ref(dtype, metric, scheme, k, g)[5]
    L0, L1 = min(first, limit, N), min(limit, N)
    done0 = (need <= L0) | (L0 >= N)
    done1 = (need <= L1) | (L1 >= N)
    tiers = (int(done0.sum()), int((done1 & ~done0).sum()), int((~done1).sum()))
    sim = expected_rounds(xs, q, _keys(scheme), k, g, metric, first, limit)
    assert tuple(sum(1 for t, _ in sim if t == i) for i in range(3)) == tiers
    return tiers + (sum(r for _, r in sim),)


def _index(idx, x, dtype, metric):
    ix = idx.FlatIndex(x.shape[1], metric, dtype)
    if x.shape[0]:
        ix.add(np.ascontiguousarray(x))
    return ix


def _eq(res, ref, what=""):
    keys, D, I, found, sizes = ref[:5]
    np.testing.assert_array_equal(res.keys, keys, err_msg=f"{what}: keys")
    np.testing.assert_array_equal(res.I, I, err_msg=f"{what}: I")
    np.testing.assert_array_equal(res.D.view(np.uint32), np.asarray(D).view(np.uint32), err_msg=f"{what}: D")
    np.testing.assert_array_equal(res.found, found, err_msg=f"{what}: found")
    np.testing.assert_array_equal(res.sizes, sizes, err_msg=f"{what}: sizes")
    assert res.sizes.dtype == np.int64 and res.found.dtype == np.int32 and res.keys.dtype == np.int64


def _stats(ix):
    st = ix.group_last_stats()
    return st["first"], st["deeper"], st["finished"], st["rounds"]


def _sim_stats(sim):
    return tuple(sum(1 for t, _ in sim if t == i) for i in range(3)) + (sum(r for _, r in sim),)


# ---- 1. the burst corpus: key schemes x depths ---------------------------------------------------------------
@pytest.mark.parametrize("k,g", KG)
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_burst_corpus_key_schemes_and_depths(idx, dtype, metric, k, g):
    x, xs, q = _stored(dtype)
    ix = _index(idx, x, dtype, metric)
    for scheme in SCHEMES:
        groups = ix.group_keys(_keys(scheme))
        assert groups.rows == N and groups.count == np.unique(_keys(scheme)[_keys(scheme) >= 0]).shape[0]
        ref = _ref(dtype, metric, scheme, k, g)
        for depth, resolved in _depths(k, g):
            ix.set_group_depth(*depth)
            what = f"{dtype} {metric} {scheme} k={k} g={g} depth={depth}"
            _eq(ix.search_groups(q, k, groups, g), ref, what)
            st = ix.group_last_stats()
            want = _want_stats(dtype, metric, scheme, k, g, *resolved)
            print(what, st, want)
            assert st["queries"] == 8 and _stats(ix) == want, (what, st, want)
        groups.close()
    ix.close()


def test_every_tier_is_reached_by_the_parametrisation():
    """A condition, not a measurement: over the cases of the test above each of the four stats -- first,
    deeper, finished, and a query that takes more than one restricted round -- is reached (from the
    reference-derived counts, so a run that never left tier 1 cannot pass for the wrong reason)."""
    seen = np.zeros(4, dtype=np.int64)
    for dtype in DTYPES:
        for metric in METRICS:
            for k, g in KG:
                for scheme in SCHEMES:
                    for _, resolved in _depths(k, g):
                        first, deeper, finished, rounds = _want_stats(dtype, metric, scheme, k, g, *resolved)
                        seen += (first, deeper, finished, int(rounds > finished))
    assert (seen >= 1).all(), seen


# ---- 2. ties ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,metric", [("bf16", "ip"), ("f32", "l2"), ("f16", "ip")])
def test_identical_rows_under_different_keys(idx, dtype, metric):
    """Identical rows score alike: the groups they belong to are ordered by the lower id."""
    rng = np.random.default_rng(5)
    x = rng.standard_normal((96, D_)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    copies = np.sort(rng.permutation(96)[:24])
    x[copies] = x[copies[0]]
    keys = np.arange(96, dtype=np.int64) % 5 + BASE
    keys[copies] = BASE + 100 + (np.arange(24)[::-1] // 2)  # pairs of copies, the keys descending with the id
    keys[copies[3]] = -9
    xs = O.round_dtype(x, dtype)
    q = np.ascontiguousarray(xs[[copies[0]]])
    ix = _index(idx, x, dtype, metric)
    groups = ix.group_keys(keys)
    for k, g in ((6, 1), (6, 2), (20, 3)):
        ref = group_reference(xs, q, keys, k, g, metric)
        assert ref[2][0, 0, 0] == copies[0] and ref[0][0, 0] == keys[copies[0]] and ref[0][0, 1] == keys[copies[2]]
        for depth in ((0, 0), (k * g, k * g)):
            ix.set_group_depth(*depth)
            _eq(ix.search_groups(q, k, groups, g), ref, f"ties k={k} g={g} {depth}")


@pytest.mark.parametrize("dtype,metric", [("bf16", "ip"), ("f32", "l2"), ("f16", "ip")])
def test_one_group_of_identical_rows_floods_the_first_list(idx, dtype, metric):
    rng = np.random.default_rng(21)
    x = rng.standard_normal((320, D_)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    copies = np.sort(rng.permutation(320)[:300])
    x[copies] = x[copies[0]]
    keys = np.arange(320, dtype=np.int64) % 4 + BASE
    keys[copies] = BASE + 77
    xs = O.round_dtype(x, dtype)
    q = np.ascontiguousarray(xs[[copies[0]]])
    ref = group_reference(xs, q, keys, 3, 2, metric)
    assert ref[0][0, 0] == BASE + 77 and ref[4][0, 0] == 300 and ref[5][0] > 300 and (ref[3][0] == 2).all()
    ix = _index(idx, x, dtype, metric)
    groups = ix.group_keys(keys)
    ix.set_group_depth(6, 6)  # the first list is one group: restricted rounds must find the rest
    _eq(ix.search_groups(q, 3, groups, 2), ref, "flooded, depth (6, 6)")
    sim = expected_rounds(xs, q, keys, 3, 2, metric, 6, 6)
    assert sim[0][0] == 2 and sim[0][1] >= 1
    assert _stats(ix) == _sim_stats(sim) == (0, 0, 1, sim[0][1]) and ix.group_last_stats()["longest"] == 6
    ix.set_group_depth(0, 0)
    _eq(ix.search_groups(q, 3, groups, 2), ref, "flooded, default depths")
    assert _stats(ix) == _sim_stats(expected_rounds(xs, q, keys, 3, 2, metric, 64, KMAX)) == (0, 1, 0, 0)


# ---- 3. selectors ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_selectors(idx, dtype, metric):
    from photo_search_engine_amd import _lib
    x, xs, q = _stored(dtype)
    keys = _keys("mixed")
    ix = _index(idx, x[:200], dtype, metric)
    early_sel = ix.selector(np.arange(200) % 2 == 0)  # made before the adds: later rows are not selected
    early_groups = ix.group_keys(keys[:200])          # made before the adds: later rows are no members
    ix.add(np.ascontiguousarray(x[200:230]))
    mid_sel = ix.selector(np.arange(230) % 3 != 1)    # covers rows the early groups do not
    ix.add(np.ascontiguousarray(x[230:]))
    groups = ix.group_keys(keys)
    burst = burst_keys()
    mask = (burst % 3 != 0) & (np.arange(N) % 2 == 0)  # empties some groups, shrinks others
    for depth in ((0, 0), (16, 64), (30, 30)):
        ix.set_group_depth(*depth)
        for k, g in ((10, 3), (4, 1)):
            ref = group_reference(xs, q, keys, k, g, metric, mask)
            full = group_reference(xs, q, keys, k, g, metric)
            assert (ref[4] != full[4]).any() and (ref[0] != full[0]).any()
            _eq(ix.search_groups(q, k, groups, g, sel=mask), ref, f"mask k={k} g={g} {depth}")
            em = np.zeros((N,), dtype=bool)
            em[:200] = np.arange(200) % 2 == 0
            _eq(ix.search_groups(q, k, groups, g, sel=early_sel), group_reference(xs, q, keys, k, g, metric, em),
                f"early selector {depth}")
            _eq(ix.search_groups(q, k, early_groups, g), group_reference(xs, q, keys[:200], k, g, metric),
                f"early groups {depth}")
            mm = np.zeros((N,), dtype=bool)
            mm[:230] = np.arange(230) % 3 != 1
            _eq(ix.search_groups(q, k, early_groups, g, sel=mid_sel), group_reference(xs, q, keys[:200], k, g, metric, mm),
                f"early groups, later selector {depth}")
        few = np.zeros((N,), dtype=bool)
        few[[3, 50, 51, 137]] = True
        _eq(ix.search_groups(q, 12, groups, 2, sel=few), group_reference(xs, q, keys, 12, 2, metric, few), "k > groups")
        none = ix.search_groups(q, 4, groups, 2, sel=np.zeros((N,), dtype=bool))
        assert (none.I == -1).all() and (none.found == 0).all() and (none.sizes == 0).all() and (none.keys == KEY_PAD).all()
        assert (none.D == (-FLT_MAX if metric == "ip" else FLT_MAX)).all()
        one = np.zeros((N,), dtype=bool)
        one[137] = True
        _eq(ix.search_groups(q, 4, groups, 2, sel=one), group_reference(xs, q, keys, 4, 2, metric, one), f"one row {depth}")
    ix.set_group_depth(0, 0)
    assert ix.remove_ids([5]) == 1
    for kwargs in (dict(groups=groups), dict(groups=early_groups), dict(groups=ix.group_keys(keys[:-1]), sel=early_sel)):
        with pytest.raises(_lib.VsError) as e:
            ix.search_groups(q, 4, kwargs["groups"], 1, sel=kwargs.get("sel"))
        assert e.value.code == _lib.VS_ERR_ARG
    fresh = ix.group_keys(keys[:-1])
    ix.reset()
    with pytest.raises(_lib.VsError) as e:
        ix.search_groups(q, 4, fresh, 1)
    assert e.value.code == _lib.VS_ERR_ARG


# ---- 4. the identities that pin the contract -----------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_identities_against_search(idx, dtype, metric):
    x, xs, q = _stored(dtype)
    ix = _index(idx, x, dtype, metric)
    mask = np.arange(N) % 3 != 0
    members = int(mask.sum())
    alone = ix.group_keys(np.full((N,), -5, dtype=np.int64))                 # all keys negative
    distinct = ix.group_keys(np.arange(N, dtype=np.int64)[::-1] + BASE)      # all keys distinct
    same = ix.group_keys(np.full((N,), BASE + 3, dtype=np.int64))            # all keys equal
    for depth in ((0, 0), (16, 320)):
        ix.set_group_depth(*depth)
        for sel, m in ((None, N), (mask, members)):
            for k in (10, 64, 300):  # 300 > members: padding
                D, I = ix.search(q, k, sel=sel)
                for groups, key_of in ((alone, lambda i: np.full_like(i, -5)), (distinct, lambda i: N - 1 - i + BASE)):
                    res = ix.search_groups(q, k, groups, 1, sel=sel)
                    np.testing.assert_array_equal(res.I[:, :, 0], I)
                    np.testing.assert_array_equal(res.D[:, :, 0].view(np.uint32), D.view(np.uint32))
                    np.testing.assert_array_equal(res.keys, np.where(I >= 0, key_of(I), KEY_PAD))
                    np.testing.assert_array_equal(res.found, (I >= 0).astype(np.int32))
                    np.testing.assert_array_equal(res.sizes, (I >= 0).astype(np.int64))
            for g in (1, 7, 64):
                D, I = ix.search(q, g, sel=sel)
                res = ix.search_groups(q, 3, same, g, sel=sel)
                np.testing.assert_array_equal(res.I[:, 0, :], I)
                np.testing.assert_array_equal(res.D[:, 0, :].view(np.uint32), D.view(np.uint32))
                assert (res.keys[:, 0] == BASE + 3).all() and (res.keys[:, 1:] == KEY_PAD).all()
                assert (res.found[:, 0] == g).all() and (res.sizes[:, 0] == m).all() and (res.I[:, 1:] == -1).all()
                assert (res.found[:, 1:] == 0).all() and (res.sizes[:, 1:] == 0).all()


# ---- 5. argument errors, empty inputs -----------------------------------------------------------------------------
def _raw(ix, groups, q, nq, k, g, sel=None, keys=True, D=True, I=True, found=True, sizes=True, qnull=False):
    """``vs_search_groups`` itself, outputs pre-filled with sentinels: (rc, keys, D, I, found, sizes)."""
    kk, gg = max(k, 1), max(g, 1)
    n = max(nq, 1)
    Kv = np.full((n, kk), -7, dtype=np.int64)
    Dv = np.full((n, kk, gg), -7.0, dtype=np.float32)
    Iv = np.full((n, kk, gg), -7, dtype=np.int64)
    fv = np.full((n, kk), -7, dtype=np.int32)
    sv = np.full((n, kk), -7, dtype=np.int64)
    p = lambda a, on: a.ctypes.data if on else None  # noqa: E731
    rc = ix._L.vs_search_groups(ix._h, groups, sel, p(q, not qnull), nq, k, g, p(Kv, keys), p(Dv, D), p(Iv, I),
                                p(fv, found), p(sv, sizes))
    return rc, Kv, Dv, Iv, fv, sv


def _untouched(out):
    _, Kv, Dv, Iv, fv, sv = out
    return (Kv == -7).all() and (Dv == -7.0).all() and (Iv == -7).all() and (fv == -7).all() and (sv == -7).all()


def test_argument_errors_and_empty_inputs(idx):
    from photo_search_engine_amd import _lib
    x, xs, q = _stored("bf16")
    ix = _index(idx, x, "bf16", "ip")
    other = _index(idx, x, "bf16", "ip")
    keys = _keys("burst")
    groups, foreign = ix.group_keys(keys), other.group_keys(keys)
    ref = _ref("bf16", "ip", "burst", 10, 3)
    # nq = 0 returns at once, nothing is written
    out = _raw(ix, groups._h, q, 0, 5, 2)
    assert out[0] == 0 and _untouched(out)
    assert ix.search_groups(np.zeros((0, D_), dtype=np.float32), 5, groups, 2).I.shape == (0, 5, 2)
    # found and sizes may be NULL
    rc, Kv, Dv, Iv, fv, sv = _raw(ix, groups._h, q, 8, 10, 3, found=False, sizes=False)
    assert rc == 0 and (fv == -7).all() and (sv == -7).all()
    np.testing.assert_array_equal(Iv, ref[2])
    np.testing.assert_array_equal(Kv, ref[0])
    # argument errors: checked before anything is launched, outputs untouched
    for case in (dict(k=0), dict(k=-3), dict(g=0), dict(g=-1), dict(k=KMAX + 1, g=1), dict(k=1, g=KMAX + 1),
                 dict(k=1092, g=3 + 1), dict(k=58, g=57), dict(keys=False), dict(D=False), dict(I=False),
                 dict(qnull=True), dict(nq=-1), dict(groups=foreign._h), dict(groups=None)):
        flags = {n: v for n, v in case.items() if n not in ("k", "g", "nq", "groups")}
        out = _raw(ix, case.get("groups", groups._h), q, case.get("nq", 8), case.get("k", 10), case.get("g", 3), **flags)
        assert out[0] == _lib.VS_ERR_ARG and _untouched(out), case
    assert _raw(ix, groups._h, q, 8, KMAX, 1)[0] == 0 and _raw(ix, groups._h, q, 8, 1092, 3)[0] == 0  # the limit is legal
    with pytest.raises(TypeError):
        ix.search_groups(q, 3, keys, 1)
    with pytest.raises(ValueError):
        ix.group_keys(keys[:-1])
    h = ctypes.c_void_p()
    assert ix._L.vs_groups_create(ix._h, keys.ctypes.data, N - 1, ctypes.byref(h)) == _lib.VS_ERR_ARG and not h.value
    assert ix._L.vs_groups_create(ix._h, None, N, ctypes.byref(h)) == _lib.VS_ERR_ARG
    # the depth setting: 1 <= first <= limit <= 3276, and k g beyond the limit is an argument error
    for bad in ((-1, 0), (0, KMAX + 1), (65, 64), (KMAX + 1, KMAX + 1)):
        with pytest.raises(_lib.VsError):
            ix.set_group_depth(*bad)
    ix.set_group_depth(4, 29)
    out = _raw(ix, groups._h, q, 8, 10, 3)
    assert out[0] == _lib.VS_ERR_ARG and _untouched(out)
    ix.set_group_depth(4, 30)
    _eq(ix.search_groups(q, 10, groups, 3), ref, "k g == limit")
    # the empty index: all padding
    empty = _index(idx, x[:0], "bf16", "ip")
    eg = empty.group_keys(np.zeros((0,), dtype=np.int64))
    assert eg.rows == 0 and eg.count == 0
    res = empty.search_groups(q, 4, eg, 2)
    assert (res.I == -1).all() and (res.D == -FLT_MAX).all() and (res.found == 0).all() and (res.sizes == 0).all()
    assert (res.keys == KEY_PAD).all()
    assert _raw(empty, eg._h, q, 8, KMAX + 1, 1)[0] == _lib.VS_ERR_ARG


# ---- 6. larger shapes and accounting ------------------------------------------------------------------------------
def test_wide_rows_bf16(idx):
    x, q = burst_corpus(d=1536, nbase=80, nq=3, seed=9)
    keys = np.ascontiguousarray(burst_keys(nbase=80, seed=9, d=1536)[:512] + BASE)
    x = np.ascontiguousarray(x[:512])
    xs = O.round_dtype(x, "bf16")
    ix = _index(idx, x, "bf16", "ip")
    groups = ix.group_keys(keys)
    for depth, k, g in (((0, 0), 10, 3), ((16, 64), 10, 3), ((8, 8), 4, 2)):
        ix.set_group_depth(*depth)
        _eq(ix.search_groups(q, k, groups, g), group_reference(xs, q, keys, k, g, "ip"), f"d = 1536 {depth} k={k} g={g}")


def test_batch_of_300_and_workspace_accounting(idx):
    x, xs, q = _stored("bf16")
    ix = _index(idx, x, "bf16", "ip")
    L = ix._L
    q300 = np.ascontiguousarray(np.tile(q, (38, 1))[:300])
    base = int(L.vs_device_bytes_live())
    groups = ix.group_keys(_keys("giant"))
    assert int(L.vs_device_bytes_live()) > base  # the object's HBM is counted
    ref = tuple(np.tile(a, (38,) + (1,) * (a.ndim - 1))[:300] for a in _ref("bf16", "ip", "giant", 10, 3))
    mask = np.arange(N) % 3 != 0
    ref_m = group_reference(xs, q300[:8], _keys("giant"), 10, 3, "ip", mask)
    ref_m = tuple(np.tile(a, (38,) + (1,) * (a.ndim - 1))[:300] for a in ref_m)
    for depth in ((0, 0), (16, 64), (30, 30)):
        ix.set_group_depth(*depth)
        _eq(ix.search_groups(q300, 10, groups, 3), ref, f"300 queries {depth}")
        st = ix.group_last_stats()
        assert st["queries"] == 300 and st["first"] + st["deeper"] + st["finished"] == 300
        _eq(ix.search_groups(q300, 10, groups, 3, sel=mask), ref_m, f"300 queries, mask {depth}")
    sel = ix.selector(mask)
    before = int(L.vs_device_bytes_live())  # (the context's workspaces exist by now)
    _eq(ix.search_groups(q300, 10, groups, 3, sel=sel), ref_m, "300 queries again")
    assert ix.group_last_stats()["finished"] > 0  # the call went through the rounds' own buffers
    assert int(L.vs_device_bytes_live()) == before
    sel.close()
    with_groups = int(L.vs_device_bytes_live())
    groups.close()
    assert int(L.vs_device_bytes_live()) < with_groups
    again = ix.group_keys(_keys("giant"))
    assert int(L.vs_device_bytes_live()) == with_groups
    again.close()


def test_tiers_run_over_several_staged_chunks(idx):
    """Lists of 1400 rows make a staged chunk 256 queries (8 MiB of pinned staging, 12 L + 4 bytes per
    query), so 300 queries take two.  Key scheme: as in "mixed" every fifth burst is taken apart, but its
    rows are dealt over keys of three rows each that lie anywhere in a ranking; a query that meets one
    of them among its first ten groups is complete only near the end of the list.  Of the eight distinct
    queries the last meets none.  Depths (1400, 1400): tier 1 runs over chunks of 256 + 44.  Depths
    (350, 1400): tier 1 is one chunk, and the 263 queries left, which are no prefix of the batch, go
    through tier 2 as 256 + 7."""
    x, q = burst_corpus(nbase=216, nq=10)
    x, q = np.ascontiguousarray(x[:1400]), q[2:]  # (L = 1400 then holds every member: no restricted rounds)
    xs = O.round_dtype(x, "bf16")
    n, k, g = x.shape[0], 10, 3
    burst = burst_keys(nbase=216)[:n]
    apart = burst % 5 == 0
    keys = np.ascontiguousarray(np.where(apart, BASE + 10 ** 6 + np.cumsum(apart) % (int(apart.sum()) // 3), burst + BASE))
    q300 = np.ascontiguousarray(np.tile(q, (38, 1))[:300])
    ref = tuple(np.tile(a, (38,) + (1,) * (a.ndim - 1))[:300] for a in group_reference(xs, q, keys, k, g, "ip"))
    need = ref[5]
    want = {}
    for first, limit in ((1400, 1400), (350, 1400)):
        done0, done1 = (need <= first) | (first >= n), (need <= limit) | (limit >= n)
        want[(first, limit)] = (int(done0.sum()), int((done1 & ~done0).sum()), int((~done1).sum()), 0)
    # conditions, from the reference alone: both tier loops run over more than one chunk of 256
    assert n == 1400 and staged_chunk(1400, D_) == 256 and staged_chunk(350, D_) >= 300
    assert want[(1400, 1400)] == (300, 0, 0, 0)
    assert want[(350, 1400)][0] >= 1 and want[(350, 1400)][1] >= 257 and want[(350, 1400)][2] == 0
    pending = np.flatnonzero(need > 350)
    assert pending.shape[0] == want[(350, 1400)][1] and (pending != np.arange(pending.shape[0])).any()
    ix = _index(idx, x, "bf16", "ip")
    groups = ix.group_keys(keys)
    for depth in ((1400, 1400), (350, 1400)):
        ix.set_group_depth(*depth)
        _eq(ix.search_groups(q300, k, groups, g), ref, f"300 queries, lists of 1400, depth {depth}")
        assert _stats(ix) == want[depth] and ix.group_last_stats()["longest"] == 1400, (ix.group_last_stats(), want[depth])
    groups.close()
    ix.close()


# ---- 7. routes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index_type,metric", [("flat", "cosine"), ("hnsw", "l2"), ("flat", "l2"), ("hnsw", "cosine")])
def test_store_route_equals_the_oracle_store(tmp_path, monkeypatch, index_type, metric):
    from photo_search_engine_amd import vector_store as vsmod
    x, q = burst_corpus()
    burst = burst_keys()
    meta = [{"photo_path": f"/p/{i}.jpg", "year": 2019 + i % 6, "day": None if burst[i] % 5 == 0 else f"day-{burst[i]}"}
            for i in range(N)]

    def make(sub):
        store = vsmod.VectorStore(dimension=D_, index_path=str(tmp_path / sub / "idx"),
                                  metadata_path=str(tmp_path / sub / "meta.json"), metric=metric, index_type=index_type)
        store.add(np.array(x), meta)
        return store

    gpu = make("gpu")
    monkeypatch.setattr(vsmod, "_index_factory", oracle_group_factory)
    ref = make("ref")
    ref.index._x = gpu.index.reconstruct_n(0, N)  # (the values as stored)
    pred = lambda m: m["year"] != 2020  # noqa: E731
    for qi, k, g in ((0, 10, 3), (3, 1, 1), (5, 1000, 2)):
        for by in ("day", "year", lambda m: m["year"] % 2 or None, (burst // 3).tolist()):
            got = gpu.search_grouped(q[qi].tolist(), k, by, group_size=g)
            assert got == ref.search_grouped(q[qi].tolist(), k, by, group_size=g) and got
            assert gpu.search_grouped(q[qi].tolist(), k, by, g, allowed=pred) == ref.search_grouped(q[qi].tolist(), k, by, g,
                                                                                                   allowed=pred)
    page = gpu.search_grouped(q[5].tolist(), 1000, "day", group_size=12)
    assert sum(len(p["items"]) for p in page) == N and sum(p["size"] for p in page) == N
    assert sum(1 for p in page if p["group"] is None) == int((burst % 5 == 0).sum())
    with pytest.raises(ValueError):
        gpu.search_grouped(q[0, :10].tolist(), 3, "day")
    with pytest.raises(ValueError):
        gpu.search_grouped(q[0].tolist(), 200, "day", group_size=20)


def test_multi_device_route_equals_one_device(idx):
    x, xs, q = _stored("f32")
    keys = _keys("mixed")
    mi = idx.MultiDeviceFlatIndex(D_, "ip", "f32", devices=(0, 0))
    mi.add(np.ascontiguousarray(x[:200]))
    early = mi.group_keys(keys[:200])
    mi.add(np.ascontiguousarray(x[200:]))
    groups = mi.group_keys(keys)
    assert groups.rows == N and groups.count == np.unique(keys[keys >= 0]).shape[0]
    _eq(mi.search_groups(q, 10, groups, 3), _ref("f32", "ip", "mixed", 10, 3), "multi")
    mask = np.arange(N) % 3 != 0
    want = group_reference(xs, q, keys, 10, 3, "ip", mask)
    _eq(mi.search_groups(q, 10, groups, 3, sel=mask), want, "multi, mask")
    _eq(mi.search_groups(q, 10, groups, 3, sel=mi.selector(mask)), want, "multi, selector")
    _eq(mi.search_groups(q, 10, early, 3, sel=mask), group_reference(xs, q, keys[:200], 10, 3, "ip", mask), "multi, early")
    groups.close()
    early.close()
    mi.close()

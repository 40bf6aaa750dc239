"""Exact fused search on the GPU (MI355X only): ``vs_search_fused`` through ``FlatIndex.search_fused`` and
``VectorStore.search_any`` / ``search_all``.

Reference for every case (tests/oracle_fuse_index.py ``fuse_reference``): the members scored with the
oracle's canonical fp64 score against every sub-query, F = max / min along the sub-query axis, ordered by
a stable lexicographic sort on (F, id), ``which`` the first argmax / argmin.  ``I`` and ``which`` must be
equal, ``D`` and ``D_sub`` equal as bits, under every tier and depth; ``fuse_last_stats`` must equal what
``fuse_need`` predicts from the reference rankings alone (the certificate replayed on prefixes of them).

The burst corpus (256 rows, d = 72: the last 64-element chunk is partial; 8 queries) with four families of
fused queries (``burst_families``): three noisy copies of a query, two neighbouring queries, a query and its
negative, and all eight.  Depths: the default, (16, 64) and (k, k)."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from oracle_diverse_index import burst_corpus
from oracle_fuse_index import (FAMILIES, FUSE_WALK_MAX, burst_depths, burst_families, fuse_need, fuse_reference, k_limit,
                               resolve_depth, tier_reach)
from test_fuse_host import check_store

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "bf16", "f16"]
METRICS = ["ip", "l2"]
KS = [1, 10, 100]
N, D_ = 256, 72
FLT_MAX = np.float32(3.4028235e38)
MODES = ["any", "all"]
TIERS = ["auto", "lists", "scan"]


@pytest.fixture(scope="module")
def idx():
    from photo_search_engine_amd import index
    return index


@functools.lru_cache(maxsize=None)
def _stored(dtype):
    x, q = burst_corpus()
    xs = O.round_dtype(x, dtype)
    xs.setflags(write=False)
    return x, xs, q, burst_families(q)


@functools.lru_cache(maxsize=None)
def _ref(dtype, metric, name, k, mode, masked=False):
    _, xs, _, fam = _stored(dtype)
    out = fuse_reference(xs, fam[name], k, metric, mode, (np.arange(N) % 3 != 0) if masked else None)
    for a in out:
        a.setflags(write=False)
    return out


def _index(idx, x, dtype, metric):
    ix = idx.FlatIndex(x.shape[1], metric, dtype)
    if x.shape[0]:
        ix.add(np.ascontiguousarray(x))
    return ix


def _eq(res, ref, what=""):
    for g, w, name in zip(res, ref, ("D", "I", "which", "D_sub")):
        if g.dtype == np.float32:
            np.testing.assert_array_equal(g.view(np.uint32), np.asarray(w).view(np.uint32), err_msg=f"{what}: {name}")
        else:
            np.testing.assert_array_equal(g, w, err_msg=f"{what}: {name}")


def _stats(ix):
    st = ix.fuse_last_stats()
    return {n: st[n] for n in ("first", "deeper", "scan", "longest", "tier")}


def _reset(ix):
    ix.set_fuse_mode("auto")
    ix.set_fuse_depth(0, 0)


# ---- 1. the burst corpus: families x modes x depths x tiers ----------------------------------------------------
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_burst_corpus_families_modes_depths_and_tiers(idx, dtype, metric, k):
    x, xs, q, fam = _stored(dtype)
    ix = _index(idx, x, dtype, metric)
    for name in FAMILIES:
        fq = fam[name]
        for mode in MODES:
            ref = _ref(dtype, metric, name, k, mode)
            for depth in burst_depths(k):
                ix.set_fuse_depth(*depth)
                first, limit = resolve_depth(k, fq.shape[1], *depth)
                for tier in TIERS:
                    ix.set_fuse_mode(tier)
                    what = f"{dtype} {metric} {name} k={k} {mode} depth={depth} tier={tier}"
                    _eq(ix.search_fused(fq, k, mode, return_sub=True), ref, what)
                    want, _ = fuse_need(xs, fq, k, metric, mode, first, limit, tier)
                    st = ix.fuse_last_stats()
                    print(what, st, want)
                    assert _stats(ix) == want and st["queries"] == fq.shape[0], what
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_all_reaches_the_first_list_a_deeper_list_and_the_scan(dtype, metric):
    """From ``fuse_need`` alone (the burst test holds the library's stats to it): ALL completes in the first
    list, in a deeper list and in the scan, on the inputs the table names."""
    _, xs, _, fam = _stored(dtype)

    def need(name, fq, k, depth):
        return fuse_need(xs, fq, k, metric, "all", *resolve_depth(k, fq.shape[1], *depth))

    tier_reach(need, fam)


# ---- 2. identities -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_identities(idx, dtype, metric):
    x, xs, q, fam = _stored(dtype)
    ix = _index(idx, x, dtype, metric)
    mask = np.arange(N) % 3 != 0
    sel = ix.selector(mask)
    for tier in TIERS:
        ix.set_fuse_mode(tier)
        for k in (10, 100):
            # m = 1 under either mode: bit-equal to vs_search / vs_search_sel, which = 0
            for s in (None, sel):
                Dp, Ip = ix.search(q, k, sel=s) if s is not None else ix.search(q, k)
                for mode in MODES:
                    D, I, W, U = ix.search_fused(q[:, None, :], k, mode, sel=s, return_sub=True)
                    what = f"m=1 {mode} {tier} k={k} sel={s is not None}"
                    np.testing.assert_array_equal(I, Ip, err_msg=what)
                    np.testing.assert_array_equal(D.view(np.uint32), Dp.view(np.uint32), err_msg=what)
                    np.testing.assert_array_equal(U[:, :, 0].view(np.uint32), Dp.view(np.uint32), err_msg=what)
                    assert (W == 0).all(), what
            for name in FAMILIES:
                fq = fam[name]
                nsub = fq.shape[1]
                # ANY equals the host merge of the m lists of vs_search(q_j, k)
                lists = [ix.search(np.ascontiguousarray(fq[:, j]), k) for j in range(nsub)]
                D, I, W = ix.search_fused(fq, k, "any")
                for a in range(fq.shape[0]):
                    best = {}
                    for Dj, Ij in lists:
                        for sc, i in zip(Dj[a].tolist(), Ij[a].tolist()):
                            if i >= 0 and (i not in best or (sc > best[i] if metric == "ip" else sc < best[i])):
                                best[i] = sc
                    page = sorted(best.items(), key=lambda t: ((-t[1] if metric == "ip" else t[1]), t[0]))[:k]
                    assert I[a].tolist() == [i for i, _ in page] and D[a].tolist() == [sc for _, sc in page], (name, tier, k, a)
                for mode in MODES:
                    ref = ix.search_fused(fq, k, mode, return_sub=True)
                    _eq(ref, _ref(dtype, metric, name, k, mode), f"{name} {mode} {tier}")
                    # permuting the sub-queries changes only which and the order inside D_sub
                    perm = np.roll(np.arange(nsub), 1)
                    rp = ix.search_fused(np.ascontiguousarray(fq[:, perm]), k, mode, return_sub=True)
                    _eq(rp[:2], ref[:2], f"{name} {mode} {tier} permuted")
                    np.testing.assert_array_equal(rp[3].view(np.uint32), np.ascontiguousarray(ref[3][:, :, perm]).view(np.uint32))
                    ok = ref[1] >= 0
                    np.testing.assert_array_equal(perm[rp[2][ok]], ref[2][ok])
                    # repeating a sub-query changes nothing; which keeps the lower index
                    if nsub < 8:
                        rr = ix.search_fused(np.concatenate([fq, fq[:, :1]], axis=1), k, mode, return_sub=True)
                        _eq(rr[:3], ref[:3], f"{name} {mode} {tier} repeated")
                        np.testing.assert_array_equal(np.ascontiguousarray(rr[3][:, :, :nsub]).view(np.uint32),
                                                      ref[3].view(np.uint32))
    _reset(ix)
    ix.close()


# ---- 3. ties -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_forty_tied_rows(idx, dtype, metric):
    """Rows arange(5, 256, 6)[:40] hold one vector and a sub-query is aimed at it: the 40 rows tie on every
    S_j, so on F.  The lowest ids win under every tier, and the strict certificate sends ALL where
    ``fuse_need`` says."""
    x, _, q, _ = _stored(dtype)
    x = np.array(x)
    tied = np.arange(5, N, 6)[:40]
    x[tied] = x[tied[0]]
    xs = O.round_dtype(x, dtype)
    aim = xs[tied[0]].astype(np.float32)
    fq = np.ascontiguousarray(np.stack([np.stack([aim, aim]), np.stack([aim, q[0]]), np.stack([q[1], aim])]), dtype=np.float32)
    ix = _index(idx, x, dtype, metric)
    for k in (10, 100):
        for mode in MODES:
            ref = fuse_reference(xs, fq, k, metric, mode)
            assert ref[1][0, :min(k, 40)].tolist() == tied[:min(k, 40)].tolist()
            for depth in burst_depths(k):
                ix.set_fuse_depth(*depth)
                first, limit = resolve_depth(k, 2, *depth)
                for tier in TIERS:
                    ix.set_fuse_mode(tier)
                    what = f"ties {dtype} {metric} k={k} {mode} depth={depth} tier={tier}"
                    _eq(ix.search_fused(fq, k, mode, return_sub=True), ref, what)
                    want, _ = fuse_need(xs, fq, k, metric, mode, first, limit, tier)
                    assert _stats(ix) == want, (what, ix.fuse_last_stats(), want)
    # k = 10 inside the 40 ties: the k-th best F equals U at every list shorter than the ties, so the strict
    # certificate cannot close before the list leaves them
    st, where = fuse_need(xs, fq[:1], 10, metric, "all", 16, 64)
    assert where == [1] and st["longest"] == 64
    _reset(ix)
    ix.close()


# ---- 4. selector and arguments -----------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_selector(idx, dtype, metric):
    x, xs, q, fam = _stored(dtype)
    ix = _index(idx, x, dtype, metric)
    mask = np.arange(N) % 3 != 0
    sel = ix.selector(mask)
    worst = -FLT_MAX if metric == "ip" else FLT_MAX
    for name in FAMILIES:
        fq = fam[name]
        for k in (10, 100):
            for mode in MODES:
                ref = _ref(dtype, metric, name, k, mode, True)
                for depth in burst_depths(k):
                    ix.set_fuse_depth(*depth)
                    first, limit = resolve_depth(k, fq.shape[1], *depth)
                    for tier in TIERS:
                        ix.set_fuse_mode(tier)
                        what = f"selector {dtype} {metric} {name} k={k} {mode} depth={depth} tier={tier}"
                        for s in (sel, mask):
                            _eq(ix.search_fused(fq, k, mode, sel=s, return_sub=True), ref, what)
                        want, _ = fuse_need(xs, fq, k, metric, mode, first, limit, tier, mask)
                        assert _stats(ix) == want, (what, ix.fuse_last_stats(), want)
    fq = fam["pair"]
    for tier in TIERS:
        ix.set_fuse_mode(tier)
        ix.set_fuse_depth(0, 0)
        for mode in MODES:
            # a selector that allows nothing: all padding
            D, I, W, U = ix.search_fused(fq, 5, mode, sel=np.zeros((N,), bool), return_sub=True)
            assert (I == -1).all() and (D == worst).all() and (W == -1).all() and (U == worst).all()
            assert ix.fuse_last_stats()["first"] == fq.shape[0]
            # k larger than the member count: padded, which = -1
            few = np.zeros((N,), bool)
            few[[3, 44, 200]] = True
            out = ix.search_fused(fq, 10, mode, sel=few, return_sub=True)
            _eq(out, fuse_reference(xs, fq, 10, metric, mode, few), f"3 members {mode} {tier}")
            assert (out[1][:, 3:] == -1).all() and (out[2][:, 3:] == -1).all() and (out[3][:, 3:] == worst).all()
    _reset(ix)
    ix.close()


def _raw(ix, q, nq, m, mode, k, sel=None, D=True, I=True, W=True, U=True, qnull=False):
    n, kk, mm = max(nq, 1), max(k, 1), max(m, 1)
    Dv = np.full((n, kk), -7.0, dtype=np.float32)
    Iv = np.full((n, kk), -7, dtype=np.int64)
    Wv = np.full((n, kk), -7, dtype=np.int32)
    Uv = np.full((n, kk, mm), -7.0, dtype=np.float32)
    p = lambda a, on: a.ctypes.data if on else None  # noqa: E731
    rc = ix._L.vs_search_fused(ix._h, sel, p(q, not qnull), nq, m, mode, k, p(Dv, D), p(Iv, I), p(Wv, W), p(Uv, U))
    return rc, Dv, Iv, Wv, Uv


def _untouched(out):
    return (out[1] == -7.0).all() and (out[2] == -7).all() and (out[3] == -7).all() and (out[4] == -7.0).all()


def test_argument_errors_stale_selector_and_empty_inputs(idx):
    from photo_search_engine_amd import _lib
    x, xs, q, fam = _stored("bf16")
    ix = _index(idx, x, "bf16", "ip")
    other = _index(idx, x, "bf16", "ip")
    fq = np.ascontiguousarray(fam["pair"])
    ref = _ref("bf16", "ip", "pair", 10, "all")
    out = _raw(ix, fq, 0, 2, 1, 5)  # nq = 0 returns at once
    assert out[0] == 0 and _untouched(out)
    assert ix.search_fused(np.zeros((0, 2, D_), dtype=np.float32), 5)[1].shape == (0, 5)
    rc, Dv, Iv, Wv, Uv = _raw(ix, fq, 8, 2, 1, 10, W=False, U=False)  # which and D_sub may be NULL
    assert rc == 0 and (Wv == -7).all() and (Uv == -7.0).all()
    np.testing.assert_array_equal(Iv, ref[1])
    np.testing.assert_array_equal(Dv.view(np.uint32), ref[0].view(np.uint32))
    for case in (dict(m=0), dict(m=-1), dict(m=9), dict(mode=2), dict(mode=-1), dict(k=0), dict(k=-3), dict(k=k_limit(2) + 1),
                 dict(D=False), dict(I=False), dict(qnull=True), dict(nq=-1)):
        flags = {n: v for n, v in case.items() if n not in ("k", "nq", "m", "mode")}
        out = _raw(ix, fq, case.get("nq", 8), case.get("m", 2), case.get("mode", 1), case.get("k", 10), **flags)
        assert out[0] == _lib.VS_ERR_ARG and _untouched(out), case
    # the limit on k follows m: legal at the limit, an error one past it
    eight = np.ascontiguousarray(fam["eight"])
    assert _raw(ix, eight, 2, 8, 0, FUSE_WALK_MAX // 8)[0] == 0
    out = _raw(ix, eight, 2, 8, 0, FUSE_WALK_MAX // 8 + 1)
    assert out[0] == _lib.VS_ERR_ARG and _untouched(out)
    assert _raw(ix, fq, 8, 2, 1, k_limit(2))[0] == 0
    foreign_sel = other.selector(np.ones((N,), bool))
    out = _raw(ix, fq, 8, 2, 1, 10, sel=foreign_sel._h)
    assert out[0] == _lib.VS_ERR_ARG and _untouched(out)
    # the Python layer
    for bad in (q, fq[:, :, :-1], np.zeros((2, 9, D_), np.float32), np.zeros((2, 0, D_), np.float32)):
        with pytest.raises(ValueError):
            ix.search_fused(bad, 5)
    with pytest.raises(ValueError):
        ix.search_fused(fq, 5, mode="most")
    with pytest.raises(_lib.VsError):
        ix.search_fused(fq, 0)
    # depth and tier settings
    for bad in ((-1, 0), (0, 3277), (65, 64), (3277, 3277)):
        with pytest.raises(_lib.VsError):
            ix.set_fuse_depth(*bad)
    with pytest.raises(ValueError):
        ix.set_fuse_mode("fast")
    assert ix._L.vs_set_fuse_mode(ix._h, 7) == _lib.VS_ERR_ARG
    ix.set_fuse_depth(2000, 3000)  # beyond m = 8's own limit: the call cuts both to 1024
    _eq(ix.search_fused(eight, 10, "all", return_sub=True), _ref("bf16", "ip", "eight", 10, "all"), "depth cut to the limit")
    assert ix.fuse_last_stats()["longest"] == N
    _reset(ix)
    # a stale selector after remove_ids; rows added after the selector was made are not selected
    sel = ix.selector(np.arange(N) % 3 != 0)
    ix.add(np.ascontiguousarray(x[:8]))
    D, I, W = ix.search_fused(fq, 10, "all", sel=sel)
    np.testing.assert_array_equal(I, _ref("bf16", "ip", "pair", 10, "all", True)[1])
    assert ix.remove_ids([5]) == 1
    with pytest.raises(_lib.VsError):
        ix.search_fused(fq, 10, "all", sel=sel)
    # the empty index: all padding
    empty = _index(idx, x[:0], "bf16", "ip")
    D, I, W, U = empty.search_fused(fq, 4, "any", return_sub=True)
    assert (I == -1).all() and (D == -FLT_MAX).all() and (W == -1).all() and (U == -FLT_MAX).all()
    assert empty.fuse_last_stats()["first"] == fq.shape[0]


# ---- 5. shapes that cross the kernels' other edges ---------------------------------------------------------------
def _unit_rows(rng, n, d):
    a = rng.standard_normal((n, d)).astype(np.float32)
    return a / np.linalg.norm(a, axis=1, keepdims=True)


@pytest.mark.parametrize("m", [2, 3])
def test_777_rows_partial_tile_and_idle_workgroups(idx, m):
    """n = 777, d = 40: a partial last tile, and more scan workgroups than some shares hold rows."""
    rng = np.random.default_rng(31)
    x, fq = _unit_rows(rng, 777, 40), _unit_rows(rng, 5 * m, 40).reshape(5, m, 40)
    mask = np.arange(777) % 5 != 1
    for dtype, metric in (("bf16", "ip"), ("f32", "l2")):
        xs = O.round_dtype(x, dtype)
        ix = _index(idx, x, dtype, metric)
        for k, depth in ((7, (0, 0)), (7, (8, 32)), (100, (0, 0))):
            ix.set_fuse_depth(*depth)
            first, limit = resolve_depth(k, m, *depth)
            for mode in MODES:
                for msk in (None, mask):
                    ref = fuse_reference(xs, fq, k, metric, mode, msk)
                    for tier in TIERS:
                        ix.set_fuse_mode(tier)
                        what = f"777 rows {dtype} {metric} m={m} k={k} {mode} depth={depth} tier={tier} mask={msk is not None}"
                        _eq(ix.search_fused(fq, k, mode, sel=msk, return_sub=True), ref, what)
                        want, _ = fuse_need(xs, fq, k, metric, mode, first, limit, tier, msk)
                        assert _stats(ix) == want, (what, ix.fuse_last_stats(), want)
        ix.close()


@pytest.mark.parametrize("m", [2, 8])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_d4096_queries_from_global_memory_and_the_widest_walk(idx, dtype, m):
    """n = 96, d = 4096, k = 5: at m = 8 the scan reads its sub-queries from global memory (they do not fit
    beside the lists in LDS), and the walk holds one sub-query of the product's widest d."""
    rng = np.random.default_rng(37)
    x, fq = _unit_rows(rng, 96, 4096), _unit_rows(rng, 3 * m, 4096).reshape(3, m, 4096)
    xs = O.round_dtype(x, dtype)
    for metric in METRICS:
        ix = _index(idx, x, dtype, metric)
        for mode in MODES:
            ref = fuse_reference(xs, fq, 5, metric, mode)
            for depth in ((0, 0), (8, 32)):
                ix.set_fuse_depth(*depth)
                for tier in TIERS:
                    ix.set_fuse_mode(tier)
                    what = f"d=4096 {dtype} {metric} m={m} {mode} depth={depth} tier={tier}"
                    _eq(ix.search_fused(fq, 5, mode, return_sub=True), ref, what)
                    want, _ = fuse_need(xs, fq, 5, metric, mode, *resolve_depth(5, m, *depth), tier)
                    assert _stats(ix) == want, (what, ix.fuse_last_stats(), want)
        ix.close()


def test_walk_at_capacity(idx):
    """m = 8 at k = VS_FUSE_WALK_MAX / 8 on the burst corpus: the largest k the call admits (padded past the
    256 rows), and a walk of 8 lists of 1024 entries -- VS_FUSE_WALK_MAX -- over 1100 rows."""
    x, xs, q, fam = _stored("bf16")
    k = FUSE_WALK_MAX // 8
    ix = _index(idx, x, "bf16", "ip")
    for mode in MODES:
        ref = fuse_reference(xs, fam["eight"], k, "ip", mode)
        for tier in TIERS:
            ix.set_fuse_mode(tier)
            _eq(ix.search_fused(fam["eight"], k, mode, return_sub=True), ref, f"capacity {mode} {tier}")
    ix.close()
    rng = np.random.default_rng(41)
    big = np.concatenate([np.asarray(x), _unit_rows(rng, 1100 - N, D_)])
    bs = O.round_dtype(big, "bf16")
    ix = _index(idx, big, "bf16", "ip")
    for mode in MODES:
        ref = fuse_reference(bs, fam["eight"], k, "ip", mode)
        for tier in ("auto", "scan"):
            ix.set_fuse_mode(tier)
            _eq(ix.search_fused(fam["eight"], k, mode, return_sub=True), ref, f"capacity, 1100 rows {mode} {tier}")
            want, _ = fuse_need(bs, fam["eight"], k, "ip", mode, *resolve_depth(k, 8), tier)
            assert _stats(ix) == want, (mode, tier, ix.fuse_last_stats(), want)
    ix.close()


def test_batch_of_300_fused_queries(idx):
    """More fused queries than one scan block (256), and the queries a deeper list takes are no prefix."""
    x, xs, q, fam = _stored("bf16")
    ix = _index(idx, x, "bf16", "ip")
    for name, k, depth in (("near3", 10, (16, 64)), ("pair", 1, (16, 64)), ("oppo", 10, (0, 0)), ("pair", 10, (10, 10))):
        fq = np.ascontiguousarray(np.tile(fam[name], (38, 1, 1))[:300])
        ix.set_fuse_depth(*depth)
        for mode in MODES:
            ref = tuple(np.tile(a, (38,) + (1,) * (a.ndim - 1))[:300] for a in _ref("bf16", "ip", name, k, mode))
            _eq(ix.search_fused(fq, k, mode, return_sub=True), ref, f"300 fused queries {name} {mode} {depth}")
            want, _ = fuse_need(xs, fq, k, "ip", mode, *resolve_depth(k, fq.shape[1], *depth))
            assert _stats(ix) == want, (name, mode, ix.fuse_last_stats(), want)
    ix.close()


# ---- 6. scratch accounting ---------------------------------------------------------------------------------------
def test_scratch_is_freed_before_return(idx):
    x, xs, q, fam = _stored("bf16")
    ix = _index(idx, x, "bf16", "ip")
    L = ix._L
    calls = [("near3", 10, (0, 0), "auto"), ("near3", 10, (16, 64), "auto"), ("oppo", 10, (16, 64), "lists"),
             ("pair", 10, (0, 0), "scan")]

    def run():
        took = set()
        for name, k, depth, tier in calls:
            ix.set_fuse_depth(*depth)
            ix.set_fuse_mode(tier)
            for mode in MODES:
                ix.search_fused(fam[name], k, mode, return_sub=True)
                st = ix.fuse_last_stats()
                took |= {w for w in ("first", "deeper", "scan") if st[w]}
        return took

    assert run() == {"first", "deeper", "scan"}  # (every tier's workspaces in the context exist now)
    before = int(L.vs_device_bytes_live())
    assert run() == {"first", "deeper", "scan"}
    assert int(L.vs_device_bytes_live()) == before
    ix.close()


# ---- 7. the store route ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index_type", ["flat", "hnsw"])
def test_store_search_any_and_all(tmp_path, index_type):
    from photo_search_engine_amd import vector_store as vsmod
    x, q = burst_corpus()
    meta = [{"photo_path": f"/p/{i}.jpg", "year": 2019 + i % 6} for i in range(64)]
    store = vsmod.VectorStore(dimension=D_, index_path=str(tmp_path / "idx"), metadata_path=str(tmp_path / "meta.json"),
                              metric="cosine", index_type=index_type)
    store.add(np.array(x[:64]), meta)
    check_store(store, q, meta)
    with pytest.raises(ValueError):
        store.search_any([], 3)

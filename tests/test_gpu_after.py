"""Exact paged search on the GPU (MI355X only): ``vs_search_after`` through ``FlatIndex.search_after`` /
``iter_search`` and ``VectorStore.search_page`` / ``iter_search``.

Reference for every case (tests/oracle_after_index.py ``after_reference``): every row scored with the
oracle's canonical fp64 score, the members in a stable lexicographic order on (S, id), the members at or
before the cursor's position counted into ``rank`` and the next ``k`` returned.  ``I`` and ``rank`` must be
equal and ``D`` equal as bits under every tier, depth and hint; ``after_last_stats`` must equal what
``after_need`` predicts from the reference's ``rank`` alone.

Cursor variants travel as extra queries of one call.  The burst corpus (256 rows, d = 72: the last
64-element chunk is partial; 8 queries) has no tied and no fp32-colliding scores, so the collision corpus
(six rows whose distinct S round to at most two D) and the tied corpus (4000 identical rows) carry the
comparison logic."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from oracle_after_index import (DEEP_RANKS, KMAX, MASK3, MODES, TIED_POSITIONS, after_need, after_reference, burst_cursors,
                                burst_depths, collision_corpus, collision_precondition, cursors_at, deep_corpus,
                                full_ranking, tied_corpus)
from oracle_diverse_index import burst_corpus
from test_after_host import check_store

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "bf16", "f16"]
METRICS = ["ip", "l2"]
KS = [1, 10, 100, 300]
N, D_ = 256, 72


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


def _index(idx, x, dtype, metric):
    ix = idx.FlatIndex(x.shape[1], metric, dtype)
    if x.shape[0]:
        ix.add(np.ascontiguousarray(x))
    return ix


def _eq(res, ref, what=""):
    for g, w, name in zip(res, ref, ("D", "I", "rank")):
        if g.dtype == np.float32:
            np.testing.assert_array_equal(g.view(np.uint32), np.asarray(w).view(np.uint32), err_msg=f"{what}: {name}")
        else:
            np.testing.assert_array_equal(g, w, err_msg=f"{what}: {name}")


def _stats(ix):
    st = ix.after_last_stats()
    return {n: st[n] for n in ("first", "deeper", "scan", "longest", "tier")}


def _check(ix, xs, qs, after, k, metric, mode, depth=(0, 0), hint=None, mask=None, sel=None, ref=None, what=""):
    """One call under (mode, depth, hint) against the reference and ``after_need``."""
    ix.set_after_mode(mode)
    ix.set_after_depth(*depth)
    what = f"{what} {metric} k={k} mode={mode} depth={depth} hint={'none' if hint is None else 'given'} masked={mask is not None}"
    ref = ref if ref is not None else after_reference(xs, qs, after, k, metric, mask)
    out = ix.search_after(qs, k, after, sel=sel if sel is not None else mask, rank_hint=hint, return_rank=True)
    _eq(out, ref, what)
    want, _ = after_need(xs, qs, after, k, metric, mode, depth[0], depth[1], hint, mask)
    st = ix.after_last_stats()
    print(what, st, want)
    assert _stats(ix) == want and st["queries"] == qs.shape[0], what
    return out


# ---- 1. the burst corpus: cursors x modes x depths x masks -----------------------------------------------------
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_burst_corpus_cursors_modes_depths_and_masks(idx, dtype, metric, k):
    x, xs, q = _stored(dtype)
    ix = _index(idx, x, dtype, metric)
    qs, after = burst_cursors(xs, q, k, metric)
    assert (~MASK3[after[after >= 0]]).any()  # (cursors the mask disallows are among them)
    sel = ix.selector(MASK3)
    for mask in (None, MASK3):
        ref = after_reference(xs, qs, after, k, metric, mask)
        for depth in burst_depths(k):
            for mode in MODES:
                _check(ix, xs, qs, after, k, metric, mode, depth, mask=mask, sel=None if mask is None else sel, ref=ref,
                       what=dtype)
    sel.close()
    ix.close()


# ---- 2. chains ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("page", [7, 100])
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_chains_concatenate_to_the_whole_ranking(idx, dtype, metric, page):
    x, xs, q = _stored(dtype)
    ix = _index(idx, x, dtype, metric)
    nq = q.shape[0]
    for mask in (None, MASK3):
        members = N if mask is None else int(mask.sum())
        whole = full_ranking(xs, q, metric, mask)
        lims, Dr, Ir = ix.range_search(q, np.inf if metric == "l2" else -np.inf, sel=mask)
        for a in range(nq):  # (the reference's ranking is the infinite-radius range search's)
            np.testing.assert_array_equal(Ir[lims[a]:lims[a + 1]], whole[a][1])
        for mode in MODES:
            for hints in ("none", "true") if page == 7 and mode != "auto" else ("none", "true", "zero", "oversized"):
                after = np.full((nq,), -1, dtype=np.int64)
                Ds, Is, so_far = [[] for _ in range(nq)], [[] for _ in range(nq)], 0
                while True:
                    hint = {"none": None, "true": np.full((nq,), so_far), "zero": np.zeros((nq,), np.int64),
                            "oversized": np.full((nq,), 5000)}[hints]
                    D, I, rank = _check(ix, xs, q, after, page, metric, mode, hint=hint, mask=mask,
                                        what=f"{dtype} chain {hints} at {so_far}")
                    assert (rank == so_far).all()
                    if hints == "true" and mode != "scan":  # one list of hint + k (or the default first list)
                        st = ix.after_last_stats()
                        assert st["first"] == nq and st["longest"] == min(max(so_far + page, 4 * page, 64), members)
                    got = (I >= 0).sum(axis=1)
                    assert (got == got[0]).all()
                    for a in range(nq):
                        Ds[a].append(D[a, : got[a]])
                        Is[a].append(I[a, : got[a]])
                    so_far += int(got[0])
                    if got[0] < page:
                        break
                    after = I[:, page - 1].copy()
                assert so_far == members
                for a in range(nq):
                    np.testing.assert_array_equal(np.concatenate(Is[a]), whole[a][1])
                    np.testing.assert_array_equal(np.concatenate(Ds[a]).view(np.uint32), whole[a][0].view(np.uint32))
        # iter_search yields the same pages
        ix.set_after_mode("auto")
        pages = list(ix.iter_search(q, page, sel=mask))
        assert len(pages) == members // page + 1
        for j, (D, I) in enumerate(pages):
            for a in range(nq):
                part = whole[a][1][j * page:(j + 1) * page]
                np.testing.assert_array_equal(I[a, : part.shape[0]], part)
                assert (I[a, part.shape[0]:] == -1).all()
                np.testing.assert_array_equal(D[a, : part.shape[0]].view(np.uint32),
                                              whole[a][0][j * page:(j + 1) * page].view(np.uint32))
    ix.close()


# ---- 3. fp32 collisions: distinct S behind one D ---------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_cursor_inside_a_run_of_equal_fp32_scores(idx, dtype, metric):
    x, qv, rows = collision_corpus()
    xs = O.round_dtype(x, dtype)
    collision_precondition(xs, qv, rows, metric)
    ix = _index(idx, x, dtype, metric)
    q6 = np.ascontiguousarray(np.repeat(qv[None, :], 6, axis=0))
    for k in (1, 4, 10):
        for mode in ("lists", "scan", "auto"):
            for depth in ((0, 0), (8, 8)):
                D, I, rank = _check(ix, xs, q6, rows, k, metric, mode, depth, what=f"{dtype} collision")
        assert sorted(rank.tolist()) == [1, 2, 3, 4, 5, 6]  # (the six rows lead the ranking)
    # a chain of pages of one row walks the run in S order
    after, seen = np.asarray([-1]), []
    for _ in range(6):
        D, I = ix.search_after(qv[None, :], 1, after)
        seen.append(int(I[0, 0]))
        after = I[:, 0]
    assert seen == after_reference(xs, qv[None, :], -1, 6, metric)[1][0].tolist() and sorted(seen) == rows.tolist()
    ix.close()


# ---- 4. ties beyond the limit ----------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_thousands_of_rows_tied_with_the_cursor(idx, dtype, metric):
    x, q, tied = tied_corpus()
    xs = O.round_dtype(x, dtype)
    ix = _index(idx, x, dtype, metric)
    # the random query, then the zero query (under the inner product every row ties at 0)
    qs = np.ascontiguousarray(np.repeat(q, len(TIED_POSITIONS), axis=0))
    after = np.concatenate([tied[list(TIED_POSITIONS)]] * 2)
    for k in (10, 300):
        ref = after_reference(xs, qs, after, k, metric)
        for j, p in enumerate(TIED_POSITIONS):  # (the random query) pages of the tied run come in id order
            np.testing.assert_array_equal(ref[1][j, : min(k, 3999 - p)], tied[p + 1:p + 1 + min(k, 3999 - p)])
        for mode in MODES:
            _check(ix, xs, qs, after, k, metric, mode, ref=ref, what=f"{dtype} tied")
        _, where = after_need(xs, qs, after, k, metric)
        assert where[0] != 2 and where[2:5] == [2, 2, 2]  # AUTO reaches the scan where the page leaves the limit
        _check(ix, xs, qs, after, k, metric, "auto", hint=ref[2], ref=ref, what=f"{dtype} tied, true hint")
    ix.close()


# ---- 5. beyond the limit -------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_cursors_beyond_the_depth_limit(idx, dtype, metric):
    x, q = deep_corpus()
    xs = O.round_dtype(x, dtype)
    ix = _index(idx, x, dtype, metric)
    mask = np.arange(4096) % 5 != 1
    for m in (None, mask):
        members = 4096 if m is None else int(m.sum())
        ranks = [r for r in DEEP_RANKS if r < members - 1] + [members - 1]
        qs, after = cursors_at(xs, q, ranks, metric, m)
        for k in (10, 300):
            ref = after_reference(xs, qs, after, k, metric, m)
            assert ref[2].tolist() == [r + 1 for r in ranks] * q.shape[0]
            assert (ref[1][len(ranks) - 1] == -1).all() and ref[2][len(ranks) - 1] == members  # the last member: all padding
            assert ((ref[1] >= 0).sum(axis=1) < k).sum() >= 2 * q.shape[0]  # (padded pages)
            for mode in MODES:
                _check(ix, xs, qs, after, k, metric, mode, mask=m, ref=ref, what=f"{dtype} deep")
            _check(ix, xs, qs, after, k, metric, "auto", hint=ref[2], mask=m, ref=ref, what=f"{dtype} deep, true hint")
    ix.close()


# ---- 6. the lists through the int8 screen --------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_lists_from_the_int8_screen(idx, dtype, metric):
    x, xs, q = _stored(dtype)
    ix = _index(idx, x, dtype, metric)
    ix.set_screen("int8")
    ix.set_scan_limit(0)
    k = 10
    qs, after = burst_cursors(xs, q, k, metric)
    assert qs.shape[0] >= 16
    for mask in (None, MASK3):
        ref = after_reference(xs, qs, after, k, metric, mask)
        for depth in burst_depths(k):
            for mode in ("auto", "lists"):
                _check(ix, xs, qs, after, k, metric, mode, depth, mask=mask, ref=ref, what=f"{dtype} i8")
        _check(ix, xs, qs[:16], after[:16], k, metric, "lists", mask=mask, what=f"{dtype} i8, 16 queries")
    ix.close()


# ---- 7. edges ----------------------------------------------------------------------------------------------------
def test_edges(idx):
    from photo_search_engine_amd import _lib
    x, xs, q = _stored("f32")
    ix = _index(idx, x, "f32", "ip")
    # nq = 0
    D, I, rank = ix.search_after(np.zeros((0, D_), np.float32), 5, np.zeros((0,), np.int64), return_rank=True)
    assert D.shape == (0, 5) and I.shape == (0, 5) and rank.shape == (0,) and ix.after_last_stats()["queries"] == 0
    # k and after out of range, before anything is launched
    for k in (0, KMAX + 1):
        with pytest.raises(_lib.VsError):
            ix.search_after(q, k, -1)
    for bad in (-2, N):
        with pytest.raises(_lib.VsError):
            ix.search_after(q, 5, bad)
    with pytest.raises(_lib.VsError):
        ix.set_after_depth(20, 10)
    with pytest.raises(ValueError):
        ix.set_after_mode("deep")
    # forcing LISTS with (k, k) on a deep cursor still ends exact, by falling through to the scan
    k = 10
    qs, after = cursors_at(xs, q, [0, 100, 250], "ip")
    _check(ix, xs, qs, after, k, "ip", "lists", (k, k), what="edges")
    assert ix.after_last_stats()["scan"] == 24 and ix.after_last_stats()["longest"] == k
    # scratch is freed: the live bytes return to their value after a first round of the same calls (the
    # context's own workspaces, the selector road's included, exist by then)
    ix.set_after_depth(0, 0)
    for mode in MODES:
        ix.set_after_mode(mode)
        ix.search_after(qs, k, after, sel=MASK3)
        ix.search_after(qs, k, after)
    L = _lib.load()
    live = int(L.vs_device_bytes_live())
    for mode in MODES:
        ix.set_after_mode(mode)
        ix.search_after(qs, k, after, sel=MASK3)
        ix.search_after(qs, k, after)
    assert int(L.vs_device_bytes_live()) == live
    ix.set_after_mode("auto")
    # a stale selector; a cursor row added after the selector was made
    sel = ix.selector(MASK3)
    extra = np.ascontiguousarray(0.5 * (x[:4] + x[4:8]))
    ix.add(extra)
    xs2 = np.concatenate([xs, extra])
    cur = np.asarray([N, N + 1, N + 2, N + 3, 5, 6, 7, -1], dtype=np.int64)
    for mode in MODES:
        _check(ix, xs2, q, cur, k, "ip", mode, mask=MASK3, sel=sel, what="edges, cursor behind the selector")
    ix.remove_ids([3])
    with pytest.raises(_lib.VsError):
        ix.search_after(q, k, -1, sel=sel)
    sel.close()
    ix.close()
    # an empty index: only -1 is legal, the answer is all padding
    empty = idx.FlatIndex(D_, "l2", "bf16")
    D, I, rank = empty.search_after(q, 3, -1, return_rank=True)
    assert (I == -1).all() and (D == np.float32(3.4028235e38)).all() and (rank == 0).all()
    with pytest.raises(_lib.VsError):
        empty.search_after(q, 3, 0)
    empty.close()
    # an empty member set on a full index
    ix = _index(idx, x, "f32", "ip")
    D, I, rank = ix.search_after(q, 3, 5, sel=np.zeros((N,), bool), return_rank=True)
    assert (I == -1).all() and (rank == 0).all() and ix.after_last_stats()["first"] == 8
    ix.close()
    # d = 1
    rng = np.random.default_rng(2)
    x1 = rng.standard_normal((300, 1)).astype(np.float32)
    q1 = np.asarray([[1.0], [-0.5], [0.0]], dtype=np.float32)
    for metric in METRICS:
        ix = _index(idx, x1, "f32", metric)
        qs, after = cursors_at(x1, q1, [0, 17, 150, 299], metric)
        for mode in MODES:
            _check(ix, x1, qs, after, 7, metric, mode, what="d=1")
        ix.close()


# ---- 8. the store ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_store_search_page_and_iter_search(tmp_path, metric):
    from photo_search_engine_amd import vector_store as vsmod
    x, q = burst_corpus()
    meta = [{"photo_path": f"/p/{i}.jpg", "year": 2019 + i % 6} for i in range(N)]
    store = vsmod.VectorStore(dimension=D_, index_path=str(tmp_path / "idx"), metadata_path=str(tmp_path / "meta.json"),
                              metric=metric, index_type="flat")
    store.add(np.array(x), meta)
    check_store(store, q, meta, "ip" if metric == "cosine" else "l2")

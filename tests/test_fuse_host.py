"""The fused search's reference recipe and the store route, without a GPU: the contract's identities on
``fuse_reference``, where ``fuse_need`` sends ALL on the burst corpus (the tier-reach table of the GPU test),
and ``VectorStore.search_any`` / ``search_all`` on the oracle index against explicit loops over all rows."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from oracle_diverse_index import burst_corpus
from oracle_fuse_index import (FAMILIES, burst_families, fuse_need, fuse_reference, k_limit,
                               oracle_fuse_factory, resolve_depth, tier_reach)
from oracle_sel_index import filtered_reference

N, D_ = 256, 72
KS = [1, 10, 100]


@functools.lru_cache(maxsize=None)
def _corpus(dtype="f32"):
    x, q = burst_corpus()
    xs = O.round_dtype(x, dtype)
    xs.setflags(write=False)
    return xs, q, burst_families(q)


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want, what=""):
    for g, w, name in zip(got, want, ("D", "I", "which", "D_sub")):
        if g.dtype == np.float32:
            np.testing.assert_array_equal(_bits(g), _bits(w), err_msg=f"{what}: {name}")
        else:
            np.testing.assert_array_equal(g, w, err_msg=f"{what}: {name}")


def host_merge(xs, fq, k, metric, mask=None):
    """ANY as the reference's merge: the m plain top-k lists, the union, the best score per id, the first k
    by (score, id)."""
    nq, m, _ = fq.shape
    worst = np.float32(-3.4028235e38 if metric == "ip" else 3.4028235e38)
    D = np.full((nq, k), worst, dtype=np.float32)
    I = np.full((nq, k), -1, dtype=np.int64)
    allow = np.ones((xs.shape[0],), bool) if mask is None else mask
    for a in range(nq):
        best = {}
        for j in range(m):
            Dj, Ij = filtered_reference(xs, fq[a, j:j + 1], allow, k, metric)
            for s, i in zip(Dj[0].tolist(), Ij[0].tolist()):
                if i >= 0 and (i not in best or (s > best[i] if metric == "ip" else s < best[i])):
                    best[i] = s
        page = sorted(best.items(), key=lambda t: ((-t[1] if metric == "ip" else t[1]), t[0]))[:k]
        for r, (i, s) in enumerate(page):
            I[a, r], D[a, r] = i, s
    return D, I


@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_reference_identities(metric):
    xs, q, fam = _corpus()
    mask = np.arange(N) % 3 != 0
    for k in KS:
        for m in (None, mask):
            # m = 1 under either mode: the plain (filtered) search, which = 0
            Dp, Ip = filtered_reference(xs, q, np.ones((N,), bool) if m is None else m, k, metric)
            for mode in ("any", "all"):
                D, I, W, U = fuse_reference(xs, q[:, None, :], k, metric, mode, m)
                _same((D, I), (Dp, Ip), f"m=1 {mode}")
                assert (W == 0).all()
                np.testing.assert_array_equal(_bits(U[:, :, 0]), _bits(Dp))
            for name in FAMILIES:
                fq = fam[name]
                nsub = fq.shape[1]
                D, I, W, U = fuse_reference(xs, fq, k, metric, "any", m)
                Dm, Im = host_merge(xs, fq, k, metric, m)
                _same((D, I), (Dm, Im), f"{name} ANY against the host merge")
                for mode in ("any", "all"):
                    ref = fuse_reference(xs, fq, k, metric, mode, m)
                    # D is the sub-score `which` names, and no other sub-score beats it (ANY) / is worse (ALL)
                    ok = ref[1] >= 0
                    picked = np.take_along_axis(ref[3], np.maximum(ref[2], 0)[:, :, None].astype(np.int64), axis=2)[:, :, 0]
                    np.testing.assert_array_equal(_bits(picked[ok]), _bits(ref[0][ok]))
                    # a permutation changes only which and the order inside D_sub
                    perm = np.roll(np.arange(nsub), 1)
                    rp = fuse_reference(xs, fq[:, perm], k, metric, mode, m)
                    _same(rp[:2], ref[:2], f"{name} {mode} permuted")
                    np.testing.assert_array_equal(_bits(rp[3]), _bits(ref[3][:, :, perm]))
                    # a repeated sub-query changes nothing; which keeps the lower index
                    if nsub < 8:
                        rr = fuse_reference(xs, np.concatenate([fq, fq[:, :1]], axis=1), k, metric, mode, m)
                        _same(rr[:3], ref[:3], f"{name} {mode} repeated")
                        np.testing.assert_array_equal(_bits(rr[3][:, :, :nsub]), _bits(ref[3]))


@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_all_reaches_the_first_list_a_deeper_list_and_the_scan(dtype, metric):
    xs, q, fam = _corpus(dtype)

    def need(name, fq, k, depth):
        first, limit = resolve_depth(k, fq.shape[1], *depth)
        st, where = fuse_need(xs, fq, k, metric, "all", first, limit)
        assert st["first"] + st["deeper"] + st["scan"] == fq.shape[0] and st["tier"] == "lists"
        return st, where

    tier_reach(need, fam)
    # ANY needs one list of k and never deepens; a forced scan takes every query
    st, where = fuse_need(xs, fam["pair"], 10, metric, "any", 16, 64)
    assert st == {"first": 8, "deeper": 0, "scan": 0, "longest": 10, "tier": "lists"} and where == [0] * 8
    st, where = fuse_need(xs, fam["pair"], 10, metric, "all", 16, 64, "scan")
    assert st == {"first": 0, "deeper": 0, "scan": 8, "longest": 0, "tier": "scan"} and where == [2] * 8
    assert resolve_depth(10, 8) == (64, 1024) and resolve_depth(100, 2, 0, 300) == (300, 300) and k_limit(3) == 2730


def test_all_finds_rows_outside_every_per_query_list():
    """Why ALL needs the index: for ``oppo`` (q, -q) the best rows under the worst score are near the
    equator, far down both sub-queries' lists."""
    xs, q, fam = _corpus()
    D, I, W, U = fuse_reference(xs, fam["oppo"], 5, "ip", "all")
    S = O.canon_scores(xs, q, "ip")
    for a in range(8):
        rank = np.empty((N,), dtype=np.int64)
        rank[np.lexsort((np.arange(N), -S[a]))] = np.arange(N)
        assert rank[I[a]].min() >= 64 and (N - 1 - rank[I[a]]).min() >= 64


# ---- VectorStore.search_any / search_all on the oracle index ---------------------------------------------
def _store(tmp_path, monkeypatch, metric="cosine", n=N):
    from photo_search_engine_amd import vector_store as vsmod
    monkeypatch.setattr(vsmod, "_index_factory", oracle_fuse_factory)
    x, q = burst_corpus()
    meta = [{"photo_path": f"/p/{i}.jpg", "year": 2019 + i % 6} for i in range(n)]
    store = vsmod.VectorStore(dimension=D_, index_path=str(tmp_path / "idx"), metadata_path=str(tmp_path / "meta.json"),
                              metric=metric, index_type="flat")
    if n:
        store.add(np.array(x[:n]), meta)
    return store, q, meta


def fused_loops(xs, queries, mode, metric, top_k, allowed=None):
    """``[(row, distance, matched_query, distances)]`` in explicit loops over every row."""
    ip = metric == "ip"
    S = O.canon_scores(xs, np.stack(queries), metric)
    rows = []
    for row in range(xs.shape[0]):
        if allowed is not None and not allowed[row]:
            continue
        sub = [S[j, row] for j in range(len(queries))]
        f, which = sub[0], 0
        for j, s in enumerate(sub):
            better = s > f if ip else s < f
            worse = s < f if ip else s > f
            if better if mode == "any" else worse:
                f, which = s, j
        rows.append(((-f if ip else f), row, f, which, sub))
    rows.sort(key=lambda t: (t[0], t[1]))
    return [(row, float(np.float32(f)), which, [float(np.float32(s)) for s in sub]) for _, row, f, which, sub in rows[:top_k]]


def check_store(store, q, meta, metric="ip"):
    xs = store.index._x if hasattr(store.index, "_x") else store.index.reconstruct_n(0, len(meta))
    wordings = [(2.5 * q[0]).tolist(), q[3].tolist(), (0.5 * q[0] + 0.5 * q[5]).tolist()]  # (normalised by the store)
    queries = [store._normalize_query(w)[0] for w in wordings]
    pred = lambda m: m["year"] != 2020  # noqa: E731
    for method, mode in ((store.search_any, "any"), (store.search_all, "all")):
        for allowed in (None, pred):
            mask = None if allowed is None else [allowed(m) for m in meta]
            for top_k in (1, 10):
                got = method(wordings, top_k, allowed=allowed)
                want = fused_loops(xs, queries, mode, metric, top_k, mask)
                assert [(meta.index(r["metadata"]), r["distance"], r["matched_query"], r["distances"]) for r in got] == want
                assert all(set(r) == {"metadata", "distance", "matched_query", "distances"} for r in got)
    # one embedding: search's page with matched_query 0
    plain = store.search(wordings[1], 10)
    for method in (store.search_any, store.search_all):
        page = method([wordings[1]], 10)
        assert [(r["metadata"], r["distance"]) for r in page] == [(r["metadata"], r["distance"]) for r in plain]
        assert all(r["matched_query"] == 0 and r["distances"] == [r["distance"]] for r in page)


def test_store_search_any_and_all_equal_explicit_loops(tmp_path, monkeypatch):
    store, q, meta = _store(tmp_path, monkeypatch)
    check_store(store, q, meta)
    # the clamp, and a filter that leaves fewer than top_k items
    assert len(store.search_any([q[0].tolist(), q[1].tolist()], 1000)) == N
    few = store.search_all([q[0].tolist(), q[1].tolist()], 10, allowed=[3, 44, 200])
    assert sorted(meta.index(r["metadata"]) for r in few) == [3, 44, 200]
    l2, _, meta16 = _store(tmp_path / "l2", monkeypatch, metric="l2", n=16)
    xs = l2.index._x
    got = l2.search_all([q[0].tolist(), q[1].tolist()], 5)
    want = fused_loops(xs, [l2._normalize_query(q[j].tolist())[0] for j in (0, 1)], "all", "l2", 5)
    assert [(meta16.index(r["metadata"]), r["distance"], r["matched_query"], r["distances"]) for r in got] == want


def test_store_argument_errors(tmp_path, monkeypatch):
    store, q, meta = _store(tmp_path, monkeypatch)
    for method in (store.search_any, store.search_all):
        with pytest.raises(ValueError):
            method([], 5)
        with pytest.raises(ValueError):
            method([q[0].tolist(), q[1].tolist()[:-1]], 5)
        with pytest.raises(ValueError):
            method([q[0].tolist()] * 9, 5)
    empty, _, _ = _store(tmp_path / "empty", monkeypatch, n=0)
    assert empty.search_any([q[0].tolist()], 5) == [] and empty.search_all([q[0].tolist(), q[1].tolist()], 5) == []
    with pytest.raises(ValueError):
        empty.search_any([], 5)


def test_oracle_index_fuse_surface():
    ix = oracle_fuse_factory(D_, "cosine")
    xs, q, fam = _corpus()
    ix.add(np.array(xs))
    out = ix.search_fused(fam["pair"], 10, "all", return_sub=True)
    _same(out, fuse_reference(xs, fam["pair"], 10, "ip", "all"))
    assert len(ix.search_fused(fam["pair"], 10)) == 3
    sel = ix.selector(np.arange(N) % 3 != 0)
    _same(ix.search_fused(fam["near3"], 10, "any", sel=sel, return_sub=True),
          fuse_reference(xs, fam["near3"], 10, "ip", "any", np.arange(N) % 3 != 0))
    for bad in (q, fam["pair"][:, :, :-1], np.zeros((2, 9, D_), np.float32), np.zeros((2, 0, D_), np.float32)):
        with pytest.raises(ValueError):
            ix.search_fused(bad, 5)
    with pytest.raises(ValueError):
        ix.search_fused(fam["pair"], 5, mode="most")
    with pytest.raises(RuntimeError):
        ix.search_fused(fam["eight"], 1025)
    ix.remove_ids([3])
    with pytest.raises(RuntimeError):
        ix.search_fused(fam["pair"], 5, sel=sel)

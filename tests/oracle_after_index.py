"""TEST INFRASTRUCTURE: the reference recipe the GPU tests hold ``vs_search_after`` to, an
``OracleAfterFlatIndex`` with FlatIndex's ``search_after`` / ``iter_search`` surface so
``VectorStore.search_page`` / ``iter_search`` run on the CPU, and the corpora of tests/test_gpu_after.py.

Recipe (include/vs.h "paged search"): every row scored with the oracle's canonical fp64 score S, the members
ordered by a stable lexicographic sort on (S in the metric's direction, id) -- numpy compares doubles
numerically, so +0.0 and -0.0 tie and the id decides.  The cursor row c has the position (S_c, c); the
members at or before it are a prefix of that order, ``rank`` is its length and the page is the next ``k``
members.  ``after_reference`` knows nothing of lists or tiers.  ``after_need`` replays the contract's
completion rule on the reference's ``rank`` alone: a list of L members holds min(rank, L) entries at or before
the cursor, so it completes a query iff rank + k <= L or L holds every member."""
from __future__ import annotations

import numpy as np

from oracle import oracle as O
from oracle_diverse_index import burst_corpus
from oracle_fuse_index import OracleFuseFlatIndex
from oracle_sel_index import FLT_MAX
from photo_search_engine_amd.index import after_arrays, iter_pages

KMAX = 3276
MODES = ("auto", "lists", "scan")


def _member_ids(n: int, mask):
    member = np.ones((n,), dtype=bool)
    if mask is not None:
        m = np.asarray(mask, dtype=bool)[:n]
        member[: m.shape[0]] &= m
        member[m.shape[0]:] = False  # rows added after the selector was made are not selected
    return np.flatnonzero(member).astype(np.int64)


def _rankings(xs, q, metric: str, mask):
    """(key nq x n, ids, [members in ranking order per query]): key = -S (ip) or S (l2), smaller is better."""
    q = np.ascontiguousarray(q, dtype=np.float32)
    ids = _member_ids(xs.shape[0], mask)
    S = O.canon_scores(xs, q, metric) if xs.shape[0] else np.zeros((q.shape[0], 0))
    key = -S if metric == "ip" else S
    orders = [ids[np.lexsort((ids, key[a, ids]))] for a in range(q.shape[0])]
    return S, key, ids, orders


def _rank_of(key_row, ids, c: int) -> int:
    """Members at or before the cursor (key_row[c], c): a better key, or an equal key and an id <= c."""
    if c < 0:
        return 0
    km = key_row[ids]
    return int(((km < key_row[c]) | ((km == key_row[c]) & (ids <= c))).sum())


def after_reference(xs, q, after, k: int, metric: str, mask=None):
    """(D float32 nq x k, I int64 nq x k, rank int64 nq) of ``search_after(q, k, after)`` over rows ``xs`` (the
    values as stored); ``after`` one row id per query (or a scalar), -1 = from the top; ``mask`` restricts the
    members, not the cursor."""
    q = np.ascontiguousarray(q, dtype=np.float32)
    nq, k, ip = int(q.shape[0]), int(k), metric == "ip"
    after, _ = after_arrays(nq, after)
    D = np.full((nq, k), -FLT_MAX if ip else FLT_MAX, dtype=np.float32)
    I = np.full((nq, k), -1, dtype=np.int64)
    rank = np.zeros((nq,), dtype=np.int64)
    S, key, ids, orders = _rankings(xs, q, metric, mask)
    for a in range(nq):
        c = int(after[a])
        assert -1 <= c < xs.shape[0], "after must be -1 or a stored row"
        p = _rank_of(key[a], ids, c)
        page = orders[a][p:p + k]
        rank[a] = p
        I[a, : page.shape[0]] = page
        D[a, : page.shape[0]] = S[a, page].astype(np.float32)
    return D, I, rank


def full_ranking(xs, q, metric: str, mask=None):
    """Per query (D float32, I int64) of the members' whole ranking: what ``range_search`` with an infinite
    radius returns."""
    S, _, _, orders = _rankings(xs, q, metric, mask)
    return [(S[a, o].astype(np.float32), o) for a, o in enumerate(orders)]


def resolve_depth(k: int, first: int = 0, limit: int = 0):
    """(first, limit) as ``set_after_depth`` resolves them."""
    lim = limit if limit > 0 else KMAX
    return min(first if first > 0 else max(4 * k, 64), lim), lim


def after_need(xs, q, after, k: int, metric: str, mode: str = "auto", first: int = 0, limit: int = 0, hint=None,
               mask=None):
    """What ``after_last_stats`` must report -- {"first", "deeper", "scan", "longest", "tier"} -- and per query
    where it completed (0 first list, 1 deeper list, 2 scan), from the reference ranking alone.  ``first`` /
    ``limit`` as given to ``set_after_depth``; ``hint`` as ``rank_hint`` (None, a scalar or one per query)."""
    assert mode in MODES
    q = np.ascontiguousarray(q, dtype=np.float32)
    nq, k = int(q.shape[0]), int(k)
    after, hint = after_arrays(nq, after, hint)
    first, limit = resolve_depth(k, first, limit)
    tier = "scan" if mode == "scan" else "lists"
    _, key, ids, _ = _rankings(xs, q, metric, mask)
    members = int(ids.shape[0])
    if members == 0 or nq == 0:
        return {"first": nq, "deeper": 0, "scan": 0, "longest": 0, "tier": tier}, [0] * nq
    p = [_rank_of(key[a], ids, int(after[a])) for a in range(nq)]
    where = [2] * nq
    pending, L0 = [], first
    for a in range(nq):
        h = -1 if hint is None else int(hint[a])
        beyond = h >= 0 and h + k > limit
        if mode == "scan" or (mode == "auto" and beyond):
            continue  # straight to the scan
        pending.append(a)
        if h >= 0 and not beyond:
            L0 = max(L0, h + k)
    done, longest = [0, 0], 0
    if pending:
        Lmax = min(limit, members)
        L, t = min(L0, Lmax), 0
        while True:
            left = [a for a in pending if not (L >= members or p[a] + k <= L)]
            for a in set(pending) - set(left):
                where[a] = t
            done[t] += len(pending) - len(left)
            pending, longest = left, L
            if not pending or L >= Lmax:
                break
            L, t = min(4 * L, Lmax), 1
    return {"first": done[0], "deeper": done[1], "scan": where.count(2), "longest": longest, "tier": tier}, where


class OracleAfterFlatIndex(OracleFuseFlatIndex):
    def search_after(self, q, k: int, after, sel=None, rank_hint=None, return_rank: bool = False):
        q = np.ascontiguousarray(q, dtype=np.float32)
        if q.ndim != 2 or q.shape[1] != self.d:
            raise ValueError(f"search_after expects an (nq, {self.d}) array, got {q.shape}")
        if not 1 <= int(k) <= KMAX:
            raise RuntimeError("k must be in 1..3276")
        after, _ = after_arrays(q.shape[0], after, rank_hint)
        if after.size and (int(after.min()) < -1 or int(after.max()) >= self.ntotal):
            raise RuntimeError("after must be -1 or a stored row's id")
        D, I, rank = after_reference(self._x, q, after, int(k), "ip" if self.metric_type == 0 else "l2", self._mask(sel))
        return (D, I, rank) if return_rank else (D, I)

    def iter_search(self, q, page: int, sel=None):
        q = np.ascontiguousarray(q, dtype=np.float32)
        if int(page) < 1:
            raise ValueError("page must be >= 1")
        return iter_pages(lambda after, hint: self.search_after(q, page, after, sel=sel, rank_hint=hint, return_rank=True),
                          q.shape[0], page)


def oracle_after_factory(dimension: int, metric: str):
    return OracleAfterFlatIndex(dimension, "ip" if metric == "cosine" else "l2")


# ---- the corpora of tests/test_gpu_after.py (and their CPU checks in tests/test_after_host.py) -------------
CURSOR_RANKS = (0, None, 15, 16, 63, 64, 199, 254, 255)  # (None stands for k - 1)
FIXED_ID = 77
MASK3 = np.arange(256) % 3 != 0
BURST_DEPTHS = ((0, 0), (16, 64), None, (16, 256))  # (None stands for (k, k))


def burst_cursors(xs, q, k: int, metric: str):
    """The burst test's one call: (queries, after) -- every query once per cursor variant: -1, the rows ranked
    0, k-1, 15, 16, 63, 64, 199, 254 and 255 in the query's own ranking of all rows, and one fixed id."""
    _, _, _, orders = _rankings(xs, q, metric, None)
    qs, after = [], []
    for a in range(q.shape[0]):
        last = orders[a].shape[0] - 1  # (k - 1 beyond the last row, at k = 300: the last row)
        variants = [-1] + [int(orders[a][min(k - 1, last) if r is None else r]) for r in CURSOR_RANKS] + [FIXED_ID]
        for c in variants:
            qs.append(q[a])
            after.append(c)
    return np.ascontiguousarray(np.stack(qs), dtype=np.float32), np.asarray(after, dtype=np.int64)


def burst_depths(k: int):
    return [(k, k) if d is None else d for d in BURST_DEPTHS]


COLLISION_M = (3, 0, 5, 1, 4, 2)  # the six rows' component, in units of 2^-24, in id order: not their S order
COLLISION_J = 11


def collision_corpus(seed: int = 3):
    """(x, qv, rows): the burst corpus with six rows appended that differ in one component alone -- 0 in the
    base row, m 2^-24 (m = 1..5: exact in f32, bf16 and f16) in its five copies, in the id order COLLISION_M --
    and the query qv (cosine about 0.6 with the base row, 2^-4 in that component).  The six canonical scores
    are distinct and differ by about 2^-28 per step, under one fp32 ulp in all: they round to at most two
    values of D."""
    x, _ = burst_corpus()
    d = x.shape[1]
    rng = np.random.default_rng(seed)
    base = rng.standard_normal(d)
    base[COLLISION_J] = 0.0
    base /= np.linalg.norm(base)
    u = rng.standard_normal(d)
    u[COLLISION_J] = 0.0
    u -= (u @ base) * base
    u /= np.linalg.norm(u)
    qv = 0.6 * base + 0.8 * u
    qv[COLLISION_J] = 2.0 ** -4
    six = np.repeat(base[None, :], 6, axis=0)
    six[:, COLLISION_J] = np.asarray(COLLISION_M, dtype=np.float64) * 2.0 ** -24
    xx = np.ascontiguousarray(np.concatenate([x, six.astype(np.float32)]), dtype=np.float32)
    rows = np.arange(x.shape[0], x.shape[0] + 6, dtype=np.int64)
    xx.setflags(write=False)
    return xx, np.ascontiguousarray(qv, dtype=np.float32), rows


def collision_precondition(xs, qv, rows, metric: str):
    """Asserts what the collision test rests on: the six rows have pairwise distinct S, at least three of them
    share one D = (float)S, and inside that run the id order is not the S order."""
    S = O.canon_scores(xs[rows], qv[None, :], metric)[0]
    assert np.unique(S).shape[0] == 6, S
    Df = S.astype(np.float32)
    vals, counts = np.unique(Df, return_counts=True)
    assert vals.shape[0] <= 2 and counts.max() >= 3, (S, Df)
    run = np.flatnonzero(Df == vals[np.argmax(counts)])
    key = -S[run] if metric == "ip" else S[run]
    assert not np.array_equal(np.argsort(key, kind="stable"), np.arange(run.shape[0])), (run, key)


TIED_POSITIONS = (0, 1, 3275, 3276, 3999)


def tied_corpus(seed: int = 5, d: int = 72):
    """(x, q, tied_ids): 4096 rows, 4000 of them one and the same unit vector and 96 distinct ones spread among
    them (every 43rd id, from 7 on); two queries -- a random one, under which some distinct rows rank before
    the tied run and some behind it, and the zero vector, under which every row ties (inner product)."""
    rng = np.random.default_rng(seed)
    n = 4096
    same = rng.standard_normal(d)
    same /= np.linalg.norm(same)
    x = np.repeat(same[None, :], n, axis=0)
    distinct = 7 + 43 * np.arange(96)
    other = rng.standard_normal((96, d))
    x[distinct] = other / np.linalg.norm(other, axis=1, keepdims=True)
    tied = np.setdiff1d(np.arange(n), distinct).astype(np.int64)
    assert tied.shape[0] == 4000 and distinct.max() < n
    qr = rng.standard_normal(d)
    qr /= np.linalg.norm(qr)
    q = np.stack([qr, np.zeros(d)])
    x = np.ascontiguousarray(x, dtype=np.float32)
    x.setflags(write=False)
    return x, np.ascontiguousarray(q, dtype=np.float32), tied


DEEP_RANKS = (3270, 3276, 4000, 4090, 4095)


def deep_corpus(seed: int = 9, d: int = 72, nq: int = 2):
    """(x, q): 4096 random unit rows and ``nq`` random unit queries."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((4096, d))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    q = rng.standard_normal((nq, d))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    x = np.ascontiguousarray(x, dtype=np.float32)
    x.setflags(write=False)
    return x, np.ascontiguousarray(q, dtype=np.float32)


def cursors_at(xs, q, ranks, metric: str, mask=None):
    """(queries, after): every query once per rank in ``ranks``, the cursor on the member ranked there."""
    _, _, _, orders = _rankings(xs, q, metric, mask)
    qs, after = [], []
    for a in range(q.shape[0]):
        for r in ranks:
            qs.append(q[a])
            after.append(int(orders[a][r]))
    return np.ascontiguousarray(np.stack(qs), dtype=np.float32), np.asarray(after, dtype=np.int64)

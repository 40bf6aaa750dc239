"""TEST INFRASTRUCTURE: the reference recipe the GPU tests hold ``vs_search_maxsim`` to, and an
``OracleMaxSimFlatIndex`` with FlatIndex's ``search_maxsim`` surface so ``VectorStore.search_multivector``
runs on the CPU.

Recipe (include/vs.h "multi-vector search"): the members scored with the oracle's canonical fp64 score
against every sub-query; per group code the maximum (minimum for L2) of each sub-query's scores and the lowest
member id that attains it; ``F`` the fp64 sum of those, left to right; the groups ordered by a stable
lexicographic sort on (F in the metric's direction, code).  A code is the index of a non-negative key among
the distinct ones, ascending, or ``G + u`` for the u-th ungrouped row.  ``maxsim_reference`` knows nothing of
lists or tiers.  ``maxsim_need`` replays the contract's certificate and row cap on prefixes of the
sub-queries' reference rankings and says, per query, in which list it completes or that the scan answers
it."""
from __future__ import annotations

import numpy as np

from oracle import oracle as O
from oracle_after_index import OracleAfterFlatIndex
from oracle_fuse_index import FUSE_MAX_Q, _fq, k_limit
from oracle_sel_index import FLT_MAX
from photo_search_engine_amd.index import MaxSimResult

KEY_PAD = np.iinfo(np.int64).min
WALK_ROWS_PER_QUERY, WALK_ROWS_QUERIES = 400, 256  # the default row cap: 400 min(nq, 256)


def group_codes(keys):
    """(code int64 per covered row, key of every code int64 [G + U], G)."""
    keys = np.asarray(keys, dtype=np.int64)
    grouped = keys >= 0
    uniq = np.unique(keys[grouped])
    G = int(uniq.shape[0])
    code = np.empty(keys.shape, dtype=np.int64)
    code[grouped] = np.searchsorted(uniq, keys[grouped])
    code[~grouped] = G + np.arange(int((~grouped).sum()))
    return code, np.concatenate([uniq, keys[~grouped]]), G


def _members(keys, n_cov, mask):
    n_cov = int(keys.shape[0] if n_cov is None else n_cov)
    member = np.ones((n_cov,), dtype=bool)
    if mask is not None:
        mk = np.asarray(mask, dtype=bool)[:n_cov]
        member[mk.shape[0]:] = False
        member[: mk.shape[0]] &= mk
    return np.flatnonzero(member).astype(np.int64)


def _sub_scores(xs, fq, ids, metric: str):
    """S[a, j, c]: the canonical fp64 score of member column c with sub-query j of query a."""
    nq, m, d = fq.shape
    S = O.canon_scores(xs[ids], fq.reshape(nq * m, d), metric)
    return np.asarray(S, dtype=np.float64).reshape(nq, m, ids.shape[0])


def _group_best(S, ids, code, ip: bool):
    """Per query: (the codes that have a member, ascending; M [nq, m, groups]; the lowest member id that
    attains each M; the members of each group)."""
    order = np.lexsort((ids, code))  # members by (code, id)
    cs, rows = code[order], ids[order]
    starts = np.flatnonzero(np.concatenate([[True], cs[1:] != cs[:-1]]))
    seg = np.cumsum(np.concatenate([[False], cs[1:] != cs[:-1]]))
    Ss = S[:, :, order]
    M = (np.maximum if ip else np.minimum).reduceat(Ss, starts, axis=2)
    pos = np.where(Ss == M[:, :, seg], np.arange(order.shape[0]), order.shape[0])
    first = np.minimum.reduceat(pos, starts, axis=2)  # (the rows ascend inside a group)
    sizes = np.diff(np.concatenate([starts, [order.shape[0]]]))
    return cs[starts], M, rows[first], sizes


def _sum_left_to_right(M):
    F = M[:, 0].copy()
    for j in range(1, M.shape[1]):
        F = F + M[:, j]
    return F


def maxsim_reference(xs, q3, k: int, metric: str, keys, n_cov=None, mask=None):
    """(keys int64 nq x k, F float64 nq x k, D_sub float32 nq x k x m, I_sub int64 nq x k x m, sizes int64
    nq x k) of ``search_maxsim(q3, k, groups(keys))`` over rows ``xs`` (the values as stored; ``keys`` covers
    the first ``len(keys)`` of them, ``n_cov`` cuts that further); ``mask`` restricts the members."""
    fq = _fq(q3)
    keys = np.asarray(keys, dtype=np.int64)
    nq, m, k, ip = int(fq.shape[0]), int(fq.shape[1]), int(k), metric == "ip"
    Ko = np.full((nq, k), KEY_PAD, dtype=np.int64)
    F = np.full((nq, k), -np.inf if ip else np.inf, dtype=np.float64)
    U = np.full((nq, k, m), -FLT_MAX if ip else FLT_MAX, dtype=np.float32)
    J = np.full((nq, k, m), -1, dtype=np.int64)
    Z = np.zeros((nq, k), dtype=np.int64)
    ids = _members(keys, n_cov, mask)
    if nq == 0 or ids.shape[0] == 0:
        return Ko, F, U, J, Z
    code, key_of, _ = group_codes(keys)
    S = _sub_scores(xs, fq, ids, metric)
    codes, M, best, sizes = _group_best(S, ids, code[ids], ip)
    Fg = _sum_left_to_right(M)
    kk = min(k, int(codes.shape[0]))
    for a in range(nq):
        order = np.lexsort((codes, -Fg[a] if ip else Fg[a]))[:kk]
        Ko[a, :kk] = key_of[codes[order]]
        F[a, :kk] = Fg[a, order]
        U[a, :kk] = M[a][:, order].T.astype(np.float32)
        J[a, :kk] = best[a][:, order].T
        Z[a, :kk] = sizes[order]
    return Ko, F, U, J, Z


def resolve_depth(k: int, m: int, first: int = 0, limit: int = 0):
    """(first, limit) as a call with ``m`` sub-queries resolves ``set_maxsim_depth``'s settings."""
    klim = k_limit(m)
    lim = min(limit, klim) if limit > 0 else klim
    return min(first if first > 0 else max(4 * k, 64), lim), lim


def maxsim_need(xs, q3, k: int, metric: str, keys, first: int, limit: int, walk_rows: int = 0, tier: str = "auto",
                n_cov=None, mask=None):
    """What ``maxsim_last_stats`` must report -- {"first", "deeper", "scan", "longest", "tier"} -- and per query
    where it completed (0 first list, 1 deeper list, 2 scan), from the reference rankings alone: the lists are
    prefixes of each sub-query's ranking of the members, first, then 4x up to min(limit, members).  Complete
    iff the lists held every member, or there are k candidates and the k-th best candidate F is strictly better
    than U, the left-to-right sum of the score of list j's last entry under sub-query j.  Lists that do not hold
    every member and whose candidate groups' member lists hold more than ``walk_rows`` rows (0: the default,
    400 min(nq, 256)) send the query to the scan at once: deeper lists only add candidates; so does an open walk
    over more than a quarter of the cap, whose next lists are four times as long."""
    assert tier in ("auto", "lists", "scan")
    fq = _fq(q3)
    keys = np.asarray(keys, dtype=np.int64)
    nq, m, k, ip = int(fq.shape[0]), int(fq.shape[1]), int(k), metric == "ip"
    walk_rows = int(walk_rows) if walk_rows else WALK_ROWS_PER_QUERY * min(nq, WALK_ROWS_QUERIES)
    taken = "scan" if tier == "scan" else "lists"
    ids = _members(keys, n_cov, mask)
    members = int(ids.shape[0])
    if members == 0 or nq == 0:
        return {"first": nq, "deeper": 0, "scan": 0, "longest": 0, "tier": taken}, [0] * nq
    if taken == "scan":
        return {"first": 0, "deeper": 0, "scan": nq, "longest": 0, "tier": taken}, [2] * nq
    code, _, _ = group_codes(keys)
    cov = int(keys.shape[0] if n_cov is None else n_cov)
    list_rows = np.bincount(code[:cov], minlength=int(code.max()) + 1)  # (the member lists know no selector)
    S = _sub_scores(xs, fq, ids, metric)
    codes, M, _, _ = _group_best(S, ids, code[ids], ip)
    Fg = _sum_left_to_right(M)
    col = {int(c): i for i, c in enumerate(codes.tolist())}
    mcode = code[ids]
    orders = [[np.lexsort((ids, -S[a, j] if ip else S[a, j])) for j in range(m)] for a in range(nq)]

    def complete(a, L):
        if L >= members:
            return True
        cand = np.unique(np.concatenate([mcode[orders[a][j][:L]] for j in range(m)]))
        rows = int(list_rows[cand].sum())
        if rows > walk_rows:
            return None  # over the cap
        still_open = None if 4 * rows > walk_rows else False  # (lists four times as long: over the cap by that estimate)
        if cand.shape[0] < k:
            return still_open
        u = S[a, 0, orders[a][0][L - 1]]
        for j in range(1, m):
            u = u + S[a, j, orders[a][j][L - 1]]
        f = np.sort(Fg[a, [col[int(c)] for c in cand]])
        return (bool(f[-k] > u) if ip else bool(f[k - 1] < u)) or still_open

    where = [2] * nq
    Lmax = min(limit, members)
    L = min(first, Lmax)
    pending, done, t = list(range(nq)), [0, 0], 0
    while True:
        state = {a: complete(a, L) for a in pending}
        for a in pending:
            if state[a]:
                where[a] = t
                done[t] += 1
        pending, longest = [a for a in pending if state[a] is False], L  # (capped queries leave for the scan)
        if not pending or L >= Lmax:
            break
        L, t = min(4 * L, Lmax), 1
    return {"first": done[0], "deeper": done[1], "scan": where.count(2), "longest": longest, "tier": taken}, where


class OracleMaxSimFlatIndex(OracleAfterFlatIndex):
    def search_maxsim(self, q, k: int, groups, sel=None) -> MaxSimResult:
        q = _fq(q, self.d)
        if not 1 <= q.shape[1] <= FUSE_MAX_Q:
            raise ValueError(f"search_maxsim takes 1..{FUSE_MAX_Q} sub-queries per query, got {q.shape[1]}")
        if not 1 <= int(k) <= k_limit(q.shape[1]):
            raise RuntimeError(f"k must be in 1..{k_limit(q.shape[1])}")
        if groups.generation != self._generation or groups.rows > self.ntotal:
            raise RuntimeError("stale groups")
        return MaxSimResult(*maxsim_reference(self._x, q, int(k), "ip" if self.metric_type == 0 else "l2", groups.keys,
                                              mask=self._mask(sel)))


def oracle_maxsim_factory(dimension: int, metric: str):
    return OracleMaxSimFlatIndex(dimension, "ip" if metric == "cosine" else "l2")

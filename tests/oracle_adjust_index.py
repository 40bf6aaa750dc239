"""TEST INFRASTRUCTURE: the reference recipe the GPU tests hold ``vs_search_adjusted`` to, and an
``OracleAdjustFlatIndex`` with FlatIndex's ``score_adjust`` / ``score_adjust_sparse`` / ``search_adjusted``
surface so ``VectorStore.search_hybrid`` runs on the CPU.

Recipe (include/vs.h "adjusted search"): the members scored with the oracle's canonical fp64 score S,
``A = float64(scale) * S`` then ``+ float64(bias)`` (two numpy float64 operations: two roundings, no
FMA), ordered by a stable lexicographic sort on (A in the metric's direction, id).  ``adjust_reference``
knows nothing of lists or tiers.  ``adjust_need`` replays the contract's two certificates on the
reference's plain ranking and says, per query, in which list it completes or that the scan answers it."""
from __future__ import annotations

import numpy as np

from oracle import oracle as O
from oracle_group_index import OracleGroupFlatIndex
from oracle_sel_index import FLT_MAX
from photo_search_engine_amd.index import adjust_arrays, adjust_sparse_arrays

KMAX = 3276


def _members(n_cov: int, mask):
    member = np.ones((n_cov,), dtype=bool)
    if mask is not None:
        m = np.asarray(mask, dtype=bool)[:n_cov]
        member[: m.shape[0]] &= m
        member[m.shape[0]:] = False
    return np.flatnonzero(member).astype(np.int64)


def _adjusted(scale, bias, S, ids):
    """A of the member columns of S (nq x members), float64: a rounded multiply, then a rounded add."""
    A = scale[ids].astype(np.float64)[None, :] * S
    return A + bias[ids].astype(np.float64)[None, :]


def adjust_reference(xs, q, scale, bias, k: int, metric: str, mask=None):
    """(D float32 nq x k, I int64 nq x k, D_raw float32 nq x k) of ``search_adjusted(q, k, adjust)`` over
    rows ``xs`` (the values as stored); ``scale`` / ``bias`` float32, one per covered row (the first
    ``len(scale)`` rows); ``mask`` restricts the members."""
    q = np.ascontiguousarray(q, dtype=np.float32)
    scale = np.asarray(scale, dtype=np.float32)
    bias = np.asarray(bias, dtype=np.float32)
    nq, k, ip = int(q.shape[0]), int(k), metric == "ip"
    worst = -FLT_MAX if ip else FLT_MAX
    D = np.full((nq, k), worst, dtype=np.float32)
    I = np.full((nq, k), -1, dtype=np.int64)
    R = np.full((nq, k), worst, dtype=np.float32)
    ids = _members(scale.shape[0], mask)
    kk = min(k, int(ids.shape[0]))
    if nq == 0 or kk == 0:
        return D, I, R
    S = O.canon_scores(xs[ids], q, metric)
    A = _adjusted(scale, bias, S, ids)
    for qi in range(nq):
        order = np.lexsort((ids, -A[qi] if ip else A[qi]))[:kk]
        I[qi, :kk] = ids[order]
        D[qi, :kk] = A[qi, order].astype(np.float32)
        R[qi, :kk] = S[qi, order].astype(np.float32)
    return D, I, R


def plain_rows(scale, bias):
    scale = np.asarray(scale, dtype=np.float32)
    bias = np.asarray(bias, dtype=np.float32)
    return (scale == np.float32(1.0)) & (bias == np.float32(0.0))


def adjust_bound(S_L, scale, bias, metric: str):
    """The BOUND certificate's bound on A of every member whose plain score is no better than ``S_L``
    (extrema over all covered rows; float64, rounded multiply then add)."""
    smin, smax = np.float64(np.min(scale)), np.float64(np.max(scale))
    S_L = np.float64(S_L)
    if metric == "ip":
        b = np.float64(np.max(bias))
        return max(smax * S_L + b, smin * S_L + b)
    b = np.float64(np.min(bias))
    return min(smin * S_L + b, smax * S_L + b)


def resolve_depth(k: int, m_adj: int, first: int = 0, limit: int = 0):
    """(first, limit) as ``set_adjust_depth`` resolves them."""
    lim = limit if limit > 0 else KMAX
    return min(first if first > 0 else k + min(m_adj, max(k, 64)), lim), lim


def adjust_need(xs, q, scale, bias, k: int, metric: str, first: int, limit: int, mode: str = "auto", mask=None):
    """What ``adjust_last_stats`` must report -- {"first", "deeper", "scan", "longest", "tier"} -- and
    per query where it completed (0 first list, 1 deeper list, 2 scan), from the reference ranking alone:
    the lists are prefixes of the members' plain ranking (first, then 4x up to min(limit, members))."""
    q = np.ascontiguousarray(q, dtype=np.float32)
    scale = np.asarray(scale, dtype=np.float32)
    bias = np.asarray(bias, dtype=np.float32)
    nq, k, ip = int(q.shape[0]), int(k), metric == "ip"
    plain = plain_rows(scale, bias)
    m_adj = int((~plain).sum())
    tier = mode if mode != "auto" else ("direct" if m_adj + k <= limit else "bound")
    assert not (tier == "direct" and m_adj + k > limit), "forced DIRECT beyond the limit is an argument error"
    ids = _members(scale.shape[0], mask)
    members = int(ids.shape[0])
    if members == 0 or nq == 0:
        return {"first": nq, "deeper": 0, "scan": 0, "longest": 0, "tier": tier}, [0] * nq
    if tier == "scan" or (tier == "bound" and limit < min(k, members)):
        return {"first": 0, "deeper": 0, "scan": nq, "longest": 0, "tier": tier}, [2] * nq
    S = O.canon_scores(xs[ids], q, metric)
    A = _adjusted(scale, bias, S, ids)
    orders = [np.lexsort((ids, -S[qi] if ip else S[qi])) for qi in range(nq)]

    def complete(qi, L):
        if L >= members:
            return True
        head = orders[qi][:L]
        if tier == "direct":
            return int(plain[ids[head]].sum()) >= k
        if L < k:
            return False
        a = np.sort(A[qi, head])
        bound = adjust_bound(S[qi, head[-1]], scale, bias, metric)
        return bool(a[-k] > bound) if ip else bool(a[k - 1] < bound)

    where = [2] * nq
    L, Lmax = min(first, limit, members), min(limit, members)
    pending, done, t = list(range(nq)), [0, 0], 0
    while True:
        left = [qi for qi in pending if not complete(qi, L)]
        for qi in set(pending) - set(left):
            where[qi] = t
        done[t] += len(pending) - len(left)
        pending, longest = left, L
        if not pending or L >= Lmax:
            break
        L, t = min(4 * L, Lmax), 1
    return {"first": done[0], "deeper": done[1], "scan": len(pending), "longest": longest, "tier": tier}, where


class OracleAdjust:
    def __init__(self, index, scale, bias) -> None:
        for name, a in (("scale", scale), ("bias", bias)):
            if not np.all(np.isfinite(a)):
                raise RuntimeError(f"{name} must be finite")
        if np.any(scale < 0):
            raise RuntimeError("scale must be >= 0")
        self.scale, self.bias = scale, bias
        self.generation = index._generation

    @property
    def count(self) -> int:
        return int((~plain_rows(self.scale, self.bias)).sum())

    @property
    def rows(self) -> int:
        return int(self.scale.shape[0])

    def close(self) -> None:
        pass


class OracleAdjustFlatIndex(OracleGroupFlatIndex):
    def score_adjust(self, scale=None, bias=None) -> OracleAdjust:
        n = self.ntotal
        scale, bias = adjust_arrays(n, scale, bias)
        return OracleAdjust(self, np.ones((n,), np.float32) if scale is None else scale,
                            np.zeros((n,), np.float32) if bias is None else bias)

    def score_adjust_sparse(self, ids, scale=None, bias=None) -> OracleAdjust:
        n = self.ntotal
        ids, scale, bias = adjust_sparse_arrays(ids, scale, bias)
        if ids.size and (int(ids.min()) < 0 or int(ids.max()) >= n or np.unique(ids).shape[0] != ids.shape[0]):
            raise RuntimeError("adjustment ids must be distinct and in range")
        s, b = np.ones((n,), np.float32), np.zeros((n,), np.float32)
        if scale is not None:
            s[ids] = scale
        if bias is not None:
            b[ids] = bias
        return OracleAdjust(self, s, b)

    def search_adjusted(self, q, k: int, adjust, sel=None, return_raw: bool = False):
        q = np.ascontiguousarray(q, dtype=np.float32)
        if q.ndim != 2 or q.shape[1] != self.d:
            raise ValueError(f"search_adjusted expects an (nq, {self.d}) array, got {q.shape}")
        if not 1 <= int(k) <= KMAX:
            raise RuntimeError("k must be in 1..3276")
        if adjust.generation != self._generation or adjust.rows > self.ntotal:
            raise RuntimeError("stale adjustment")
        D, I, R = adjust_reference(self._x, q, adjust.scale, adjust.bias, int(k), "ip" if self.metric_type == 0 else "l2",
                                   self._mask(sel))
        return (D, I, R) if return_raw else (D, I)


def oracle_adjust_factory(dimension: int, metric: str):
    return OracleAdjustFlatIndex(dimension, "ip" if metric == "cosine" else "l2")


# ---- the adjustment schemes of the burst corpus (tests/test_gpu_adjust.py, tests/test_adjust_host.py) ----
SCHEMES = ["none", "sparse", "flood", "dense_narrow", "dense_wide", "ties", "mixed_scale"]


def plain_ranks(S, metric: str):
    """rank[q, row] (0 = best) of every row in ``vs_search``'s total order, from its scores S (nq x n)."""
    n = S.shape[1]
    ids = np.arange(n, dtype=np.int64)
    rank = np.empty(S.shape, dtype=np.int64)
    for qi in range(S.shape[0]):
        rank[qi, np.lexsort((ids, -S[qi] if metric == "ip" else S[qi]))] = ids
    return rank


def far_rows(S, metric: str, count: int = 6):
    """The ``count`` rows whose best rank over the queries is the worst: far from the top of every list."""
    best = plain_ranks(S, metric).min(axis=0)
    return np.sort(np.lexsort((np.arange(best.shape[0]), -best))[:count])


def burst_scheme(name: str, S, metric: str):
    """(scale, bias) float32, one per row, of a scheme over a corpus whose canonical plain scores for the
    test's queries are S (nq x n).  A bonus is a positive bias for the inner product, a negative one for
    L2; ``lift`` is more than the whole spread of S, so a lifted row beats every row that is not."""
    n = S.shape[1]
    rng = np.random.default_rng(11)
    sgn = 1.0 if metric == "ip" else -1.0
    spread = float(S.max() - S.min())
    lift = sgn * (spread + 0.25)
    scale, bias = np.ones((n,), np.float64), np.zeros((n,), np.float64)
    rank = plain_ranks(S, metric)
    if name == "none":
        pass
    elif name == "sparse":
        # 12 rows: the 6 farthest from the top of every query's ranking, lifted above every plain row (in
        # distinct steps), and 6 others, rescaled with a small bonus
        far = far_rows(S, metric)
        others = np.setdiff1d(np.arange(3, n, 41), far)[:6]
        assert far.shape[0] == 6 and others.shape[0] == 6
        bias[far] = lift + sgn * 0.01 * np.arange(6)
        scale[others] = 0.5
        bias[others] = sgn * 0.05 * np.arange(1, 7)
    elif name == "flood":
        # 60 rows above every plain row: the 16 best of queries 0, 1 and 2 (their first lists of 16 then
        # hold no plain row at all), filled up with the best of query 3
        rows = []
        for qi in (0, 1, 2):
            rows += np.flatnonzero(rank[qi] < 16).tolist()
        for r in np.argsort(rank[3], kind="stable").tolist():
            if len(set(rows)) >= 60:
                break
            rows.append(r)
        rows = np.asarray(sorted(set(rows)), dtype=np.int64)
        assert rows.shape[0] == 60
        bias[rows] = lift
    elif name == "dense_narrow":
        bias[:] = sgn * rng.uniform(0.0, 0.02, n)
    elif name == "dense_wide":
        bias[:] = sgn * rng.uniform(0.0, 2.0 * spread, n)
    elif name == "ties":
        rows = np.arange(5, n, 6)[:40]
        scale[rows] = 0.0
        bias[rows] = (float(S.max()) + 1.0) if metric == "ip" else (float(S.min()) - 1.0)
    elif name == "mixed_scale":
        scale[:] = rng.uniform(0.5, 2.0, n)
    else:
        raise ValueError(name)
    return scale.astype(np.float32), bias.astype(np.float32)


# ---- VectorStore.search_hybrid: the fusion over all rows, in explicit loops ---------------------------
def hybrid_reference(xs, query, paths, keyword_scores, boost_of_row, wv: float, wk: float, k: int, allowed=None):
    """``[(row, score, vector_score, keyword_score)]``, best first: every row's cosine D (canonical fp64),
    its fused A = fl(fl(scale D) + bias) with (scale, bias) the fp32 roundings of the formula's two
    coefficients, ranked by (A descending, row ascending), the first ``k``."""
    D = O.canon_scores(xs, np.ascontiguousarray(query, dtype=np.float32).reshape(1, -1), "ip")[0]
    fused = []
    for row, path in enumerate(paths):
        if allowed is not None and not allowed[row]:
            continue
        ks = keyword_scores.get(path)
        boost = float(boost_of_row(row))
        if ks is None:  # A = b D + (b - 1)
            s, b = boost, boost - 1.0
        else:  # A = b (wv D + wk (2 ks - 1)) + (b - 1)
            s, b = boost * wv, boost * wk * (2.0 * float(ks) - 1.0) + (boost - 1.0)
        A = np.float64(np.float32(s)) * np.float64(D[row])
        A = A + np.float64(np.float32(b))
        fused.append((-A, row, A, ks))
    fused.sort(key=lambda t: (t[0], t[1]))
    return [(row, (float(np.float32(A)) + 1.0) / 2.0, (float(np.float32(D[row])) + 1.0) / 2.0,
             None if ks is None else float(ks)) for _, row, A, ks in fused[:k]]

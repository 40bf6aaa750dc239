"""TEST INFRASTRUCTURE: the reference recipe the GPU tests hold ``vs_search_fused`` to, and an
``OracleFuseFlatIndex`` with FlatIndex's ``search_fused`` surface so ``VectorStore.search_any`` /
``search_all`` run on the CPU.

Recipe (include/vs.h "fused search"): the members scored with the oracle's canonical fp64 score against
every sub-query, ``F`` = the best (ANY) or the worst (ALL) of a row's scores -- ``max`` / ``min`` along the
sub-query axis, no arithmetic -- ordered by a stable lexicographic sort on (F in the metric's direction,
id); ``which`` is the first ``argmax`` / ``argmin``.  ``fuse_reference`` knows nothing of lists or tiers.
``fuse_need`` replays the contract's certificate on prefixes of the sub-queries' reference rankings and
says, per fused query, in which list it completes or that the scan answers it."""
from __future__ import annotations

import numpy as np

from oracle import oracle as O
from oracle_adjust_index import OracleAdjustFlatIndex
from oracle_sel_index import FLT_MAX

KMAX = 3276
FUSE_MAX_Q = 8
FUSE_WALK_MAX = 8192
MODES = ("any", "all")


def k_limit(m: int) -> int:
    return min(KMAX, FUSE_WALK_MAX // int(m))


def _fq(fq, d=None):
    fq = np.ascontiguousarray(fq, dtype=np.float32)
    if fq.ndim != 3 or (d is not None and fq.shape[2] != d):
        raise ValueError(f"fused queries are (nq, m, d), got {fq.shape}")
    return fq


def _member_ids(n: int, mask):
    if mask is None:
        return np.arange(n, dtype=np.int64)
    m = np.zeros((n,), dtype=bool)
    mk = np.asarray(mask, dtype=bool)[:n]
    m[: mk.shape[0]] = mk
    return np.flatnonzero(m).astype(np.int64)


def _sub_scores(xs, fq, ids, metric: str):
    """S[a, j, c]: the canonical fp64 score of member column c with sub-query j of fused query a."""
    nq, m, d = fq.shape
    S = O.canon_scores(xs[ids], fq.reshape(nq * m, d), metric)
    return np.asarray(S, dtype=np.float64).reshape(nq, m, ids.shape[0])


def _fuse(S, metric: str, mode: str):
    """(F, which) along the sub-query axis of S (..., m, members)."""
    best_is_max = metric == "ip"
    take_max = best_is_max if mode == "any" else not best_is_max
    F = S.max(axis=-2) if take_max else S.min(axis=-2)
    W = S.argmax(axis=-2) if take_max else S.argmin(axis=-2)  # (the first index at the extreme)
    return F, W


def fuse_reference(xs, fq, k: int, metric: str, mode: str, mask=None):
    """(D float32 nq x k, I int64 nq x k, which int32 nq x k, D_sub float32 nq x k x m) of
    ``search_fused(fq, k, mode)`` over rows ``xs`` (the values as stored); ``mask`` restricts the members."""
    assert mode in MODES
    fq = _fq(fq)
    nq, m, k, ip = int(fq.shape[0]), int(fq.shape[1]), int(k), metric == "ip"
    worst = -FLT_MAX if ip else FLT_MAX
    D = np.full((nq, k), worst, dtype=np.float32)
    I = np.full((nq, k), -1, dtype=np.int64)
    W = np.full((nq, k), -1, dtype=np.int32)
    U = np.full((nq, k, m), worst, dtype=np.float32)
    ids = _member_ids(xs.shape[0], mask)
    kk = min(k, int(ids.shape[0]))
    if nq == 0 or kk == 0:
        return D, I, W, U
    S = _sub_scores(xs, fq, ids, metric)
    F, Wh = _fuse(S, metric, mode)
    for a in range(nq):
        order = np.lexsort((ids, -F[a] if ip else F[a]))[:kk]
        I[a, :kk] = ids[order]
        D[a, :kk] = F[a, order].astype(np.float32)
        W[a, :kk] = Wh[a, order]
        U[a, :kk] = S[a][:, order].T.astype(np.float32)
    return D, I, W, U


def resolve_depth(k: int, m: int, first: int = 0, limit: int = 0):
    """(first, limit) as a call with ``m`` sub-queries resolves ``set_fuse_depth``'s settings."""
    klim = k_limit(m)
    lim = min(limit, klim) if limit > 0 else klim
    return min(first if first > 0 else max(4 * k, 64), lim), lim


def fuse_need(xs, fq, k: int, metric: str, mode: str, first: int, limit: int, tier: str = "auto", mask=None):
    """What ``fuse_last_stats`` must report -- {"first", "deeper", "scan", "longest", "tier"} -- and per
    fused query where it completed (0 first list, 1 deeper list, 2 scan), from the reference rankings alone:
    the lists are prefixes of each sub-query's ranking of the members.  ANY: one list of min(k, members).
    ALL: first, then 4x up to min(limit, members); complete iff the lists held every member, or there are
    k candidates and the k-th best candidate F is strictly better than U, the worst over j of the score of
    list j's last entry under sub-query j."""
    assert mode in MODES and tier in ("auto", "lists", "scan")
    fq = _fq(fq)
    nq, m, k, ip = int(fq.shape[0]), int(fq.shape[1]), int(k), metric == "ip"
    taken = "scan" if tier == "scan" else "lists"
    ids = _member_ids(xs.shape[0], mask)
    members = int(ids.shape[0])
    if members == 0 or nq == 0:
        return {"first": nq, "deeper": 0, "scan": 0, "longest": 0, "tier": taken}, [0] * nq
    if taken == "scan":
        return {"first": 0, "deeper": 0, "scan": nq, "longest": 0, "tier": taken}, [2] * nq
    if mode == "any":
        return {"first": nq, "deeper": 0, "scan": 0, "longest": min(k, members), "tier": taken}, [0] * nq
    S = _sub_scores(xs, fq, ids, metric)
    F, _ = _fuse(S, metric, mode)
    orders = [[np.lexsort((ids, -S[a, j] if ip else S[a, j])) for j in range(m)] for a in range(nq)]

    def complete(a, L):
        if L >= members:
            return True
        cand = np.unique(np.concatenate([orders[a][j][:L] for j in range(m)]))
        if cand.shape[0] < k:
            return False
        last = np.array([S[a, j, orders[a][j][L - 1]] for j in range(m)])
        f = np.sort(F[a, cand])
        return bool(f[-k] > last.min()) if ip else bool(f[k - 1] < last.max())

    where = [2] * nq
    Lmax = min(limit, members)
    L = min(first, Lmax)
    pending, done, t = list(range(nq)), [0, 0], 0
    while True:
        left = [a for a in pending if not complete(a, L)]
        for a in set(pending) - set(left):
            where[a] = t
        done[t] += len(pending) - len(left)
        pending, longest = left, L
        if not pending or L >= Lmax:
            break
        L, t = min(4 * L, Lmax), 1
    return {"first": done[0], "deeper": done[1], "scan": len(pending), "longest": longest, "tier": taken}, where


class OracleFuseFlatIndex(OracleAdjustFlatIndex):
    def search_fused(self, q, k: int, mode: str = "any", sel=None, return_sub: bool = False):
        q = _fq(q, self.d)
        if mode not in MODES:
            raise ValueError(f"fuse mode must be one of {sorted(MODES)}")
        if not 1 <= q.shape[1] <= FUSE_MAX_Q:
            raise ValueError(f"search_fused takes 1..{FUSE_MAX_Q} sub-queries per fused query, got {q.shape[1]}")
        if not 1 <= int(k) <= k_limit(q.shape[1]):
            raise RuntimeError(f"k must be in 1..{k_limit(q.shape[1])}")
        D, I, W, U = fuse_reference(self._x, q, int(k), "ip" if self.metric_type == 0 else "l2", mode, self._mask(sel))
        return (D, I, W, U) if return_sub else (D, I, W)


def oracle_fuse_factory(dimension: int, metric: str):
    return OracleFuseFlatIndex(dimension, "ip" if metric == "cosine" else "l2")


# ---- the fused queries of the burst corpus (tests/test_gpu_fuse.py, tests/test_fuse_host.py) -------------
FAMILIES = ["near3", "pair", "oppo", "eight"]


def _unit(v):
    return v / np.linalg.norm(v)


def burst_families(q):
    """{family: fused queries (nq, m, d) float32, read-only} from the burst corpus' 8 queries:
    ``near3`` three noisy copies of q[i] (``unit(q[i] + 0.15 N(0, 1))``, drawn first, i ascending, from
    ``default_rng(23)``), ``pair`` (q[i], q[i + 1]), ``oppo`` (q[i], -q[i]), ``eight`` all 8 rolled by i."""
    q = np.asarray(q, dtype=np.float32)
    nq, d = q.shape
    rng = np.random.default_rng(23)
    near3 = np.empty((nq, 3, d), dtype=np.float32)
    for i in range(nq):
        for j in range(3):
            near3[i, j] = _unit(q[i].astype(np.float64) + 0.15 * rng.standard_normal(d)).astype(np.float32)
    out = {
        "near3": near3,
        "pair": np.stack([np.stack([q[i], q[(i + 1) % nq]]) for i in range(nq)]),
        "oppo": np.stack([np.stack([q[i], -q[i]]) for i in range(nq)]),
        "eight": np.stack([np.roll(q, -i, axis=0) for i in range(2)]),
    }
    out = {name: np.ascontiguousarray(a, dtype=np.float32) for name, a in out.items()}
    for a in out.values():
        a.setflags(write=False)
    return out


def burst_depths(k: int):
    return [(0, 0), (16, 64), (k, k)]


def tier_reach(need, q_families, ks=(1, 10, 100)):
    """The destinations ALL reaches on the burst corpus, as the issue's table states them; ``need(name, fq,
    k, depth)`` returns ``fuse_need``'s (stats, where) for ALL under AUTO.  Asserts every row of the table."""
    def where(name, k, depth):
        return need(name, q_families[name], k, depth)[1]

    for k in ks:  # first list: near3 at the default depth
        assert where("near3", k, (0, 0)) == [0] * 8, ("near3 default", k)
    assert where("near3", 10, (16, 64)).count(1) == 4  # deeper list
    assert where("pair", 1, (16, 64)).count(1) == 4
    for k in (1, 10):
        assert where("oppo", k, (0, 0)) == [1] * 8, ("oppo default", k)
    for name in FAMILIES:  # scan: every family under (k, k); oppo under (16, 64)
        for k in ks:
            w = where(name, k, (k, k))
            assert w == [2] * len(w), (name, k, "(k, k)")
    for k in ks:
        assert where("oppo", k, (16, 64)) == [2] * 8, ("oppo (16, 64)", k)

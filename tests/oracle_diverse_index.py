"""TEST INFRASTRUCTURE: the reference recipe the GPU tests hold ``vs_search_diverse`` to, written as
plain loops, and an ``OracleDiverseFlatIndex`` with FlatIndex's ``search_diverse`` surface so
``VectorStore.search_diverse`` runs on the CPU.

Recipe (include/vs.h "diversified search"): the members ranked by the oracle's canonical fp64 score,
ties to the lower id; walked best first; a row is accepted iff the fp32 value of its canonical score
with every row accepted before it does not pass the radius strictly (``> r`` inner product, ``< r``
squared L2), otherwise it is hidden under the earliest-accepted row it is near; the walk ends with the
k-th acceptance or with the ranking.  It knows nothing of lists or tiers."""
from __future__ import annotations

import numpy as np

from oracle import oracle as O
from oracle_rows_index import OracleRowsFlatIndex
from oracle_sel_index import FLT_MAX
from photo_search_engine_amd.index import DiverseResult, range_radius


def diverse_reference(xs, q, k: int, radius, metric: str, mask=None):
    """(D float32 nq x k, I int64 nq x k, hidden int32 nq x k, examined int64 nq) of
    ``search_diverse(q, k, radius)`` over rows ``xs`` (the values as stored); ``mask`` restricts the
    members."""
    q = np.ascontiguousarray(q, dtype=np.float32)
    nq, n, k = int(q.shape[0]), int(xs.shape[0]), int(k)
    r = range_radius(radius, nq)
    ip = metric == "ip"
    D = np.full((nq, k), -FLT_MAX if ip else FLT_MAX, dtype=np.float32)
    I = np.full((nq, k), -1, dtype=np.int64)
    hidden = np.zeros((nq, k), dtype=np.int32)
    examined = np.zeros((nq,), dtype=np.int64)
    ids = np.arange(n, dtype=np.int64) if mask is None else np.flatnonzero(np.asarray(mask, dtype=bool)).astype(np.int64)
    if nq == 0 or ids.shape[0] == 0:
        return D, I, hidden, examined
    S = O.canon_scores(xs[ids], q, metric)  # (nq, members) fp64
    for qi in range(nq):
        order = np.lexsort((ids, -S[qi] if ip else S[qi]))
        accepted = []
        for pos in order.tolist():
            c = int(ids[pos])
            examined[qi] += 1
            under = -1
            if accepted:
                pair = O.canon_scores(xs[accepted], xs[[c]], metric).astype(np.float32)[0]
                near = pair > r[qi] if ip else pair < r[qi]
                for j in range(len(accepted)):
                    if near[j]:
                        under = j
                        break
            if under >= 0:
                hidden[qi, under] += 1
                continue
            I[qi, len(accepted)] = c
            D[qi, len(accepted)] = np.float32(S[qi, pos])
            accepted.append(c)
            if len(accepted) == k:
                break
    return D, I, hidden, examined


class OracleDiverseFlatIndex(OracleRowsFlatIndex):
    def search_diverse(self, q, k: int, radius, sel=None) -> DiverseResult:
        q = np.ascontiguousarray(q, dtype=np.float32)
        if q.ndim != 2 or q.shape[1] != self.d:
            raise ValueError(f"search_diverse expects an (nq, {self.d}) array, got {q.shape}")
        if k <= 0:
            raise RuntimeError("k must be > 0")
        return DiverseResult(*diverse_reference(self._x, q, int(k), radius, "ip" if self.metric_type == 0 else "l2",
                                                self._mask(sel)))


def oracle_diverse_factory(dimension: int, metric: str):
    return OracleDiverseFlatIndex(dimension, "ip" if metric == "cosine" else "l2")


def burst_corpus(d: int = 72, nbase: int = 40, nq: int = 8, seed: int = 7):
    """The burst corpus of the GPU tests: ``nbase`` base vectors, burst ``b`` of ``1 + (5 b) % 12``
    members ``base[b] + 0.05 noise``, shuffled, unit-normalised (256 rows for 40 bases); ``nq`` queries
    ``base[:nq] + 0.3 noise``, normalised.  Returns (x, q), read-only."""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((nbase, d))
    rows = []
    for b in range(nbase):
        for _ in range(1 + (5 * b) % 12):
            rows.append(base[b] + 0.05 * rng.standard_normal(d))
    x = np.asarray(rows)
    rng.shuffle(x)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    q = base[:nq] + 0.3 * rng.standard_normal((nq, d))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    x = np.ascontiguousarray(x, dtype=np.float32)
    q = np.ascontiguousarray(q, dtype=np.float32)
    x.setflags(write=False)
    q.setflags(write=False)
    return x, q


def staged_chunk(L: int, d: int) -> int:
    """Queries of one staged chunk of a search at list depth ``L`` without a selector: 8 MiB of pinned
    staging, per query the larger of its fp32 row and its list (int64 id + fp32 score per entry, one
    certificate); from 256 queries on, whole batches of 256."""
    chunk = max(1, (8 << 20) // max(4 * d, 12 * L + 4))
    return chunk // 256 * 256 if chunk >= 256 else chunk

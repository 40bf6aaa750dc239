"""TEST INFRASTRUCTURE: the reference recipe the GPU tests hold ``vs_range_search`` to, and an
``OracleRangeFlatIndex`` with FlatIndex's ``range_search`` surface so ``VectorStore.search_range`` runs
on the CPU.  Recipe: the oracle's canonical fp64 scores ``S`` of the stored (dtype-rounded) rows;
members are the rows whose fp32 value ``S.astype(float32)`` passes the radius strictly (``> r`` inner
product, ``< r`` squared L2), restricted to the mask; each query's members ordered by (S, then id)."""
from __future__ import annotations

import numpy as np

from oracle import oracle as O
from oracle_sel_index import OracleSelector, OracleSelFlatIndex
from photo_search_engine_amd.index import range_radius


def range_reference(xs, q, radius, metric: str, mask=None):
    """(lims int64 nq + 1, D float32, I int64) of the range search of ``q`` over rows ``xs`` (the values
    as stored); ``radius`` a scalar or nq values; ``mask`` restricts the rows."""
    q = np.ascontiguousarray(q, dtype=np.float32)
    nq, n = int(q.shape[0]), int(xs.shape[0])
    r = range_radius(radius, nq)
    lims = np.zeros((nq + 1,), dtype=np.int64)
    Ds, Is = [], []
    if n and nq:
        S = O.canon_scores(xs, q, metric)  # (nq, n) fp64
        D = S.astype(np.float32)
        for i in range(nq):
            member = D[i] > r[i] if metric == "ip" else D[i] < r[i]
            if mask is not None:
                member = member & np.asarray(mask, dtype=bool)
            ids = np.flatnonzero(member)
            key = -S[i, ids] if metric == "ip" else S[i, ids]
            ids = ids[np.lexsort((ids, key))]  # by score, ties to the lower id
            lims[i + 1] = lims[i] + ids.shape[0]
            Ds.append(D[i, ids])
            Is.append(ids.astype(np.int64))
    D = np.concatenate(Ds).astype(np.float32) if Ds else np.empty((0,), dtype=np.float32)
    I = np.concatenate(Is).astype(np.int64) if Is else np.empty((0,), dtype=np.int64)
    return lims, D, I


class OracleRangeFlatIndex(OracleSelFlatIndex):
    def range_search(self, q, radius, sel=None, max_total=None):
        q = np.ascontiguousarray(q, dtype=np.float32)
        if q.ndim != 2 or q.shape[1] != self.d:
            raise ValueError(f"range_search expects an (nq, {self.d}) array, got {q.shape}")
        mask = None
        if sel is not None:
            s = sel if isinstance(sel, OracleSelector) else OracleSelector(self, sel)
            if s.generation != self._generation:
                raise RuntimeError("stale selector")
            mask = np.zeros((self.ntotal,), dtype=bool)  # rows added after the selector are not selected
            mask[: s.n] = s.mask
        lims, D, I = range_reference(self._x, q, radius, "ip" if self.metric_type == 0 else "l2", mask)
        if max_total is not None and int(lims[-1]) > int(max_total):
            raise RuntimeError(f"range search found {int(lims[-1])} results, max_total is {int(max_total)}")
        return lims, D, I


def oracle_range_factory(dimension: int, metric: str):
    return OracleRangeFlatIndex(dimension, "ip" if metric == "cosine" else "l2")

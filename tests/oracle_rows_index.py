"""TEST INFRASTRUCTURE: the reference recipes the GPU tests hold ``vs_search_rows`` and
``vs_range_search_rows`` to, and an ``OracleRowsFlatIndex`` with FlatIndex's ``search_rows`` /
``range_search_rows`` surface so ``VectorStore.search_similar`` / ``duplicate_pairs`` /
``find_duplicates`` run on the CPU.

Query ``i`` is the stored value of row ``ids[i]`` (``xs[ids[i]]``, the rows as stored).  Top-k: the
oracle's exact search (``O.knn_exact``, or the filtered recipe with a mask) at ``min(k + 1, n)``, the
entry whose id is ``ids[i]`` dropped by id -- when it is not there, the last entry -- padded to ``k``.
Range: ``range_reference`` of those queries with, per query, the row itself (drop) or every row at or
below it (above) left out."""
from __future__ import annotations

import numpy as np

from oracle import oracle as O
from oracle_range_index import OracleRangeFlatIndex, range_reference
from oracle_sel_index import FLT_MAX, OracleSelector, filtered_reference
from photo_search_engine_amd.index import range_radius

SELF_MODES = ("keep", "drop", "above")


def _check_ids(ids, n: int) -> np.ndarray:
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    if ids.size and (int(ids.min()) < 0 or int(ids.max()) >= n):
        raise RuntimeError(f"row ids must lie in [0, {n})")
    return ids


def rows_topk_reference(xs, ids, k: int, metric: str, mask=None, drop_self: bool = True):
    """(D float32 n x k, I int64 n x k) of ``search_rows(ids, k)`` over rows ``xs`` (values as stored)."""
    n = int(xs.shape[0])
    ids = _check_ids(ids, n)
    k = int(k)
    worst = -FLT_MAX if metric == "ip" else FLT_MAX
    D = np.full((ids.shape[0], k), worst, dtype=np.float32)
    I = np.full((ids.shape[0], k), -1, dtype=np.int64)
    if ids.shape[0] == 0:
        return D, I
    kk = min(k + 1 if drop_self else k, n)
    q = np.ascontiguousarray(xs[ids], dtype=np.float32)
    if mask is None:
        S, Ik = O.knn_exact(xs, q, kk, metric)
        Dk = S.astype(np.float32)
    else:
        Dk, Ik = filtered_reference(xs, q, np.asarray(mask, dtype=bool), kk, metric)
    for i in range(ids.shape[0]):
        row_I, row_D = Ik[i], Dk[i]
        if drop_self:
            keep = row_I != ids[i]
            if keep.all():
                keep[-1] = kk <= k  # not there: the last entry goes, unless the list is shorter than k + 1
            row_I, row_D = row_I[keep], row_D[keep]
        m = min(k, row_I.shape[0])
        I[i, :m] = row_I[:m]
        D[i, :m] = row_D[:m]
    D[I < 0] = worst
    return D, I


def rows_range_reference(xs, ids, radius, metric: str, mask=None, self_mode: str = "above", keep=None):
    """(lims, D, I) of ``range_search_rows(radius, ids)`` over rows ``xs``; ``ids=None`` = every row.
    ``range_reference`` of the rows as queries, each query's list then without the rows its self mask
    excludes (masking a member out and leaving it out of the ordered list are the same thing: the
    order is total).  ``keep``: that unmasked ``range_reference`` result, when the caller has it."""
    assert self_mode in SELF_MODES
    n = int(xs.shape[0])
    ids = np.arange(n, dtype=np.int64) if ids is None else _check_ids(ids, n)
    r = range_radius(radius, ids.shape[0])
    if keep is None:
        keep = range_reference(xs, np.ascontiguousarray(xs[ids], dtype=np.float32), r, metric, mask)
    lims0, D0, I0 = keep
    if self_mode == "keep":
        return lims0.copy(), D0.copy(), I0.copy()
    lims = np.zeros((ids.shape[0] + 1,), dtype=np.int64)
    Ds, Is = [], []
    for i, row in enumerate(ids.tolist()):
        D, I = D0[lims0[i]:lims0[i + 1]], I0[lims0[i]:lims0[i + 1]]
        ok = I != row if self_mode == "drop" else I > row
        lims[i + 1] = lims[i] + int(ok.sum())
        Ds.append(D[ok])
        Is.append(I[ok])
    D = np.concatenate(Ds).astype(np.float32) if Ds else np.empty((0,), dtype=np.float32)
    I = np.concatenate(Is).astype(np.int64) if Is else np.empty((0,), dtype=np.int64)
    return lims, D, I


class OracleRowsFlatIndex(OracleRangeFlatIndex):
    def _mask(self, sel):
        if sel is None:
            return None
        s = sel if isinstance(sel, OracleSelector) else OracleSelector(self, sel)
        if s.generation != self._generation:
            raise RuntimeError("stale selector")
        mask = np.zeros((self.ntotal,), dtype=bool)  # rows added after the selector are not selected
        mask[: s.n] = s.mask
        return mask

    def search_rows(self, ids, k: int, sel=None, drop_self: bool = True):
        if k <= 0:
            raise RuntimeError("k must be > 0")
        return rows_topk_reference(self._x, ids, int(k), "ip" if self.metric_type == 0 else "l2", self._mask(sel),
                                   drop_self)

    def range_search_rows(self, radius, ids=None, sel=None, self_mode: str = "above", max_total=None):
        if self_mode not in SELF_MODES:
            raise ValueError(f"unknown self_mode {self_mode!r}")
        lims, D, I = rows_range_reference(self._x, ids, radius, "ip" if self.metric_type == 0 else "l2",
                                          self._mask(sel), self_mode)
        if max_total is not None and int(lims[-1]) > int(max_total):
            raise RuntimeError(f"range search found {int(lims[-1])} results, max_total is {int(max_total)}")
        return lims, D, I


def oracle_rows_factory(dimension: int, metric: str):
    return OracleRowsFlatIndex(dimension, "ip" if metric == "cosine" else "l2")

"""TEST INFRASTRUCTURE: the recipe the GPU tests hold ``vs_kmeans`` to, and an ``OracleKMeansFlatIndex``
with FlatIndex's ``kmeans`` / ``assign_rows`` surface so ``VectorStore.cluster_items`` and
``IVFFlatIndex.train_from``'s host logic run on the CPU.

Members are rows ``xs[ids]`` (``xs``: the values as stored, ``O.round_dtype``; ``ids`` ascending).
Assignment is the oracle's exact top-1 of each member over the centroids (``O.knn_exact``: canonical
fp64 score, ties to the lower centroid id).  The update is include/vs.h's segment rule, written as
explicit loops over the members: a cluster's members in ascending id in segments of ``SEG``, a
segment's partial from +0.0 adding one member after the other in fp64, the cluster's sum from +0.0
adding the partials in order, ``(float)(sum / count)`` per column; only the ``+=`` over the ``d``
columns is vectorised (``np.sum`` sums pairwise and is not used).  Empty clusters keep their centroid.
Stopping: pass ``t >= 1`` with no changed label, or pass ``t == niter``."""
from __future__ import annotations

import numpy as np

from oracle import oracle as O
from oracle_rows_index import OracleRowsFlatIndex
from photo_search_engine_amd import index as idxmod

SEG = 256  # VS_KMEANS_SEG


def segment_mean_update(rows: np.ndarray, labels: np.ndarray, centroids: np.ndarray) -> np.ndarray:
    """The centroids after one update: ``rows`` (m, d) fp32 members in ascending id, ``labels`` (m,)."""
    out = np.array(centroids, dtype=np.float32, copy=True)
    d = rows.shape[1]
    for c in range(out.shape[0]):
        members = np.flatnonzero(labels == c)
        if members.shape[0] == 0:
            continue
        total = np.zeros((d,), dtype=np.float64)
        for s0 in range(0, members.shape[0], SEG):
            part = np.zeros((d,), dtype=np.float64)
            for i in members[s0:s0 + SEG]:
                part += rows[i].astype(np.float64)
            total += part
        out[c] = (total / np.float64(members.shape[0])).astype(np.float32)
    return out


def assign_reference(rows: np.ndarray, centroids: np.ndarray, metric: str):
    """(labels int64 (m,), S float64 (m,)) of the members against fp32 centroids."""
    S, I = O.knn_exact(np.ascontiguousarray(centroids, dtype=np.float32), rows, 1, metric)
    return I[:, 0].astype(np.int64), S[:, 0]


def kmeans_reference(xs, ids, init, niter: int, metric: str) -> dict:
    """The whole call: ``centroids``, ``labels``, ``D`` (fp32), ``S`` (fp64), ``counts``, ``objective``,
    ``changed`` (one entry per pass run), ``abs_sums`` (the sum of ``|S|`` per pass: the scale of the
    objective's summation-error bound), ``n_iter`` (updates run)."""
    rows = np.ascontiguousarray(np.asarray(xs, dtype=np.float32)[np.asarray(ids, dtype=np.int64)])
    c = np.array(init, dtype=np.float32, copy=True)
    k, m = c.shape[0], rows.shape[0]
    assert 1 <= k <= m and niter >= 0
    prev = np.full((m,), -1, dtype=np.int64)
    objective, changed, abs_sums = [], [], []
    t = 0
    while True:
        labels, S = assign_reference(rows, c, metric)
        changed.append(int((labels != prev).sum()))
        objective.append(float(sum(S.tolist())))
        abs_sums.append(float(sum(np.abs(S).tolist())))
        prev = labels
        if (t >= 1 and changed[-1] == 0) or t == niter:
            break
        c = segment_mean_update(rows, labels, c)
        t += 1
    return {"centroids": c, "labels": labels, "D": S.astype(np.float32), "S": S,
            "counts": np.bincount(labels, minlength=k).astype(np.int64),
            "objective": np.asarray(objective, dtype=np.float64), "changed": np.asarray(changed, dtype=np.int64),
            "abs_sums": np.asarray(abs_sums, dtype=np.float64), "n_iter": t}


class OracleKMeansFlatIndex(OracleRowsFlatIndex):
    """``OracleRowsFlatIndex`` with ``kmeans`` / ``assign_rows`` (the wrappers' argument rules, the
    recipe above in place of the library call)."""

    def _member_ids(self, sel) -> np.ndarray:
        mask = self._mask(sel)
        return np.arange(self.ntotal, dtype=np.int64) if mask is None else np.flatnonzero(mask).astype(np.int64)

    def _metric(self, metric) -> str:
        return "ip" if idxmod.kmeans_metric(metric, self.metric_type) == 0 else "l2"

    def kmeans(self, k, niter=20, init=None, seed=1234, sel=None, metric=None):
        m = self._metric(metric)
        if int(k) < 1:
            raise ValueError("k must be >= 1")
        if int(niter) < 0:
            raise ValueError("niter must be >= 0")
        idxmod.kmeans_check_init(init, int(k), self.d)
        ids = self._member_ids(sel)
        k, niter = idxmod.kmeans_args(k, niter, ids.shape[0])
        c = idxmod.kmeans_init(init, k, self.d, seed, ids, self.reconstruct)
        r = kmeans_reference(self._x, ids, c, niter, m)
        return idxmod.KMeansResult(r["centroids"], r["labels"], r["D"], r["counts"], r["objective"], r["changed"],
                                   r["n_iter"])

    def assign_rows(self, centroids, sel=None, metric=None):
        m = self._metric(metric)
        c = idxmod.kmeans_centroids(centroids, self.d)
        ids = self._member_ids(sel)
        if c.shape[0] > ids.shape[0]:
            raise ValueError(f"k = {c.shape[0]} exceeds the {ids.shape[0]} members")
        labels, S = assign_reference(np.ascontiguousarray(self._x[ids]), c, m)
        return labels, S.astype(np.float32)


def oracle_kmeans_factory(dimension: int, metric: str):
    return OracleKMeansFlatIndex(dimension, "ip" if metric == "cosine" else "l2")

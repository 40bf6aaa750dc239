"""TEST INFRASTRUCTURE: the reference recipe the GPU tests hold ``vs_range_components`` to, and an
``OracleComponentsFlatIndex`` with FlatIndex's ``range_components`` surface so
``VectorStore.duplicate_groups`` / ``duplicate_labels`` run on the CPU.

Recipe (include/vs.h "duplicate groups"): the pair list of ``rows_range_reference(xs, members, radius,
self_mode="above")`` under the members' mask, a union-find over it that hooks the larger root under the
smaller (so a root is its component's smallest id), ``-1`` for the rows that are no members."""
from __future__ import annotations

import numpy as np

from oracle_facet_index import OracleFacetFlatIndex
from oracle_rows_index import rows_range_reference
from photo_search_engine_amd.index import range_radius


def components_of_pairs(n: int, first, second, members=None) -> np.ndarray:
    """Labels int64 ``(n,)`` of the graph with edges ``first[i] - second[i]`` over the ``members`` (a boolean
    mask; default every row): the smallest id of each member's component, ``-1`` for the rest."""
    parent = np.arange(n, dtype=np.int64)

    def find(x: int) -> int:
        root = x
        while parent[root] != root:
            root = parent[root]
        while parent[x] != root:
            parent[x], x = root, parent[x]
        return root

    for a, b in zip(np.asarray(first).tolist(), np.asarray(second).tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    labels = np.array([find(i) for i in range(n)], dtype=np.int64)
    if members is not None:
        labels[~np.asarray(members, dtype=bool)] = -1
    return labels


def components_reference(xs, radius, metric: str, mask=None):
    """(labels int64 n, n_components, n_edges) of ``range_components(radius, sel=mask)`` over rows ``xs``
    (the values as stored).  ``mask`` may be shorter than ``xs``: the rows behind it are no members."""
    n = int(xs.shape[0])
    r = np.float32(range_radius(radius, 1)[0])
    member = np.ones((n,), dtype=bool)
    if mask is not None:
        m = np.asarray(mask, dtype=bool)
        member[: m.shape[0]] = m[:n]
        member[m.shape[0]:] = False
    ids = np.flatnonzero(member).astype(np.int64)
    if ids.shape[0] == 0:
        return np.full((n,), -1, dtype=np.int64), 0, 0
    lims, _, I = rows_range_reference(xs, ids, r, metric, None if mask is None else member, "above")
    first = np.repeat(ids, np.diff(lims))
    labels = components_of_pairs(n, first, I, member)
    return labels, int((labels == np.arange(n)).sum()), int(lims[-1])


class OracleComponentsFlatIndex(OracleFacetFlatIndex):
    def range_components(self, radius, sel=None):
        if self.ntotal == 0:
            return np.empty((0,), dtype=np.int64), 0, 0
        return components_reference(self._x, radius, "ip" if self.metric_type == 0 else "l2", self._mask(sel))


def oracle_components_factory(dimension: int, metric: str):
    return OracleComponentsFlatIndex(dimension, "ip" if metric == "cosine" else "l2")

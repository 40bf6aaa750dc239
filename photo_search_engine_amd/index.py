"""``FlatIndex``: the faiss-IndexFlat-shaped handle over libvs (one GPU shard).

It is what ``VectorStore`` holds in ``.index`` where the reference holds a
``faiss.IndexFlatIP`` / ``faiss.IndexFlatL2`` (/root/reference/utils/vector_store.py:72-81):
``ntotal``, ``d``, ``metric_type``, ``add``, ``search``, ``reconstruct``, ``reset``.  Host
methods take numpy arrays; ``*_device`` methods take raw device pointers (ints) so callers may
hand in torch tensors' ``data_ptr()`` without torch types crossing the C ABI.
"""
from __future__ import annotations

import contextlib
import ctypes
import os
from typing import Optional, Tuple

import numpy as np

from . import _lib
from ._lib import DTYPE_CODES, METRIC_IP, METRIC_L2, check

METRIC_INNER_PRODUCT = METRIC_IP  # faiss.METRIC_INNER_PRODUCT == 0
METRIC_L2_ = METRIC_L2            # faiss.METRIC_L2 == 1


def _ptr(a: np.ndarray) -> int:
    return a.ctypes.data


def pack_allowed(n: int, allowed) -> np.ndarray:
    """The bitmap of a selector over rows ``[0, n)`` in faiss ``IDSelectorBitmap``'s layout (id ``i``
    is allowed iff ``(bitmap[i >> 3] >> (i & 7)) & 1``): ``allowed`` is a boolean mask of length
    ``n`` or an iterable of row ids (duplicates are fine).  A mask of another length or an id
    outside ``[0, n)`` raises ``ValueError``."""
    n = int(n)
    if n < 0:
        raise ValueError("n must be >= 0")
    arr = allowed if isinstance(allowed, np.ndarray) else np.asarray(list(allowed))
    if arr.dtype == np.bool_:
        if arr.ndim != 1 or arr.shape[0] != n:
            raise ValueError(f"a boolean mask must have length {n}, got shape {arr.shape}")
        mask = arr
    else:
        if arr.size == 0:
            arr = np.zeros((0,), dtype=np.int64)
        if arr.ndim != 1 or arr.dtype.kind not in "iu":
            raise ValueError("allowed must be a boolean mask or a 1-D iterable of integer row ids")
        if arr.size and (int(arr.min()) < 0 or int(arr.max()) >= n):
            raise ValueError(f"allowed ids must lie in [0, {n})")
        mask = np.zeros((n,), dtype=bool)
        mask[arr.astype(np.int64, copy=False)] = True
    return np.packbits(mask, bitorder="little")


SEL_MODES = {"auto": 0, "scan": 1, "overfetch": 2}
RANGE_MODES = {"auto": 0, "scan": 1, "screen": 2}


def range_radius(radius, nq: int) -> np.ndarray:
    """The per-query fp32 radii of a range search: a scalar is broadcast to ``nq`` values, an array
    must hold exactly ``nq``; NaN raises ``ValueError`` (``-inf`` / ``+inf`` are legal)."""
    r = np.asarray(radius, dtype=np.float32)
    if r.ndim == 0:
        r = np.full((int(nq),), r, dtype=np.float32)
    if r.ndim != 1 or r.shape[0] != int(nq):
        raise ValueError(f"radius must be a scalar or {int(nq)} values, got shape {r.shape}")
    if np.isnan(r).any():
        raise ValueError("radius must not be NaN")
    return np.ascontiguousarray(r)


def dbscan_min_samples(min_samples) -> int:
    """``min_samples`` of the density clusters as an int: an integer >= 1 (the row counts itself); anything
    else raises ``ValueError``."""
    if isinstance(min_samples, (bool, np.bool_)) or not isinstance(min_samples, (int, np.integer)):
        raise ValueError(f"min_samples must be an integer >= 1, got {min_samples!r}")
    if int(min_samples) < 1:
        raise ValueError(f"min_samples must be >= 1, got {int(min_samples)}")
    return int(min_samples)


SELF_MODES = {"keep": 0, "drop": 1, "above": 2}
SELQ_MODES = {"any": _lib.SELQ_ANY, "all": _lib.SELQ_ALL}


def selq_mode(mode) -> int:
    """The code of a score selector's mode (``"any"`` / ``"all"``); anything else raises ``ValueError``."""
    if mode not in SELQ_MODES:
        raise ValueError(f"unknown score selector mode {mode!r} (\"any\" or \"all\")")
    return SELQ_MODES[mode]


def row_ids(ids, ntotal: int) -> np.ndarray:
    """The ids of a query-from-rows call as a contiguous 1-D int64 array (repeats and any order are
    fine); anything but 1-D integers raises ``ValueError``.  Ids outside ``[0, ntotal)`` are left to
    the library, which rejects them before anything is launched."""
    arr = ids if isinstance(ids, np.ndarray) else np.asarray(list(ids))
    if arr.size == 0:
        arr = np.zeros((0,), dtype=np.int64)
    if arr.ndim != 1 or arr.dtype.kind not in "iu":
        raise ValueError("ids must be a 1-D sequence of integer row ids")
    return np.ascontiguousarray(arr, dtype=np.int64)


def drop_self_topk(D: np.ndarray, I: np.ndarray, ids: np.ndarray, k: int, metric_type: int):
    """``vs_search_rows``'s VS_SELF_DROP on the host: from lists ``min(k + 1, ntotal)`` deep, the entry
    whose id is ``ids[i]`` taken out (else the first ``k`` kept), padded to ``k`` columns."""
    n, kk = I.shape
    fill = np.float32(-3.4028235e38 if metric_type == METRIC_IP else 3.4028235e38)
    Do = np.full((n, k), fill, dtype=np.float32)
    Io = np.full((n, k), -1, dtype=np.int64)
    hit = I == ids[:, None]
    slot = np.where(hit.any(axis=1), hit.argmax(axis=1), kk)
    src = np.arange(min(k, kk))[None, :] + (np.arange(min(k, kk))[None, :] >= slot[:, None])
    ok = src < kk
    srcc = np.minimum(src, kk - 1)
    Do[:, :src.shape[1]] = np.where(ok, np.take_along_axis(D, srcc, axis=1), fill)
    Io[:, :src.shape[1]] = np.where(ok, np.take_along_axis(I, srcc, axis=1), -1)
    return Do, Io


def filter_range_self(lims: np.ndarray, D: np.ndarray, I: np.ndarray, ids: np.ndarray, mode: int):
    """``vs_range_search_rows``'s VS_SELF_DROP / VS_SELF_ABOVE on the host: a range result of the rows
    ``ids`` as queries without the entries the mode excludes (order kept)."""
    if mode == SELF_MODES["keep"] or I.shape[0] == 0:
        return lims, D, I
    n = lims.shape[0] - 1
    query = np.repeat(np.arange(n), np.diff(lims))
    keep = I != ids[query] if mode == SELF_MODES["drop"] else I > ids[query]
    out = np.zeros((n + 1,), dtype=np.int64)
    out[1:] = np.cumsum(np.bincount(query[keep], minlength=n))
    return out, D[keep], I[keep]


def _take_range_result(L, h, nq: int):
    """Copy an owned ``vs_range_result`` into numpy arrays (lims, D, I) and free it."""
    try:
        if int(L.vs_range_nq(h)) != nq:
            raise _lib.VsError(_lib.VS_ERR_INTERNAL, "range result holds another number of queries")
        lims = np.ctypeslib.as_array(ctypes.cast(L.vs_range_lims(h), ctypes.POINTER(ctypes.c_int64)),
                                     shape=(nq + 1,)).copy()
        total = int(lims[nq])
        if total:
            D = np.ctypeslib.as_array(ctypes.cast(L.vs_range_D(h), ctypes.POINTER(ctypes.c_float)),
                                      shape=(total,)).copy()
            I = np.ctypeslib.as_array(ctypes.cast(L.vs_range_I(h), ctypes.POINTER(ctypes.c_int64)),
                                      shape=(total,)).copy()
        else:
            D = np.empty((0,), dtype=np.float32)
            I = np.empty((0,), dtype=np.int64)
        return lims, D, I
    finally:
        L.vs_range_free(h)


KMEANS_METRICS = {"ip": METRIC_IP, "cosine": METRIC_IP, "inner_product": METRIC_IP, "l2": METRIC_L2,
                  "euclidean": METRIC_L2}


class KMeansResult:
    """What :meth:`FlatIndex.kmeans` returns.  ``centroids`` (k, d) fp32; ``labels`` / ``distances`` (m,):
    the cluster of each member (members in ascending id) and its fp32 score against that centroid,
    both from the last assignment pass, so they are consistent with ``centroids``; ``counts`` (k,)
    members per cluster; ``objective`` / ``changed``: one entry per assignment pass run
    (``n_iter + 1`` of them); ``n_iter``: centroid updates run."""

    __slots__ = ("centroids", "labels", "distances", "counts", "objective", "changed", "n_iter")

    def __init__(self, centroids, labels, distances, counts, objective, changed, n_iter) -> None:
        self.centroids = centroids
        self.labels = labels
        self.distances = distances
        self.counts = counts
        self.objective = objective
        self.changed = changed
        self.n_iter = int(n_iter)


class DiverseResult:
    """What :meth:`FlatIndex.search_diverse` returns.  ``D`` / ``I`` (nq, k): the accepted rows in
    acceptance order, padded with the worst score / ``-1``; ``hidden`` (nq, k) int32: the rows hidden
    under each accepted row among the rows examined; ``examined`` (nq,) int64: the rows of the ranking
    the walk looked at.  ``hidden[q].sum() + (I[q] >= 0).sum() == examined[q]``."""

    __slots__ = ("D", "I", "hidden", "examined")

    def __init__(self, D, I, hidden, examined) -> None:
        self.D = D
        self.I = I
        self.hidden = hidden
        self.examined = examined

    def __iter__(self):
        return iter((self.D, self.I, self.hidden, self.examined))


def kmeans_metric(metric, index_metric_type: int) -> int:
    """The assignment metric of a k-means call as a code: ``None`` = the index's own; a string as
    :class:`FlatIndex` takes it; anything else raises ``ValueError``."""
    if metric is None:
        return int(index_metric_type)
    if isinstance(metric, str) and metric.lower() in KMEANS_METRICS:
        return KMEANS_METRICS[metric.lower()]
    raise ValueError(f"unknown metric {metric!r}")


def kmeans_args(k, niter, members: int):
    """``(k, niter)`` of a k-means call over ``members`` rows, checked before any library call:
    ``1 <= k <= members`` and ``niter >= 0``, else ``ValueError``."""
    k, niter = int(k), int(niter)
    if k < 1:
        raise ValueError("k must be >= 1")
    if k > int(members):
        raise ValueError(f"k = {k} exceeds the {int(members)} members")
    if niter < 0:
        raise ValueError("niter must be >= 0")
    return k, niter


def kmeans_check_init(init, k: int, d: int) -> None:
    """The shape of ``init`` (see :func:`kmeans_init`), checked before the members are known."""
    if init is None:
        return
    arr = np.asarray(init)
    if arr.ndim == 2 and arr.shape == (int(k), int(d)):
        return
    if arr.ndim == 1 and arr.shape[0] == int(k) and arr.dtype.kind in "iu":
        return
    raise ValueError(f"init must be a ({int(k)}, {int(d)}) array or {int(k)} member ids, got shape {arr.shape}")


def kmeans_init(init, k: int, d: int, seed: int, member_ids: np.ndarray, reconstruct) -> np.ndarray:
    """The (k, d) fp32 initial centroids of a k-means call.  ``init`` is a (k, d) array, ``k`` member
    ids (integers: their stored rows), or ``None``: ``k`` distinct members drawn with
    ``np.random.default_rng(seed)`` and sorted (``IVFFlatIndex.train``'s recipe).  Rows are fetched
    with ``reconstruct(id)``.  A wrong shape or an id that is no member raises ``ValueError``."""
    if init is None:
        pick = np.sort(np.random.default_rng(seed).permutation(member_ids.shape[0])[:k])
        ids = member_ids[pick]
    else:
        arr = np.asarray(init)
        if arr.ndim == 2:
            if arr.shape != (k, d):
                raise ValueError(f"init must be a ({k}, {d}) array or {k} member ids, got shape {arr.shape}")
            return np.ascontiguousarray(arr, dtype=np.float32)
        if arr.ndim != 1 or arr.shape[0] != k or arr.dtype.kind not in "iu":
            raise ValueError(f"init must be a ({k}, {d}) array or {k} member ids, got shape {arr.shape}")
        ids = arr.astype(np.int64)
        if not np.isin(ids, member_ids).all():
            raise ValueError("init ids must be members (allowed rows of the index)")
    return np.ascontiguousarray(np.stack([reconstruct(int(i)) for i in ids]), dtype=np.float32)


def kmeans_centroids(centroids, d: int) -> np.ndarray:
    c = np.ascontiguousarray(centroids, dtype=np.float32)
    if c.ndim != 2 or c.shape[1] != d or c.shape[0] < 1:
        raise ValueError(f"centroids must be a (k, {d}) array with k >= 1, got shape {c.shape}")
    return c


class Selector:
    """A set of row ids of one :class:`FlatIndex` (``vs_sel``, include/vs.h): faiss's
    ``IDSelectorBitmap`` uploaded and compacted once, reused across searches.  It covers the rows
    present when it was made (rows added later are not selected) and is stale after ``reset()`` or a
    ``remove_ids`` that removed a row."""

    def __init__(self, index: "FlatIndex", allowed) -> None:
        self._h = None
        self._index = index  # (keeps the index alive while the selector is)
        self._L = index._L
        bitmap = np.ascontiguousarray(pack_allowed(index.ntotal, allowed))
        self._bitmap, self._n = bitmap, index.ntotal  # (the member ids of a k-means call)
        h = ctypes.c_void_p()
        check(self._L.vs_sel_create(index._h, _ptr(bitmap), bitmap.shape[0], ctypes.byref(h)))
        self._h = h

    @classmethod
    def from_bitmap(cls, index: "FlatIndex", bitmap) -> "Selector":
        """From a packed bitmap (``pack_allowed``'s layout; bits past ``ntotal`` are ignored, a bitmap
        shorter than ``ceil(ntotal / 8)`` bytes is an argument error)."""
        self = cls.__new__(cls)
        self._h = None
        self._index = index
        self._L = index._L
        bitmap = np.ascontiguousarray(bitmap, dtype=np.uint8)
        self._bitmap, self._n = bitmap, index.ntotal
        h = ctypes.c_void_p()
        check(self._L.vs_sel_create(index._h, _ptr(bitmap), bitmap.shape[0], ctypes.byref(h)))
        self._h = h
        return self

    @classmethod
    def _from_handle(cls, index: "FlatIndex", h, n: Optional[int] = None) -> "Selector":
        """Around a ``vs_sel`` the library built on the device (:meth:`FlatIndex.selector_from_range`,
        the set operators): there is no host bitmap until :attr:`bitmap` reads it back."""
        self = cls.__new__(cls)
        self._h = h
        self._index = index
        self._L = index._L
        # (ntotal read after the call: rows added meanwhile are past the selector's end and read as not selected)
        self._bitmap, self._n = None, index.ntotal if n is None else int(n)
        return self

    @property
    def count(self) -> int:
        """Allowed rows."""
        return int(self._L.vs_sel_count(self._h))

    @property
    def bitmap(self) -> np.ndarray:
        """The packed bitmap (``pack_allowed``'s layout, ``ceil(n / 8)`` bytes over the ``n`` rows the
        selector covers, tail bits zero).  A selector built on the device reads it back once
        (``vs_sel_bitmap``)."""
        if self._bitmap is None:
            if self._h is None:
                raise _lib.VsError(_lib.VS_ERR_ARG, "selector is closed")
            out = np.zeros(((self._n + 7) // 8,), dtype=np.uint8)
            check(self._L.vs_sel_bitmap(self._h, _ptr(out) if out.shape[0] else None, out.shape[0]))
            self._bitmap = out
        return self._bitmap

    def to_mask(self) -> np.ndarray:
        """The selector as a boolean mask over the rows it covers."""
        return np.unpackbits(self.bitmap, bitorder="little")[: self._n].astype(bool)

    def _combine(self, other, op: int) -> "Selector":
        if other is not None and not isinstance(other, Selector):
            return NotImplemented
        if self._h is None or (other is not None and other._h is None):
            raise _lib.VsError(_lib.VS_ERR_ARG, "selector is closed")
        h = ctypes.c_void_p()
        check(self._L.vs_sel_combine(self._index._h, self._h, None if other is None else other._h, op,
                                     ctypes.byref(h)))
        return Selector._from_handle(self._index, h, self._n if other is None else max(self._n, other._n))

    def __and__(self, other) -> "Selector":
        """Rows both selectors allow (``vs_sel_combine``; the operands belong to one index)."""
        return self._combine(other, _lib.SEL_AND)

    def __or__(self, other) -> "Selector":
        """Rows either selector allows."""
        return self._combine(other, _lib.SEL_OR)

    def __sub__(self, other) -> "Selector":
        """Rows this selector allows and ``other`` does not."""
        return self._combine(other, _lib.SEL_ANDNOT)

    def __invert__(self) -> "Selector":
        """The rows this selector covers and does not allow."""
        return self._combine(None, _lib.SEL_NOT)

    def close(self) -> None:
        if self._h is not None and self._h.value:
            self._L.vs_sel_destroy(self._h)
        self._h = None

    def __del__(self) -> None:  # pragma: no cover - interpreter shutdown ordering
        try:
            self.close()
        except Exception:
            pass


GROUP_KG_MAX = 3276  # k * group_size of a grouped search: ``vs_search``'s k limit
KEY_PAD = np.iinfo(np.int64).min  # ``keys`` of a group slot past the last group


class GroupedResult:
    """What :meth:`FlatIndex.search_groups` returns.  ``keys`` (nq, k) int64: the groups in order of
    their best member (an ungrouped row's negative key as given; ``KEY_PAD`` past the last group);
    ``D`` / ``I`` (nq, k, g): each group's best members in ranking order, padded with the worst score /
    ``-1``; ``found`` (nq, k) int32: the members returned for the group; ``sizes`` (nq, k) int64: the
    members the group has under the selector."""

    __slots__ = ("keys", "D", "I", "found", "sizes")

    def __init__(self, keys, D, I, found, sizes) -> None:
        self.keys = keys
        self.D = D
        self.I = I
        self.found = found
        self.sizes = sizes

    def __iter__(self):
        return iter((self.keys, self.D, self.I, self.found, self.sizes))


def group_key_array(keys, n: int) -> np.ndarray:
    """The keys of a grouped search as a contiguous int64 array of ``n`` values (one per row); anything
    but ``n`` integers raises ``ValueError``."""
    arr = keys if isinstance(keys, np.ndarray) else np.asarray(list(keys))
    if arr.size == 0:
        arr = np.zeros((0,), dtype=np.int64)
    if arr.ndim != 1 or arr.dtype.kind not in "iu" or arr.shape[0] != int(n):
        raise ValueError(f"group keys must be {int(n)} integers (one per row), got shape {arr.shape} {arr.dtype}")
    if arr.dtype.kind == "u" and arr.size and int(arr.max()) > np.iinfo(np.int64).max:
        raise ValueError("group keys must fit int64")
    return np.ascontiguousarray(arr, dtype=np.int64)


def group_args(k, group_size):
    """``(k, group_size)`` of a grouped search, checked before any library call: both ``>= 1`` and
    ``k * group_size <= GROUP_KG_MAX``, else ``ValueError``."""
    k, g = int(k), int(group_size)
    if k < 1:
        raise ValueError("k must be >= 1")
    if g < 1:
        raise ValueError("group_size must be >= 1")
    if k * g > GROUP_KG_MAX:
        raise ValueError(f"k * group_size = {k * g} exceeds {GROUP_KG_MAX}")
    return k, g


class Groups:
    """The group keys of one :class:`FlatIndex` (``vs_groups``, include/vs.h): one int64 key per row,
    uploaded once and reused across searches.  Rows with the same non-negative key form a group, a row
    with a negative key is a group of its own.  It covers the rows present when it was made (rows added
    later belong to no group and are no members of a grouped search) and is stale after ``reset()`` or a
    ``remove_ids`` that removed a row."""

    def __init__(self, index: "FlatIndex", keys) -> None:
        self._h = None
        self._index = index  # (keeps the index alive while the groups are)
        self._L = index._L
        arr = group_key_array(keys, index.ntotal)
        h = ctypes.c_void_p()
        check(self._L.vs_groups_create(index._h, _ptr(arr) if arr.size else None, arr.shape[0], ctypes.byref(h)))
        self._h = h

    @property
    def count(self) -> int:
        """Distinct non-negative keys."""
        return int(self._L.vs_groups_count(self._h))

    @property
    def rows(self) -> int:
        """Rows covered."""
        return int(self._L.vs_groups_rows(self._h))

    @property
    def keys(self) -> np.ndarray:
        """The distinct non-negative keys, ascending int64: the columns of :meth:`FlatIndex.range_count`
        (``vs_groups_keys``)."""
        if self._h is None:
            raise _lib.VsError(_lib.VS_ERR_ARG, "groups are closed")
        out = np.empty((self.count,), dtype=np.int64)
        check(self._L.vs_groups_keys(self._h, _ptr(out) if out.size else None))
        return out

    def close(self) -> None:
        if self._h is not None and self._h.value:
            self._L.vs_groups_destroy(self._h)
        self._h = None

    def __del__(self) -> None:  # pragma: no cover - interpreter shutdown ordering
        try:
            self.close()
        except Exception:
            pass


FACET_HIST = {"auto": 0, "lds": 1, "global": 2}  # VS_FACET_HIST_*
FACET_LDS_BINS = 8192  # VS_FACET_LDS_BINS
FACET_STAGING_DEFAULT = 64 << 20


ADJUST_MODES = {"auto": 0, "direct": 1, "bound": 2, "scan": 3}  # VS_ADJUST_*
FUSE_KINDS = {"any": 0, "all": 1}  # VS_FUSE_ANY / VS_FUSE_ALL
FUSE_MODES = {"auto": 0, "lists": 1, "scan": 2}  # VS_FUSE_*
FUSE_MAX_Q = 8  # VS_FUSE_MAX_Q
AFTER_MODES = {"auto": 0, "lists": 1, "scan": 2}  # VS_AFTER_*
MAXSIM_MODES = {"auto": 0, "lists": 1, "scan": 2}  # VS_MAXSIM_*
MAXSIM_STAGING_DEFAULT = 64 << 20


def maxsim_k_limit(m: int) -> int:
    """The largest ``k`` of a multi-vector search with ``m`` sub-queries: ``min(3276, VS_FUSE_WALK_MAX // m)``."""
    return min(GROUP_KG_MAX, 8192 // int(m))


def maxsim_args(q, k, d: int):
    """``(q, m, k)`` of a multi-vector search, checked before any library call: ``q`` a contiguous fp32
    ``(nq, m, d)`` array with ``1 <= m <= FUSE_MAX_Q`` and ``1 <= k <= maxsim_k_limit(m)``, else
    ``ValueError``."""
    q = np.ascontiguousarray(q, dtype=np.float32)
    if q.ndim != 3 or q.shape[2] != int(d):
        raise ValueError(f"search_maxsim expects an (nq, m, {int(d)}) array, got {q.shape}")
    m, k = q.shape[1], int(k)
    if not 1 <= m <= FUSE_MAX_Q:
        raise ValueError(f"search_maxsim takes 1..{FUSE_MAX_Q} sub-queries per query, got {m}")
    if k < 1:
        raise _lib.VsError(_lib.VS_ERR_ARG, "k must be >= 1")
    return q, m, k  # (the library rejects k above maxsim_k_limit(m))


class MaxSimResult:
    """What :meth:`FlatIndex.search_maxsim` returns.  ``keys`` (nq, k) int64: the groups, best first (an
    ungrouped row's negative key as given; ``KEY_PAD`` past the last group); ``scores`` (nq, k) float64: the
    group scores, ``-inf`` / ``+inf`` (L2) padded; ``sub_scores`` (nq, k, m) float32: the best member score
    per sub-query, padded with the worst score; ``sub_ids`` (nq, k, m) int64: the lowest member id that
    attains it, ``-1`` padded; ``sizes`` (nq, k) int64: the members the group has under the selector."""

    __slots__ = ("keys", "scores", "sub_scores", "sub_ids", "sizes")

    def __init__(self, keys, scores, sub_scores, sub_ids, sizes) -> None:
        self.keys = keys
        self.scores = scores
        self.sub_scores = sub_scores
        self.sub_ids = sub_ids
        self.sizes = sizes

    def __iter__(self):
        return iter((self.keys, self.scores, self.sub_scores, self.sub_ids, self.sizes))


def after_arrays(nq: int, after, rank_hint=None):
    """``(after, rank_hint)`` of a paged search as contiguous int64 ``(nq,)`` arrays: ``after`` a scalar (every
    query's cursor) or one row id per query, ``-1`` = from the top; ``rank_hint`` likewise, ``None`` = no
    hints."""
    out = []
    for name, a in (("after", after), ("rank_hint", rank_hint)):
        if a is None:
            if name == "after":
                raise ValueError("after must be a row id, -1, or one of either per query")
            out.append(None)
            continue
        a = np.asarray(a)
        if a.dtype.kind not in "iu":
            raise ValueError(f"{name} must hold integers")
        a = a.astype(np.int64)
        if a.ndim == 0:
            a = np.full((nq,), int(a), dtype=np.int64)
        if a.shape != (nq,):
            raise ValueError(f"{name} must be a scalar or {nq} values (one per query), got shape {a.shape}")
        out.append(np.ascontiguousarray(a))
    return out[0], out[1]


def iter_pages(search_after, nq: int, page: int):
    """The generator behind ``iter_search``: ``search_after(after, hint) -> (D, I, rank)`` called with each
    page's last id as the next cursor and ``rank + returned`` as the next hint, until every query's page came
    back short.  A query whose ranking has ended keeps its cursor (its later pages are all padding)."""
    page = int(page)
    if page < 1:
        raise ValueError("page must be >= 1")
    after = np.full((nq,), -1, dtype=np.int64)
    hint = np.zeros((nq,), dtype=np.int64)
    while True:
        D, I, rank = search_after(after, hint)
        yield D, I
        got = (I >= 0).sum(axis=1)
        if nq == 0 or bool(np.all(got < page)):
            return
        rows = np.arange(nq)
        after = np.where(got > 0, I[rows, np.maximum(got, 1) - 1], after).astype(np.int64)
        hint = (rank + got).astype(np.int64)


def adjust_arrays(n: int, scale=None, bias=None):
    """Dense ``(scale, bias)`` of an adjustment over ``n`` rows as contiguous float32 arrays (``None``
    stays ``None``: all 1 / all 0); a wrong length is ``ValueError``.  Values are checked by the library
    (``scale`` finite and ``>= 0``, ``bias`` finite)."""
    out = []
    for name, a in (("scale", scale), ("bias", bias)):
        if a is not None:
            a = np.ascontiguousarray(a, dtype=np.float32)
            if a.shape != (int(n),):
                raise ValueError(f"{name} must be {int(n)} numbers (one per row), got shape {a.shape}")
        out.append(a)
    return out[0], out[1]


def adjust_sparse_arrays(ids, scale=None, bias=None):
    """``(ids int64, scale, bias)`` of a sparse adjustment, one entry per listed row."""
    ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
    scale, bias = adjust_arrays(ids.shape[0], scale, bias)
    return ids, scale, bias


class Adjust:
    """A per-row score adjustment of one :class:`FlatIndex` (``vs_adjust``, include/vs.h): row ``i`` ranks
    by ``A = scale[i] * S + bias[i]`` instead of its score ``S``.  Uploaded once and reused across
    searches; it covers the rows present when it was made (rows added later are no members of an adjusted
    search) and is stale after ``reset()`` or a ``remove_ids`` that removed a row."""

    def __init__(self, index: "FlatIndex", scale=None, bias=None, ids=None) -> None:
        self._h = None
        self._index = index  # (keeps the index alive while the adjustment is)
        self._L = index._L
        h = ctypes.c_void_p()
        if ids is None:
            scale, bias = adjust_arrays(index.ntotal, scale, bias)
            check(self._L.vs_adjust_create(index._h, None if scale is None else _ptr(scale),
                                           None if bias is None else _ptr(bias), index.ntotal, ctypes.byref(h)))
        else:
            ids, scale, bias = adjust_sparse_arrays(ids, scale, bias)
            check(self._L.vs_adjust_create_sparse(index._h, _ptr(ids) if ids.size else None,
                                                  None if scale is None else _ptr(scale),
                                                  None if bias is None else _ptr(bias), ids.shape[0], ctypes.byref(h)))
        self._h = h

    @property
    def count(self) -> int:
        """Adjusted rows: those whose ``(scale, bias)`` is not exactly ``(1, 0)``."""
        return int(self._L.vs_adjust_count(self._h))

    @property
    def rows(self) -> int:
        """Rows covered."""
        return int(self._L.vs_adjust_rows(self._h))

    def close(self) -> None:
        if self._h is not None and self._h.value:
            self._L.vs_adjust_destroy(self._h)
        self._h = None

    def __del__(self) -> None:  # pragma: no cover - interpreter shutdown ordering
        try:
            self.close()
        except Exception:
            pass


class FlatIndex:
    """Exact flat inner-product / squared-L2 index resident in one GPU's HBM."""

    def __init__(self, d: int, metric: str = "ip", dtype: str = "f32", device: int = 0) -> None:
        self._h = None
        L = _lib.load()
        m = metric.lower()
        if m in ("ip", "cosine", "inner_product"):
            code = METRIC_IP
        elif m in ("l2", "euclidean"):
            code = METRIC_L2
        else:
            raise ValueError(f"unknown metric {metric!r}")
        if dtype not in DTYPE_CODES:
            raise ValueError(f"unknown dtype {dtype!r}")
        h = ctypes.c_void_p()
        check(L.vs_create(int(d), code, DTYPE_CODES[dtype], int(device), ctypes.byref(h)))
        self._h = h
        self._L = L
        self.d = int(d)
        self.metric_type = code
        self.dtype = dtype
        self.device = int(device)

    def _queries(self, q, name: str) -> np.ndarray:
        """``q`` as a contiguous fp32 ``(nq, d)`` array (``name``: the calling method, for the error)."""
        q = np.ascontiguousarray(q, dtype=np.float32)
        if q.ndim != 2 or q.shape[1] != self.d:
            raise ValueError(f"{name} expects an (nq, {self.d}) array, got {q.shape}")
        return q

    @contextlib.contextmanager
    def _sel(self, sel):
        """``(selector, handle)`` for one call: ``sel`` itself, a temporary :class:`Selector` made from a mask
        or row ids and closed on exit, or ``(None, None)``.  A closed selector is an argument error."""
        s = sel if sel is None or isinstance(sel, Selector) else Selector(self, sel)
        try:
            if s is not None and s._h is None:
                raise _lib.VsError(_lib.VS_ERR_ARG, "selector is closed")
            yield s, (None if s is None else s._h)
        finally:
            if s is not sel:
                s.close()

    # -- faiss-like surface ------------------------------------------------------------------
    @property
    def ntotal(self) -> int:
        return int(self._L.vs_ntotal(self._h))

    def add(self, x) -> None:
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim != 2 or x.shape[1] != self.d:
            raise ValueError(f"add expects an (n, {self.d}) array, got {x.shape}")
        check(self._L.vs_add(self._h, _ptr(x), x.shape[0]))

    def search(self, q, k: int, sel=None) -> Tuple[np.ndarray, np.ndarray]:
        """Exact top-``k``; with ``sel`` (a :class:`Selector`, a boolean mask or row ids) the exact
        top-``k`` among the allowed rows -- faiss's ``search(q, k, params=SearchParameters(sel=...))``
        -- padded with ``-1`` / the worst score when fewer than ``k`` rows are allowed."""
        q = self._queries(q, "search")
        nq = q.shape[0]
        k = int(k)
        if k <= 0:
            raise _lib.VsError(_lib.VS_ERR_ARG, "k must be > 0")
        D = np.empty((nq, k), dtype=np.float32)
        I = np.empty((nq, k), dtype=np.int64)
        if sel is None:
            check(self._L.vs_search(self._h, _ptr(q), nq, k, _ptr(D), _ptr(I)))
            return D, I
        with self._sel(sel) as (_, sh):
            check(self._L.vs_search_sel(self._h, sh, _ptr(q), nq, k, _ptr(D), _ptr(I)))
        return D, I

    def range_search(self, q, radius, sel=None, max_total: Optional[int] = None):
        """faiss ``IndexFlat.range_search``: every row whose fp32 score ``D`` passes ``radius`` (``D >
        radius`` inner product, ``D < radius`` squared L2; a scalar or one value per query) as
        ``(lims, D, I)``, query ``i``'s rows at ``[lims[i], lims[i + 1])`` best first -- the first
        entries of ``search(q, k)``.  ``sel`` as in :meth:`search`; ``max_total`` caps the number of
        results (beyond it the call raises, naming the count)."""
        q = self._queries(q, "range_search")
        nq = q.shape[0]
        r = range_radius(radius, nq)
        cap = 0 if max_total is None else int(max_total)
        if max_total is not None and cap <= 0:
            raise ValueError("max_total must be > 0")
        h = ctypes.c_void_p()
        with self._sel(sel) as (_, sh):
            check(self._L.vs_range_search(self._h, sh, _ptr(q), nq, _ptr(r), cap, ctypes.byref(h)))
        return _take_range_result(self._L, h, nq)

    def search_rows(self, ids, k: int, sel=None, drop_self: bool = True) -> Tuple[np.ndarray, np.ndarray]:
        """:meth:`search` with stored rows as the queries (``vs_search_rows``): query ``i`` is the stored
        value of row ``ids[i]`` as :meth:`reconstruct` returns it, gathered on the device -- no query
        crosses the host.  ``drop_self`` (default) leaves row ``ids[i]`` itself out of its own list, by
        id (an identical row with a lower id comes first and stays): the search runs one entry deeper
        and the list is padded as :meth:`search` pads it.  ``drop_self=False`` is bit-equal to
        ``search(reconstruct rows, k, sel)``.  ``ids`` may repeat, in any order; ``sel`` as in
        :meth:`search`."""
        ids = row_ids(ids, self.ntotal)
        n = ids.shape[0]
        k = int(k)
        if k <= 0:
            raise _lib.VsError(_lib.VS_ERR_ARG, "k must be > 0")
        D = np.empty((n, k), dtype=np.float32)
        I = np.empty((n, k), dtype=np.int64)
        with self._sel(sel) as (_, sh):
            check(self._L.vs_search_rows(self._h, sh, _ptr(ids), n, k, SELF_MODES["drop" if drop_self else "keep"],
                                         _ptr(D), _ptr(I)))
        return D, I

    def range_search_rows(self, radius, ids=None, sel=None, self_mode: str = "above",
                          max_total: Optional[int] = None):
        """:meth:`range_search` with stored rows as the queries (``vs_range_search_rows``): ``ids=None``
        is the whole-corpus self-join (rows ``0..ntotal-1``); ``radius`` a scalar or one value per
        query.  ``self_mode``: ``"above"`` returns only rows with an id above the query's own, so a
        self-join lists every pair once, as (lower id, higher id), and scans only the rows that can
        still pass; ``"drop"`` leaves out the row itself; ``"keep"`` is bit-equal to
        ``range_search(reconstruct rows, radius, sel)``.  The excluded rows are never counted:
        ``max_total`` and :meth:`range_last_stats` see the filtered answer."""
        if self_mode not in SELF_MODES:
            raise ValueError(f"unknown self_mode {self_mode!r}")
        cap = 0 if max_total is None else int(max_total)
        if max_total is not None and cap <= 0:
            raise ValueError("max_total must be > 0")
        ids = None if ids is None else row_ids(ids, self.ntotal)
        n = self.ntotal if ids is None else ids.shape[0]
        r = range_radius(radius, n)
        h = ctypes.c_void_p()
        with self._sel(sel) as (_, sh):
            check(self._L.vs_range_search_rows(self._h, sh, _ptr(ids) if ids is not None else None, n, _ptr(r),
                                               SELF_MODES[self_mode], cap, ctypes.byref(h)))
        return _take_range_result(self._L, h, n)

    def _kmeans_call(self, s, k: int, niter: int, metric: int, c: np.ndarray, m: int) -> KMeansResult:
        labels = np.empty((m,), dtype=np.int64)
        D = np.empty((m,), dtype=np.float32)
        counts = np.zeros((k,), dtype=np.int64)
        objective = np.zeros((niter + 1,), dtype=np.float64)
        changed = np.zeros((niter + 1,), dtype=np.int64)
        done = ctypes.c_int32(0)
        check(self._L.vs_kmeans(self._h, s._h if s is not None else None, k, niter, metric, _ptr(c), _ptr(labels),
                                _ptr(D), _ptr(counts), _ptr(objective), _ptr(changed), ctypes.byref(done)))
        n = int(done.value)
        return KMeansResult(c, labels, D, counts, objective[: n + 1].copy(), changed[: n + 1].copy(), n)

    def _members(self, s) -> np.ndarray:
        """Ascending ids of the members of a k-means call under selector ``s`` (``None``: every row)."""
        if s is None:
            return np.arange(self.ntotal, dtype=np.int64)
        return np.flatnonzero(np.unpackbits(s.bitmap, bitorder="little")[: s._n]).astype(np.int64)

    def kmeans(self, k: int, niter: int = 20, init=None, seed: int = 1234, sel=None, metric=None) -> KMeansResult:
        """Exact k-means over the stored rows (``vs_kmeans``, include/vs.h): the members -- every row,
        or the rows ``sel`` allows -- are assigned to their exact best centroid under ``metric``
        (``"ip"`` / ``"l2"``; ``None`` = the index's own) and the centroids are recomputed on the device
        in a fixed summation order, so the result is reproducible to the bit.  ``init``: a (k, d)
        array, ``k`` member ids, or ``None`` for ``k`` distinct members drawn with
        ``np.random.default_rng(seed)``.  It stops after ``niter`` updates or at a fixed point.
        Returns a :class:`KMeansResult`."""
        code = kmeans_metric(metric, self.metric_type)
        if int(k) < 1:
            raise ValueError("k must be >= 1")
        if int(niter) < 0:
            raise ValueError("niter must be >= 0")
        kmeans_check_init(init, int(k), self.d)
        with self._sel(sel) as (s, _):
            members = self._members(s)
            k, niter = kmeans_args(k, niter, members.shape[0])
            c = kmeans_init(init, k, self.d, seed, members, self.reconstruct).copy()
            return self._kmeans_call(s, k, niter, code, c, members.shape[0])

    def assign_rows(self, centroids, sel=None, metric=None) -> Tuple[np.ndarray, np.ndarray]:
        """The ``niter = 0`` form of :meth:`kmeans`: ``(labels, distances)`` of the members against the
        given centroids -- bit-equal to ``search(reconstruct rows, 1)`` on a flat index of them."""
        code = kmeans_metric(metric, self.metric_type)
        c = kmeans_centroids(centroids, self.d).copy()
        with self._sel(sel) as (s, _):
            m = self.ntotal if s is None else s.count
            if c.shape[0] > m:
                raise ValueError(f"k = {c.shape[0]} exceeds the {m} members")
            r = self._kmeans_call(s, c.shape[0], 0, code, c, m)
            return r.labels, r.distances

    def search_diverse(self, q, k: int, radius, sel=None) -> DiverseResult:
        """Exact top-``k`` with near-duplicates collapsed (``vs_search_diverse``, include/vs.h): the
        exact ranking of each query is walked best first and a row is accepted iff its fp32 score with
        every row accepted before it does not pass ``radius`` (``D > radius`` inner product, ``D <
        radius`` squared L2 -- the predicate of :meth:`range_search_rows`; a scalar or one value per
        query); otherwise it counts as hidden under the earliest-accepted row it is near.  ``sel`` as
        in :meth:`search`.  Returns a :class:`DiverseResult`."""
        q = self._queries(q, "search_diverse")
        nq = q.shape[0]
        k = int(k)
        if k <= 0:
            raise _lib.VsError(_lib.VS_ERR_ARG, "k must be > 0")
        r = range_radius(radius, nq)
        D = np.empty((nq, k), dtype=np.float32)
        I = np.empty((nq, k), dtype=np.int64)
        hidden = np.zeros((nq, k), dtype=np.int32)
        examined = np.zeros((nq,), dtype=np.int64)
        with self._sel(sel) as (_, sh):
            check(self._L.vs_search_diverse(self._h, sh, _ptr(q), nq, k, _ptr(r), _ptr(D), _ptr(I), _ptr(hidden),
                                            _ptr(examined)))
        return DiverseResult(D, I, hidden, examined)

    def set_diverse_depth(self, first: int = 0, limit: int = 0) -> None:
        """The list lengths :meth:`search_diverse` walks: the first list and the longest one before
        the full ranking (``0`` = the defaults; the same bits under every setting,
        ``vs_set_diverse_depth``)."""
        check(self._L.vs_set_diverse_depth(self._h, int(first), int(limit)))

    def diverse_last_stats(self) -> dict:
        """The last :meth:`search_diverse`: queries, how many were complete after the first list, after
        a deeper list, how many were answered from the full ranking, and the longest list walked
        (``vs_diverse_last_stats``)."""
        buf = (ctypes.c_int64 * 5)()
        check(self._L.vs_diverse_last_stats(self._h, buf, 5))
        return {"queries": int(buf[0]), "first": int(buf[1]), "deeper": int(buf[2]), "full": int(buf[3]),
                "longest": int(buf[4])}

    def diverse_last_times(self) -> dict:
        """HIP-event milliseconds of the last :meth:`search_diverse`, per tier (``vs_diverse_last_times``)."""
        buf = (ctypes.c_double * 6)()
        check(self._L.vs_diverse_last_times(self._h, buf, 6))
        return {"search_ms": [float(buf[0]), float(buf[2]), float(buf[4])],
                "walk_ms": [float(buf[1]), float(buf[3]), float(buf[5])]}

    def group_keys(self, keys) -> Groups:
        """Reusable :class:`Groups` over the rows present now: ``ntotal`` integer keys, one per row."""
        return Groups(self, keys)

    def search_groups(self, q, k: int, groups: Groups, group_size: int = 1, sel=None) -> GroupedResult:
        """Exact top-``k`` groups by key with the best ``group_size`` rows of each
        (``vs_search_groups``, include/vs.h): the members -- the rows ``groups`` covers, under ``sel``
        those of them it allows -- are ranked as :meth:`search` ranks them, the groups are ordered by
        their best member and each comes with its best members in ranking order.  ``sel`` as in
        :meth:`search`.  Returns a :class:`GroupedResult`."""
        q = self._queries(q, "search_groups")
        if not isinstance(groups, Groups):
            raise TypeError("groups must be a Groups object (FlatIndex.group_keys)")
        nq = q.shape[0]
        k, g = int(k), int(group_size)
        if k < 1 or g < 1:
            raise _lib.VsError(_lib.VS_ERR_ARG, "k and group_size must be >= 1")
        keys = np.empty((nq, k), dtype=np.int64)
        D = np.empty((nq, k, g), dtype=np.float32)
        I = np.empty((nq, k, g), dtype=np.int64)
        found = np.zeros((nq, k), dtype=np.int32)
        sizes = np.zeros((nq, k), dtype=np.int64)
        with self._sel(sel) as (_, sh):
            if groups._h is None:
                raise _lib.VsError(_lib.VS_ERR_ARG, "groups are closed")
            check(self._L.vs_search_groups(self._h, groups._h, sh, _ptr(q), nq, k, g, _ptr(keys), _ptr(D), _ptr(I),
                                           _ptr(found), _ptr(sizes)))
        return GroupedResult(keys, D, I, found, sizes)

    def set_group_depth(self, first: int = 0, limit: int = 0) -> None:
        """The list lengths :meth:`search_groups` walks: the first list and the longest one, which the
        restricted rounds use too (``0`` = the defaults; the same bits under every setting,
        ``vs_set_group_depth``).  A call with ``k * group_size > limit`` is an argument error."""
        check(self._L.vs_set_group_depth(self._h, int(first), int(limit)))

    def group_last_stats(self) -> dict:
        """The last :meth:`search_groups`: queries, how many were complete after the first list, after
        a deeper list, how many were finished by restricted rounds, the rounds run in total and the
        longest list walked (``vs_group_last_stats``)."""
        buf = (ctypes.c_int64 * 6)()
        check(self._L.vs_group_last_stats(self._h, buf, 6))
        return {"queries": int(buf[0]), "first": int(buf[1]), "deeper": int(buf[2]), "finished": int(buf[3]),
                "rounds": int(buf[4]), "longest": int(buf[5])}

    def group_last_times(self) -> dict:
        """HIP-event milliseconds of the last :meth:`search_groups`, per tier, and the parts of the
        restricted rounds' list search spent building and compacting the restricted set
        (``vs_group_last_times``)."""
        buf = (ctypes.c_double * 8)()
        check(self._L.vs_group_last_times(self._h, buf, 8))
        return {"search_ms": [float(buf[0]), float(buf[2]), float(buf[4])],
                "walk_ms": [float(buf[1]), float(buf[3]), float(buf[5])],
                "restrict_ms": float(buf[6]), "compact_ms": float(buf[7])}

    def score_adjust(self, scale=None, bias=None) -> Adjust:
        """Reusable :class:`Adjust` over the rows present now: ``ntotal`` scales and biases, one per row
        (``None``: all 1 / all 0)."""
        return Adjust(self, scale, bias)

    def score_adjust_sparse(self, ids, scale=None, bias=None) -> Adjust:
        """Reusable :class:`Adjust` that adjusts the listed rows (distinct ids, any order) and leaves every
        other row plain."""
        return Adjust(self, scale, bias, ids=ids)

    def search_adjusted(self, q, k: int, adjust: Adjust, sel=None, return_raw: bool = False):
        """Exact top-``k`` by the adjusted score ``A = scale * S + bias`` (``vs_search_adjusted``,
        include/vs.h): the members -- the rows ``adjust`` covers, under ``sel`` those of them it allows --
        ranked by ``A`` in the metric's direction, ties to the lower id.  Returns ``(D, I)`` with ``D`` the
        adjusted scores, and with ``return_raw`` ``(D, I, D_raw)``, ``D_raw`` the scores :meth:`search`
        reports for the same rows."""
        q = self._queries(q, "search_adjusted")
        if not isinstance(adjust, Adjust):
            raise TypeError("adjust must be an Adjust object (FlatIndex.score_adjust)")
        nq, k = q.shape[0], int(k)
        if k < 1:
            raise _lib.VsError(_lib.VS_ERR_ARG, "k must be >= 1")
        D = np.empty((nq, k), dtype=np.float32)
        I = np.empty((nq, k), dtype=np.int64)
        R = np.empty((nq, k), dtype=np.float32) if return_raw else None
        with self._sel(sel) as (_, sh):
            if adjust._h is None:
                raise _lib.VsError(_lib.VS_ERR_ARG, "adjustment is closed")
            check(self._L.vs_search_adjusted(self._h, adjust._h, sh, _ptr(q), nq, k, _ptr(D), _ptr(I),
                                             _ptr(R) if return_raw else None))
        return (D, I, R) if return_raw else (D, I)

    def set_adjust_mode(self, mode: str) -> None:
        """Force the tier of adjusted searches (``"direct"``, ``"bound"``, ``"scan"``) or let the library
        choose (``"auto"``); the same bits under every mode (``vs_set_adjust_mode``)."""
        if mode not in ADJUST_MODES:
            raise ValueError(f"adjust mode must be one of {sorted(ADJUST_MODES)}")
        check(self._L.vs_set_adjust_mode(self._h, ADJUST_MODES[mode]))

    def set_adjust_depth(self, first: int = 0, limit: int = 0) -> None:
        """The list lengths :meth:`search_adjusted` walks: the first list and the longest one (``0`` = the
        defaults; the same bits under every setting, ``vs_set_adjust_depth``)."""
        check(self._L.vs_set_adjust_depth(self._h, int(first), int(limit)))

    def adjust_last_stats(self) -> dict:
        """The last :meth:`search_adjusted`: queries, how many were complete after the first list, after a
        deeper list, how many the scan answered, the longest list walked, the tier taken and the adjusted
        rows (``vs_adjust_last_stats``)."""
        buf = (ctypes.c_int64 * 7)()
        check(self._L.vs_adjust_last_stats(self._h, buf, 7))
        tier = {v: n for n, v in ADJUST_MODES.items()}[int(buf[5])]
        return {"queries": int(buf[0]), "first": int(buf[1]), "deeper": int(buf[2]), "scan": int(buf[3]),
                "longest": int(buf[4]), "tier": tier, "adjusted": int(buf[6])}

    def adjust_last_times(self) -> dict:
        """HIP-event milliseconds of the last :meth:`search_adjusted`: list search and walk per list tier,
        the direct scan over the adjusted rows and the full scan (``vs_adjust_last_times``)."""
        buf = (ctypes.c_double * 6)()
        check(self._L.vs_adjust_last_times(self._h, buf, 6))
        return {"search_ms": [float(buf[0]), float(buf[2])], "walk_ms": [float(buf[1]), float(buf[3])],
                "direct_scan_ms": float(buf[4]), "full_scan_ms": float(buf[5])}

    def search_fused(self, q, k: int, mode: str = "any", sel=None, return_sub: bool = False):
        """Exact top-``k`` of fused queries (``vs_search_fused``, include/vs.h): ``q`` is ``(nq, m, d)``, one
        fused query per ``m`` sub-queries (``1 <= m <= 8``).  Every member -- every row, under ``sel`` the
        rows it allows -- is ranked by ``F``, its best (``mode="any"``) or its worst (``mode="all"``) score
        over the sub-queries, in the metric's direction, ties to the lower id.  Returns ``(D, I, which)``,
        ``D`` the fused scores and ``which`` the lowest sub-query index whose score is ``F``, and with
        ``return_sub`` ``(D, I, which, D_sub)``, ``D_sub`` ``(nq, k, m)`` the row's score under every
        sub-query.  ``k`` is at most ``min(3276, 8192 // m)``."""
        q = np.ascontiguousarray(q, dtype=np.float32)
        if q.ndim != 3 or q.shape[2] != self.d:
            raise ValueError(f"search_fused expects an (nq, m, {self.d}) array, got {q.shape}")
        if mode not in FUSE_KINDS:
            raise ValueError(f"fuse mode must be one of {sorted(FUSE_KINDS)}")
        nq, m, k = q.shape[0], q.shape[1], int(k)
        if not 1 <= m <= FUSE_MAX_Q:
            raise ValueError(f"search_fused takes 1..{FUSE_MAX_Q} sub-queries per fused query, got {m}")
        if k < 1:
            raise _lib.VsError(_lib.VS_ERR_ARG, "k must be >= 1")
        D = np.empty((nq, k), dtype=np.float32)
        I = np.empty((nq, k), dtype=np.int64)
        W = np.empty((nq, k), dtype=np.int32)
        U = np.empty((nq, k, m), dtype=np.float32) if return_sub else None
        with self._sel(sel) as (_, sh):
            check(self._L.vs_search_fused(self._h, sh, _ptr(q), nq, m, FUSE_KINDS[mode], k, _ptr(D), _ptr(I), _ptr(W),
                                          _ptr(U) if return_sub else None))
        return (D, I, W, U) if return_sub else (D, I, W)

    def set_fuse_mode(self, mode: str) -> None:
        """Force the tier of fused searches (``"lists"``, ``"scan"``) or let the library choose
        (``"auto"``); the same bits under every mode (``vs_set_fuse_mode``)."""
        if mode not in FUSE_MODES:
            raise ValueError(f"fuse tier must be one of {sorted(FUSE_MODES)}")
        check(self._L.vs_set_fuse_mode(self._h, FUSE_MODES[mode]))

    def set_fuse_depth(self, first: int = 0, limit: int = 0) -> None:
        """The list lengths ``mode="all"`` of :meth:`search_fused` walks: the first list and the longest one
        (``0`` = the defaults; the same bits under every setting, ``vs_set_fuse_depth``)."""
        check(self._L.vs_set_fuse_depth(self._h, int(first), int(limit)))

    def fuse_last_stats(self) -> dict:
        """The last :meth:`search_fused`: fused queries, how many were complete after the first list, after a
        deeper list, how many the scan answered, the longest list walked and the tier taken
        (``vs_fuse_last_stats``)."""
        buf = (ctypes.c_int64 * 6)()
        check(self._L.vs_fuse_last_stats(self._h, buf, 6))
        tier = {v: n for n, v in FUSE_MODES.items()}[int(buf[5])]
        return {"queries": int(buf[0]), "first": int(buf[1]), "deeper": int(buf[2]), "scan": int(buf[3]),
                "longest": int(buf[4]), "tier": tier}

    def fuse_last_times(self) -> dict:
        """HIP-event milliseconds of the last :meth:`search_fused`: list search and walk per list tier, the
        scan and the walk that reports its rows (``vs_fuse_last_times``)."""
        buf = (ctypes.c_double * 6)()
        check(self._L.vs_fuse_last_times(self._h, buf, 6))
        return {"search_ms": [float(buf[0]), float(buf[2])], "walk_ms": [float(buf[1]), float(buf[3])],
                "scan_ms": float(buf[4]), "scan_walk_ms": float(buf[5])}

    def search_maxsim(self, q, k: int, groups: Groups, sel=None) -> MaxSimResult:
        """Exact top-``k`` groups by summed best matches (``vs_search_maxsim``, include/vs.h): ``q`` is
        ``(nq, m, d)``, one query per ``m`` sub-queries (``1 <= m <= 8``).  A group's score is the fp64 sum,
        left to right, of the best score any of its members -- the rows ``groups`` covers, under ``sel``
        those of them it allows -- reaches under each sub-query; the groups are ranked by it in the metric's
        direction, ties to the lower group.  ``k`` is at most ``maxsim_k_limit(m)``.  Returns a
        :class:`MaxSimResult`."""
        q, m, k = maxsim_args(q, k, self.d)
        if not isinstance(groups, Groups):
            raise TypeError("groups must be a Groups object (FlatIndex.group_keys)")
        nq = q.shape[0]
        keys = np.empty((nq, k), dtype=np.int64)
        F = np.empty((nq, k), dtype=np.float64)
        U = np.empty((nq, k, m), dtype=np.float32)
        J = np.empty((nq, k, m), dtype=np.int64)
        sizes = np.empty((nq, k), dtype=np.int64)
        with self._sel(sel) as (_, sh):
            if groups._h is None:
                raise _lib.VsError(_lib.VS_ERR_ARG, "groups are closed")
            check(self._L.vs_search_maxsim(self._h, groups._h, sh, _ptr(q), nq, m, k, _ptr(keys), _ptr(F), _ptr(U),
                                           _ptr(J), _ptr(sizes)))
        return MaxSimResult(keys, F, U, J, sizes)

    def set_maxsim_mode(self, mode: str) -> None:
        """Force the tier of multi-vector searches (``"lists"``, ``"scan"``) or let the library choose
        (``"auto"``); the same bits under every mode (``vs_set_maxsim_mode``)."""
        if mode not in MAXSIM_MODES:
            raise ValueError(f"maxsim tier must be one of {sorted(MAXSIM_MODES)}")
        check(self._L.vs_set_maxsim_mode(self._h, MAXSIM_MODES[mode]))

    def set_maxsim_depth(self, first: int = 0, limit: int = 0, walk_rows: int = 0) -> None:
        """The list lengths :meth:`search_maxsim` walks -- the first list and the longest one -- and the rows
        one walk may go through before its query is left to the scan (``0`` = the defaults; the same bits
        under every setting, ``vs_set_maxsim_depth``)."""
        check(self._L.vs_set_maxsim_depth(self._h, int(first), int(limit), int(walk_rows)))

    def maxsim_last_stats(self) -> dict:
        """The last :meth:`search_maxsim`: queries, how many were complete after the first list, after a
        deeper list, how many the scan answered, the longest list walked, the tier taken and the rows of the
        candidate groups the answering walks went through (``vs_maxsim_last_stats``)."""
        buf = (ctypes.c_int64 * 7)()
        check(self._L.vs_maxsim_last_stats(self._h, buf, 7))
        tier = {v: n for n, v in MAXSIM_MODES.items()}[int(buf[5])]
        return {"queries": int(buf[0]), "first": int(buf[1]), "deeper": int(buf[2]), "scan": int(buf[3]),
                "longest": int(buf[4]), "tier": tier, "walked": int(buf[6])}

    def maxsim_last_times(self) -> dict:
        """HIP-event milliseconds of the last :meth:`search_maxsim`: list search and walk per list tier, the
        scan, the rank and the final walk (``vs_maxsim_last_times``)."""
        buf = (ctypes.c_double * 7)()
        check(self._L.vs_maxsim_last_times(self._h, buf, 7))
        return {"search_ms": [float(buf[0]), float(buf[2])], "walk_ms": [float(buf[1]), float(buf[3])],
                "scan_ms": float(buf[4]), "rank_ms": float(buf[5]), "scan_walk_ms": float(buf[6])}

    def search_after(self, q, k: int, after, sel=None, rank_hint=None, return_rank: bool = False):
        """The ``k`` rows that follow a cursor row in :meth:`search`'s ranking (``vs_search_after``,
        include/vs.h): ``after`` is a row id per query (or one for all), ``-1`` = from the top; the members
        -- every row, under ``sel`` the rows it allows -- that rank strictly after the cursor row's position
        (a worse score, or an equal score and a higher id) come back best first as ``(D, I)``, padded as
        :meth:`search` pads, and with ``return_rank`` as ``(D, I, rank)``, ``rank`` the members at or before
        the cursor.  The cursor row need not be a member.  ``rank_hint`` (the caller's guess of ``rank``,
        ``-1`` = unknown) changes the work only, never the result."""
        q = self._queries(q, "search_after")
        nq, k = q.shape[0], int(k)
        if k < 1:
            raise _lib.VsError(_lib.VS_ERR_ARG, "k must be >= 1")
        after, hint = after_arrays(nq, after, rank_hint)
        D = np.empty((nq, k), dtype=np.float32)
        I = np.empty((nq, k), dtype=np.int64)
        rank = np.zeros((nq,), dtype=np.int64)
        with self._sel(sel) as (_, sh):
            check(self._L.vs_search_after(self._h, sh, _ptr(q), nq, k, _ptr(after), None if hint is None else _ptr(hint),
                                          _ptr(D), _ptr(I), _ptr(rank)))
        return (D, I, rank) if return_rank else (D, I)

    def iter_search(self, q, page: int, sel=None):
        """Generator of ``(D, I)`` pages of ``page`` rows for a batch of queries: :meth:`search_after` chained
        from the top, each page's last id the next cursor and ``rank + returned`` the next hint.  The pages of
        a query concatenate to its whole ranking; the generator ends when every query's page came back short
        (a query that ended earlier yields padding meanwhile).  ``sel`` (a :class:`Selector`, a mask or ids) is
        resolved once."""
        q = self._queries(q, "iter_search")
        if int(page) < 1:
            raise ValueError("page must be >= 1")

        def pages():
            with self._sel(sel) as (s, _):
                yield from iter_pages(lambda after, hint: self.search_after(q, page, after, sel=s, rank_hint=hint,
                                                                            return_rank=True), q.shape[0], page)
        return pages()

    def set_after_mode(self, mode: str) -> None:
        """Force the tier of paged searches (``"lists"``, ``"scan"``) or let the library choose
        (``"auto"``); the same bits under every mode (``vs_set_after_mode``)."""
        if mode not in AFTER_MODES:
            raise ValueError(f"after tier must be one of {sorted(AFTER_MODES)}")
        check(self._L.vs_set_after_mode(self._h, AFTER_MODES[mode]))

    def set_after_depth(self, first: int = 0, limit: int = 0) -> None:
        """The list lengths :meth:`search_after` cuts: the first list and the longest one (``0`` = the
        defaults; the same bits under every setting, ``vs_set_after_depth``)."""
        check(self._L.vs_set_after_depth(self._h, int(first), int(limit)))

    def after_last_stats(self) -> dict:
        """The last :meth:`search_after`: queries, how many were complete after the first list, after a
        deeper list, how many the scan answered, the longest list walked and the tier taken
        (``vs_after_last_stats``)."""
        buf = (ctypes.c_int64 * 6)()
        check(self._L.vs_after_last_stats(self._h, buf, 6))
        tier = {v: n for n, v in AFTER_MODES.items()}[int(buf[5])]
        return {"queries": int(buf[0]), "first": int(buf[1]), "deeper": int(buf[2]), "scan": int(buf[3]),
                "longest": int(buf[4]), "tier": tier}

    def after_last_times(self) -> dict:
        """HIP-event milliseconds of the last :meth:`search_after`: list search and cut per list tier, the
        cursor scoring and the scan (``vs_after_last_times``)."""
        buf = (ctypes.c_double * 6)()
        check(self._L.vs_after_last_times(self._h, buf, 6))
        return {"search_ms": [float(buf[0]), float(buf[2])], "cut_ms": [float(buf[1]), float(buf[3])],
                "score_ms": float(buf[4]), "scan_ms": float(buf[5])}

    def set_range_mode(self, mode: str) -> None:
        """Force the tier of range searches (``"scan"``, ``"screen"`` where it applies) or let the
        library choose (``"auto"``); the same bits under every mode (``vs_set_range_mode``)."""
        if mode not in RANGE_MODES:
            raise ValueError(f"unknown range mode {mode!r}")
        check(self._L.vs_set_range_mode(self._h, RANGE_MODES[mode]))

    def range_last_stats(self) -> dict:
        """The last range search: results, tier taken, queries the scan re-answered after a screen
        overflow, segments sorted on the host (``vs_range_last_stats``)."""
        buf = (ctypes.c_int64 * 4)()
        check(self._L.vs_range_last_stats(self._h, buf, 4))
        return {"total": int(buf[0]), "tier": {1: "scan", 2: "screen"}.get(int(buf[1]), "none"),
                "rescanned": int(buf[2]), "host_sorted": int(buf[3])}

    def range_count(self, q, radius, groups: Optional[Groups] = None, sel=None):
        """Exact facet counts (``vs_range_count``, include/vs.h): how many members pass ``radius`` --
        :meth:`range_search`'s predicate, ``radius`` a scalar or one value per query -- and how they split
        over the groups, without producing a row.  Members: the rows ``groups`` covers (every stored row
        without ``groups``), under ``sel`` (as in :meth:`search`) those of them it allows.  Returns
        ``(totals, counts)``: ``totals`` int64 ``(nq,)``; ``counts`` int64 ``(nq, G + 1)`` -- column ``g``
        the group with key ``groups.keys[g]``, the last column the rows with a negative key -- or ``None``
        without ``groups``."""
        q = self._queries(q, "range_count")
        nq = q.shape[0]
        r = range_radius(radius, nq)
        if groups is not None and not isinstance(groups, Groups):
            raise TypeError("groups must be a Groups object (FlatIndex.group_keys)")
        totals = np.zeros((nq,), dtype=np.int64)
        with self._sel(sel) as (_, sh):
            if groups is None:
                check(self._L.vs_range_count(self._h, None, sh, _ptr(q), nq, _ptr(r), None, _ptr(totals)))
                return totals, None
            if groups._h is None:
                raise _lib.VsError(_lib.VS_ERR_ARG, "groups are closed")
            counts = np.zeros((nq, groups.count + 1), dtype=np.int64)
            check(self._L.vs_range_count(self._h, groups._h, sh, _ptr(q), nq, _ptr(r), _ptr(counts), _ptr(totals)))
        return totals, counts

    def set_facet_hist(self, form: str) -> None:
        """Force the histogram form of :meth:`range_count`'s scan (``"lds"``, ``"global"``) or let the
        library choose (``"auto"``); the same integers under every form (``vs_set_facet_hist``).  Forcing
        ``"lds"`` makes a call with more than ``FACET_LDS_BINS`` bins an argument error."""
        if form not in FACET_HIST:
            raise ValueError(f"unknown facet histogram form {form!r}")
        check(self._L.vs_set_facet_hist(self._h, FACET_HIST[form]))

    def facet_last_stats(self) -> dict:
        """The last :meth:`range_count`: the sum of its totals, the tier taken, the queries the scan
        re-answered after a screen overflow, the histogram form the scan took and the query blocks
        (``vs_facet_last_stats``)."""
        buf = (ctypes.c_int64 * 5)()
        check(self._L.vs_facet_last_stats(self._h, buf, 5))
        return {"total": int(buf[0]), "tier": {1: "scan", 2: "screen"}.get(int(buf[1]), "none"),
                "rescanned": int(buf[2]), "hist": {1: "lds", 2: "global"}.get(int(buf[3]), "none"),
                "blocks": int(buf[4])}

    def facet_last_times(self) -> dict:
        """HIP-event milliseconds of the last :meth:`range_count`: screen + refine, scan, table readback
        (``vs_facet_last_times``)."""
        buf = (ctypes.c_double * 3)()
        check(self._L.vs_facet_last_times(self._h, buf, 3))
        return {"screen_ms": float(buf[0]), "scan_ms": float(buf[1]), "readback_ms": float(buf[2])}

    def range_components(self, radius, sel=None):
        """Exact duplicate groups (``vs_range_components``, include/vs.h): the connected components of "within
        ``radius`` of each other" -- :meth:`range_search_rows`' predicate under ``self_mode="above"`` -- over
        the members: every stored row, under ``sel`` (as in :meth:`search`) the rows it allows.  Returns
        ``(labels, n_components, n_edges)``: ``labels`` int64 ``(ntotal,)``, a member's label the smallest id
        of its component and ``-1`` for a row that is no member; ``n_components`` counts singletons too;
        ``n_edges`` is the self-join's pair count.  Nothing grows with the number of pairs.  The labels of
        an unfiltered call are valid keys for :meth:`group_keys`."""
        r = float(range_radius(radius, 1)[0])  # (one scalar; NaN raises ValueError)
        labels = np.full((self.ntotal,), -1, dtype=np.int64)
        nc, ne = ctypes.c_int64(0), ctypes.c_int64(0)
        with self._sel(sel) as (_, sh):
            check(self._L.vs_range_components(self._h, sh, r, _ptr(labels) if labels.shape[0] else None,
                                              ctypes.byref(nc), ctypes.byref(ne)))
        return labels, int(nc.value), int(ne.value)

    def components_last_stats(self) -> dict:
        """The last :meth:`range_components`: members, edges, components, the tier taken, the queries the
        scan re-answered after a screen overflow and the query blocks (``vs_components_last_stats``)."""
        buf = (ctypes.c_int64 * 6)()
        check(self._L.vs_components_last_stats(self._h, buf, 6))
        return {"members": int(buf[0]), "edges": int(buf[1]), "components": int(buf[2]),
                "tier": {1: "scan", 2: "screen"}.get(int(buf[3]), "none"), "rescanned": int(buf[4]),
                "blocks": int(buf[5])}

    def components_last_times(self) -> dict:
        """HIP-event milliseconds of the last :meth:`range_components`: gather + screen + refine, scan,
        flatten + readback (``vs_components_last_times``)."""
        buf = (ctypes.c_double * 3)()
        check(self._L.vs_components_last_times(self._h, buf, 3))
        return {"screen_ms": float(buf[0]), "scan_ms": float(buf[1]), "readback_ms": float(buf[2])}

    def range_degrees(self, radius, sel=None):
        """Exact neighbour counts (``vs_range_degrees``, include/vs.h "density clusters"): for every member --
        every stored row, under ``sel`` the rows it allows -- the number of other members within ``radius``
        (:meth:`range_components`' relation).  Returns ``(degrees, n_edges)``: ``degrees`` int64 ``(ntotal,)``,
        ``-1`` for a row that is no member; the members' degrees sum to ``2 * n_edges``."""
        r = float(range_radius(radius, 1)[0])  # (one scalar; NaN raises ValueError)
        degrees = np.full((self.ntotal,), -1, dtype=np.int64)
        ne = ctypes.c_int64(0)
        with self._sel(sel) as (_, sh):
            check(self._L.vs_range_degrees(self._h, sh, r, _ptr(degrees) if degrees.shape[0] else None,
                                           ctypes.byref(ne)))
        return degrees, int(ne.value)

    def range_dbscan(self, radius, min_samples, sel=None):
        """Exact density clusters (``vs_range_dbscan``, include/vs.h): DBSCAN over the members with
        :meth:`range_components`' relation.  A member is core when it has at least ``min_samples`` members
        within ``radius``, itself included; clusters are the components of the core rows, labelled by their
        smallest core id; a non-core member with a core neighbour is a border row of its best core neighbour's
        cluster (the best score, ties to the lower id); the rest is noise.  Returns ``(labels, kinds,
        degrees, counts)``: ``labels`` int64 ``(ntotal,)``, ``-1`` for noise and non-members; ``kinds`` uint8
        (``0`` non-member, ``1`` noise, ``2`` border, ``3`` core); ``degrees`` as :meth:`range_degrees`;
        ``counts`` a dict of ``clusters``, ``core``, ``border``, ``noise`` and ``edges``."""
        r = float(range_radius(radius, 1)[0])
        ms = dbscan_min_samples(min_samples)
        n = self.ntotal
        labels = np.full((n,), -1, dtype=np.int64)
        kinds = np.zeros((n,), dtype=np.uint8)
        degrees = np.full((n,), -1, dtype=np.int64)
        cnt = (ctypes.c_int64 * 4)()
        ne = ctypes.c_int64(0)
        with self._sel(sel) as (_, sh):
            check(self._L.vs_range_dbscan(self._h, sh, r, ms, _ptr(labels) if n else None, _ptr(kinds) if n else None,
                                          _ptr(degrees) if n else None, cnt, ctypes.byref(ne)))
        return labels, kinds, degrees, {"clusters": int(cnt[0]), "core": int(cnt[1]), "border": int(cnt[2]),
                                        "noise": int(cnt[3]), "edges": int(ne.value)}

    def dbscan_last_stats(self) -> dict:
        """The last :meth:`range_degrees` / :meth:`range_dbscan`: members, edges, clusters, core, border and
        noise rows, the tier taken, per pass the queries given to the scan after a screen overflow and the
        query blocks run, and the queries pass 2 skipped (``vs_dbscan_last_stats``)."""
        buf = (ctypes.c_int64 * 12)()
        check(self._L.vs_dbscan_last_stats(self._h, buf, 12))
        return {"members": int(buf[0]), "edges": int(buf[1]), "clusters": int(buf[2]), "core": int(buf[3]),
                "border": int(buf[4]), "noise": int(buf[5]), "tier": {1: "scan", 2: "screen"}.get(int(buf[6]), "none"),
                "rescanned": int(buf[7]), "blocks": int(buf[8]), "rescanned2": int(buf[9]), "blocks2": int(buf[10]),
                "skipped": int(buf[11])}

    def dbscan_last_times(self) -> dict:
        """HIP-event milliseconds of the last :meth:`range_degrees` / :meth:`range_dbscan`: per pass gather +
        screen + refine and scan, then labels + readback (``vs_dbscan_last_times``)."""
        buf = (ctypes.c_double * 5)()
        check(self._L.vs_dbscan_last_times(self._h, buf, 5))
        return {"pass1_screen_ms": float(buf[0]), "pass1_scan_ms": float(buf[1]), "pass2_screen_ms": float(buf[2]),
                "pass2_scan_ms": float(buf[3]), "labels_ms": float(buf[4])}

    def selector(self, allowed) -> Selector:
        """A reusable :class:`Selector` over the rows present now (mask or ids, ``pack_allowed``)."""
        return Selector(self, allowed)

    def selector_from_range(self, q, radius, mode: str = "any", negate: bool = False, sel=None) -> Selector:
        """A :class:`Selector` built on the device from a score predicate (``vs_sel_from_range``,
        include/vs.h): the rows that pass ``radius`` -- :meth:`range_search`'s predicate, a scalar or one
        value per query -- for at least one query (``mode="any"``) or for every query (``"all"``); with
        ``negate`` the members that do not.  Members: every row present now, under ``sel`` (as in
        :meth:`search`) those it allows; the result is always a subset of them.  No row list is produced,
        sorted or shipped and there is no ``max_total``.  The result is an ordinary selector: pass it as
        ``sel=`` anywhere, combine it with ``&``, ``|``, ``-`` and ``~``."""
        q = self._queries(q, "selector_from_range")
        nq = q.shape[0]
        r = range_radius(radius, nq)
        code = selq_mode(mode)
        h = ctypes.c_void_p()
        with self._sel(sel) as (_, sh):
            check(self._L.vs_sel_from_range(self._h, sh, _ptr(q) if nq else None, nq, _ptr(r) if nq else None, code,
                                            int(bool(negate)), ctypes.byref(h)))
        return Selector._from_handle(self, h)

    def selector_from_range_rows(self, ids, radius, mode: str = "any", negate: bool = False, sel=None) -> Selector:
        """:meth:`selector_from_range` with stored rows as the queries (``vs_sel_from_range_rows``): query
        ``i`` is the stored value of row ``ids[i]``, gathered on the device.  A row passes its own
        predicate like any other row, so "everything near these rows" holds the rows themselves and, with
        ``negate``, "everything but what is near them" does not."""
        ids = row_ids(ids, 0)  # (the library bounds them; no check here touches the handle)
        n = ids.shape[0]
        r = range_radius(radius, n)
        code = selq_mode(mode)
        h = ctypes.c_void_p()
        with self._sel(sel) as (_, sh):
            check(self._L.vs_sel_from_range_rows(self._h, sh, _ptr(ids) if n else None, n, _ptr(r) if n else None, code,
                                                 int(bool(negate)), ctypes.byref(h)))
        return Selector._from_handle(self, h)

    def scoresel_last_stats(self) -> dict:
        """The last :meth:`selector_from_range` / ``_rows``: allowed rows, members, the tier taken, the
        queries the scan re-answered after a screen overflow and the query blocks
        (``vs_scoresel_last_stats``)."""
        buf = (ctypes.c_int64 * 5)()
        check(self._L.vs_scoresel_last_stats(self._h, buf, 5))
        return {"m": int(buf[0]), "members": int(buf[1]), "tier": {1: "scan", 2: "screen"}.get(int(buf[2]), "none"),
                "rescanned": int(buf[3]), "blocks": int(buf[4])}

    def scoresel_last_times(self) -> dict:
        """HIP-event milliseconds of the last :meth:`selector_from_range` / ``_rows``: screen + refine,
        scan (and the ALL fold), finish (``vs_scoresel_last_times``)."""
        buf = (ctypes.c_double * 3)()
        check(self._L.vs_scoresel_last_times(self._h, buf, 3))
        return {"screen_ms": float(buf[0]), "scan_ms": float(buf[1]), "finish_ms": float(buf[2])}

    def set_sel_mode(self, mode: str) -> None:
        """Force the tier of filtered searches (``"scan"``, ``"overfetch"``) or let the library choose
        (``"auto"``); results are the same bits under every mode (include/vs.h ``vs_set_sel_mode``)."""
        if mode not in SEL_MODES:
            raise ValueError(f"unknown selector mode {mode!r}")
        check(self._L.vs_set_sel_mode(self._h, SEL_MODES[mode]))

    def sel_last_stats(self) -> dict:
        """The last filtered search: allowed rows, tier taken, the overfetch depth k' and the queries
        the scan re-answered (include/vs.h ``vs_sel_last_stats``)."""
        buf = (ctypes.c_int64 * 4)()
        check(self._L.vs_sel_last_stats(self._h, buf, 4))
        return {"m": int(buf[0]), "tier": {1: "scan", 2: "overfetch"}.get(int(buf[1]), "none"),
                "kprime": int(buf[2]), "rescanned": int(buf[3])}

    def reconstruct(self, i: int) -> np.ndarray:
        out = np.empty((self.d,), dtype=np.float32)
        check(self._L.vs_reconstruct(self._h, int(i), _ptr(out)))
        return out

    def reconstruct_n(self, i0: int, n: int) -> np.ndarray:
        out = np.empty((int(n), self.d), dtype=np.float32)
        if n:
            check(self._L.vs_reconstruct_n(self._h, int(i0), int(n), _ptr(out)))
        return out

    def hnsw_prune(self, nodes, cand, W: int) -> np.ndarray:
        """faiss's HNSW neighbour selection per node on the GPU (include/vs.h ``vs_hnsw_prune``):
        ``cand`` (m x C distinct row ids, -1 padded at the end) -> (m x W) kept ids, -1 padded."""
        nodes = np.ascontiguousarray(nodes, dtype=np.int64)
        cand = np.ascontiguousarray(cand, dtype=np.int32)
        if cand.ndim != 2 or cand.shape[0] != nodes.shape[0]:
            raise ValueError("cand must be (len(nodes), C)")
        m, C = cand.shape
        out = np.full((m, int(W)), -1, dtype=np.int32)
        if m:
            check(self._L.vs_hnsw_prune(self._h, m, _ptr(nodes), _ptr(cand), int(C), int(W), _ptr(out)))
        return out

    def reset(self) -> None:
        check(self._L.vs_reset(self._h))

    def remove_ids(self, ids_or_mask) -> int:
        """faiss ``IndexFlat.remove_ids``: remove the given rows (a boolean mask over the rows or row
        ids, as :func:`pack_allowed` takes them) and return how many went.  The surviving rows keep
        their order and take ids ``0..ntotal-1``; the index then equals one built by ``add`` of the
        survivors.  A call that removes a row makes earlier :class:`Selector` objects and HNSW graphs
        stale (include/vs.h ``vs_remove_ids``); the capacity is kept."""
        return self.remove_bitmap(pack_allowed(self.ntotal, ids_or_mask))

    def remove_bitmap(self, bitmap) -> int:
        """:meth:`remove_ids` from a packed bitmap (``pack_allowed``'s layout, bit set = remove; bits
        past ``ntotal`` are ignored, a bitmap shorter than ``ceil(ntotal / 8)`` bytes is an argument
        error)."""
        bitmap = np.ascontiguousarray(bitmap, dtype=np.uint8)
        removed = ctypes.c_int64(0)
        check(self._L.vs_remove_ids(self._h, _ptr(bitmap), bitmap.shape[0], ctypes.byref(removed)))
        return int(removed.value)

    # -- screen selection ----------------------------------------------------------------------
    SCREENS = {"native": 0, "int8": 1}

    def set_screen(self, screen: str) -> None:
        """``"int8"``: keep an int8 copy of the rows and screen query batches with int8 MFMAs under
        a proven error bound (exact results, include/vs.h); ``"native"``: screen the stored rows."""
        if screen not in self.SCREENS:
            raise ValueError(f"unknown screen {screen!r}")
        check(self._L.vs_set_screen(self._h, self.SCREENS[screen]))

    @property
    def screen(self) -> str:
        v = int(self._L.vs_screen(self._h))
        return {0: "native", 1: "int8"}.get(v, "unknown")

    # -- persistence (faiss read_index / write_index payloads, streamed file <-> HBM) ---------------
    def add_from_file(self, path: str, byte_offset: int, n: int) -> None:
        """Append rows [0, n) of the row-major fp32 payload at ``byte_offset`` of ``path``."""
        check(self._L.vs_add_from_file(self._h, os.fsencode(path), int(byte_offset), int(n)))

    def write_rows(self, path: str, byte_offset: int, i0: int, n: int) -> None:
        """Write stored rows [i0, i0+n) as fp32 at ``byte_offset`` of ``path`` (no truncation)."""
        check(self._L.vs_write_rows_to_file(self._h, os.fsencode(path), int(byte_offset), int(i0), int(n)))

    # -- device-resident surface (bench / multi-GPU) -----------------------------------------
    def add_device(self, x_ptr: int, n: int, stream: Optional[int] = None) -> None:
        check(self._L.vs_add_device(self._h, x_ptr, int(n), stream or None))

    def add_synthetic(self, seed: int, global_row0: int, n: int, normalize: bool = True) -> None:
        check(self._L.vs_add_synthetic(self._h, int(seed), int(global_row0), int(n), int(bool(normalize))))

    def reserve(self, n: int) -> None:
        """Size the HBM row storage for ``n`` more rows in one allocation (no regrowth up to it)."""
        check(self._L.vs_reserve(self._h, int(n)))

    @property
    def capacity(self) -> int:
        return int(self._L.vs_capacity(self._h))

    def search_device(self, q_ptr: int, nq: int, k: int, D_ptr: Optional[int], I_ptr: int,
                      S64_ptr: Optional[int] = None, id_offset: int = 0, stream: Optional[int] = None) -> None:
        check(self._L.vs_search_device(self._h, q_ptr, int(nq), int(k), D_ptr or None, I_ptr, S64_ptr or None,
                                       int(id_offset), stream or None))

    def search_device_exact(self, q_ptr: int, nq: int, k: int, D_ptr: Optional[int], I_ptr: int,
                            S64_ptr: Optional[int] = None, id_offset: int = 0, stream: Optional[int] = None) -> None:
        """``search_device`` exact for every query: a failed certificate is re-searched by a fallback
        round queued on the device (no host sync), and a query even that round cannot certify (more
        near-tied rows than the deepest screen lists) by the exact full scan of the shard, counted in
        :meth:`full_scan_count`."""
        check(self._L.vs_search_device_exact(self._h, q_ptr, int(nq), int(k), D_ptr or None, I_ptr, S64_ptr or None,
                                             int(id_offset), stream or None))

    # -- two-phase search (the sharded step with a global T' exchange, include/vs.h) -------------
    def two_phase_ok(self, nq: int, k: int) -> bool:
        """Whether :meth:`search_phase_a` applies to a batch of ``nq`` queries at ``k`` (depends only
        on the index configuration, so every shard of a collective answers the same)."""
        return int(check(self._L.vs_two_phase_ok(self._h, int(nq), int(k)))) == 1

    def search_phase_a(self, q_ptr: int, nq: int, k: int, world: int, S_ptr: int, I_ptr: int, id_offset: int = 0,
                       stream: Optional[int] = None, stride: int = 1) -> int:
        """Phase A: this shard's best-so-far (S, I) lists for the exchange (``stride=2``: interleaved
        (score bits, id) pairs); returns the pending search for :meth:`search_phase_b` (or
        :meth:`search_pending_free`)."""
        out = ctypes.c_void_p(0)
        check(self._L.vs_search_device_phase_a(self._h, q_ptr, int(nq), int(k), int(world), int(id_offset), S_ptr,
                                               I_ptr, int(stride), stream or None, ctypes.byref(out)))
        return int(out.value)

    def search_phase_b(self, pending: int, floor_S_ptr: int, D_ptr: Optional[int], I_ptr: int,
                       S64_ptr: Optional[int] = None, stream: Optional[int] = None, stride: int = 1) -> None:
        """Phase B with the merged phase-A lists as the floor; frees the pending search."""
        check(self._L.vs_search_device_phase_b(ctypes.c_void_p(pending), floor_S_ptr, D_ptr or None, I_ptr,
                                               S64_ptr or None, int(stride), stream or None))

    def search_pending_free(self, pending: int) -> None:
        self._L.vs_search_pending_free(ctypes.c_void_p(pending))

    def set_timing(self, enable: bool) -> None:
        check(self._L.vs_set_timing(self._h, int(bool(enable))))

    def timing_fetch(self, cap: int = 4096):
        buf = (ctypes.c_float * cap)()
        kind = ctypes.c_int(0)
        n = check(self._L.vs_timing_fetch(self._h, buf, cap, ctypes.byref(kind)))
        return [float(buf[i]) for i in range(n)], {1: "mfma", 2: "gemv", 3: "mfma_i8", 4: "gemv_i8", 5: "full_scan"}.get(kind.value, "none")

    def uncertified_count(self) -> int:
        """First-pass certificate failures so far (each one was re-searched)."""
        return int(check(self._L.vs_uncertified_count(self._h)))

    def refine_rows_count(self) -> int:
        """Stored rows the adaptive exact refine has scored so far, over all queries (include/vs.h
        ``vs_refine_rows_count``)."""
        return int(check(self._L.vs_refine_rows_count(self._h)))

    def screen_state(self) -> dict:
        """The screen's state (include/vs.h ``vs_screen_state``): group residuals, the int8 margins'
        maxima and the screen-health feedback (int8 union depth, native routing, native seed depth)."""
        buf = (ctypes.c_double * 9)()
        check(self._L.vs_screen_state(self._h, buf, 9))
        keys = ("screen", "group_residuals", "groups_with_mean", "max_mean_norm", "max_code_norm",
                "max_row_error", "i8_union_log2", "i8_routed_searches", "native_seed_log2")
        return {k: (float(buf[i]) if "max" in k else int(buf[i])) for i, k in enumerate(keys)}

    def screen_probe(self, q_ptr: int, nq: int, screen: str, zero_queries: bool, stream: Optional[int] = None) -> float:
        """ms of one main-screen launch over the index with every threshold at +inf (no survivors),
        the query tile zeroed when ``zero_queries`` (include/vs.h ``vs_screen_probe``)."""
        ms = ctypes.c_float(0.0)
        check(self._L.vs_screen_probe(self._h, q_ptr, int(nq), FlatIndex.SCREENS[screen], int(bool(zero_queries)),
                                      stream or None, ctypes.byref(ms)))
        return float(ms.value)

    K1_PROBES = {"loads": 0, "lds": 1, "mfma": 2, "full": 3, "full_ms": 4, "full_prio": 5, "full_ms_prio": 6}

    def k1_probe(self, q_ptr: int, nq: int, screen: str, variant: str, zero_queries: bool, reps: int = 5,
                 stream: Optional[int] = None):
        """Diagnostic forms of the direct screen's loop (include/vs.h ``vs_k1_probe``): ``reps`` launches
        back to back -> (ms per launch, stamps [reps][G][4] uint64: s_memtime at the loop's start and
        end, s_memrealtime at the same points)."""
        import numpy as np
        ms = (ctypes.c_float * reps)()
        st = np.zeros((reps, 256, 4), dtype=np.uint64)
        G = ctypes.c_int32(0)
        check(self._L.vs_k1_probe(self._h, q_ptr, int(nq), FlatIndex.SCREENS[screen], FlatIndex.K1_PROBES[variant],
                                  int(bool(zero_queries)), int(reps), stream or None, ms, st.ctypes.data,
                                  ctypes.byref(G)))
        g = int(G.value)
        flat = st.reshape(-1)[: reps * g * 4].reshape(reps, g, 4)
        return [float(x) for x in ms], flat

    def set_scan_limit(self, nbytes: int) -> None:
        """Single-query calls over at most ``nbytes`` of stored rows use the exact full scan instead of
        a screen (include/vs.h ``vs_set_scan_limit``; 0 = always screen)."""
        check(self._L.vs_set_scan_limit(self._h, int(nbytes)))

    def full_scan_count(self) -> int:
        """Queries answered by the exact full scan so far: no bounded screen could certify them (more
        rows than KP_MAX tied within its margin).  Synchronises."""
        return int(check(self._L.vs_full_scan_count(self._h)))

    def host_staging_bytes(self) -> int:
        """Pinned host bytes held for ``search``'s query / result staging (bounded per context)."""
        return int(check(self._L.vs_host_staging_bytes(self._h)))

    def screen_copy_bytes(self) -> int:
        """HBM bytes of the int8 screen's copy (codes, per-row scale | error norm) on top of the
        stored rows; 0 on the native screen."""
        return int(check(self._L.vs_screen_copy_bytes(self._h)))

    # -- lifecycle ----------------------------------------------------------------------------
    def close(self) -> None:
        if self._h is not None and self._h.value:
            self._L.vs_destroy(self._h)
        self._h = None

    def __del__(self) -> None:  # pragma: no cover - interpreter shutdown ordering
        try:
            self.close()
        except Exception:
            pass


class MaskSelector:
    """:meth:`MultiDeviceFlatIndex.selector`: the packed bitmap of a filter over the rows present
    when it was made, kept on the host (the per-shard selectors are built per search)."""

    def __init__(self, n: int, allowed) -> None:
        self.n = int(n)
        self.bitmap = np.ascontiguousarray(pack_allowed(self.n, allowed))

    @property
    def count(self) -> int:
        return int(np.unpackbits(self.bitmap, bitorder="little")[: self.n].sum())

    def to_mask(self) -> np.ndarray:
        """The selector as a boolean mask over the rows it covers."""
        return np.unpackbits(self.bitmap, bitorder="little")[: self.n].astype(bool)

    def close(self) -> None:
        pass


class HostGroups:
    """:meth:`MultiDeviceFlatIndex.group_keys`: the group keys of the rows present when it was made,
    kept on the host (the device object is built on the one-device copy, per state of that copy)."""

    def __init__(self, n: int, keys) -> None:
        self.n = int(n)
        self.keys = group_key_array(keys, self.n)
        self._dev = None  # (the copy it was built on, its row count, Groups)

    @property
    def count(self) -> int:
        return int(np.unique(self.keys[self.keys >= 0]).shape[0])

    @property
    def rows(self) -> int:
        return self.n

    def on(self, copy: "FlatIndex") -> Groups:
        """The device groups on ``copy``; rows behind the covered ones get a key of their own (the
        caller's selector keeps them out of the member set)."""
        n = copy.ntotal
        if self._dev is None or self._dev[0] is not copy or self._dev[1] != n or self._dev[2]._h is None:
            self.close()
            keys = self.keys if n == self.n else np.concatenate([self.keys, np.full((n - self.n,), -1, dtype=np.int64)])
            self._dev = (copy, n, Groups(copy, keys))
        return self._dev[2]

    def close(self) -> None:
        dev, self._dev = self._dev, None
        if dev is not None:
            dev[2].close()


def merge_shards_device(metric_type: int, S_ptr: int, I_ptr: int, G: int, nq: int, k: int, S_out: int, I_out: int,
                        D_out: Optional[int] = None, stream: Optional[int] = None, in_stride: int = 1) -> None:
    """Merge G per-shard sorted (S64, id) lists [G][nq][k] on the device (after an all-gather);
    ``in_stride=2``: one interleaved array of (score bits, id) pairs (``I_ptr = S_ptr + 8``)."""
    L = _lib.load()
    check(L.vs_merge_shards_device(int(metric_type), S_ptr, I_ptr, int(in_stride), int(G), int(nq), int(k), S_out,
                                   I_out, D_out or None, stream or None))


def set_k1_schedule(schedule: int) -> None:
    """The K-step schedule of the int8 inner-product direct screen, process-wide (include/vs.h
    ``vs_set_k1_schedule``): 0 = a barrier at the head of every K-step, 1 (default) = the mid-step
    barrier.  Results are identical."""
    check(_lib.load().vs_set_k1_schedule(int(schedule)))


def k1_schedule() -> int:
    return int(_lib.load().vs_k1_schedule())


def set_i8_query_credit(on: bool) -> None:
    """The int8 screen's query credit, process-wide (include/vs.h ``vs_set_i8_query_credit``): on
    (default) = a query whose own int8 rounding error is below the share the rows' bounds carry for it
    refines fewer rows.  Results are identical."""
    check(_lib.load().vs_set_i8_query_credit(int(bool(on))))


def i8_query_credit() -> bool:
    return bool(_lib.load().vs_i8_query_credit())


REMOVE_STAGING_DEFAULT = 256 << 20


def set_remove_staging_bytes(nbytes: int = REMOVE_STAGING_DEFAULT) -> None:
    """Bytes of the bounce buffer a ``remove_ids`` may hold, process-wide (include/vs.h
    ``vs_set_remove_staging_bytes``): any value from 1 up, floored at one row tile of the index."""
    check(_lib.load().vs_set_remove_staging_bytes(int(nbytes)))


KMEANS_STAGING_DEFAULT = 256 << 20


def set_facet_staging_bytes(nbytes: int = FACET_STAGING_DEFAULT) -> None:
    """Bound, process-wide, of the counter table one query block of :meth:`FlatIndex.range_count` keeps on
    the device (``vs_set_facet_staging_bytes``; below one query's row of counters it acts as that row)."""
    nbytes = int(nbytes)
    if nbytes < 1:
        raise ValueError("facet staging bytes must be >= 1")
    check(_lib.load().vs_set_facet_staging_bytes(nbytes))


SCORESEL_STAGING_DEFAULT = 64 << 20


def set_scoresel_staging_bytes(nbytes: int = SCORESEL_STAGING_DEFAULT) -> None:
    """Bound, process-wide, of the per-query bitmaps one query block of an ``"all"``
    :meth:`FlatIndex.selector_from_range` keeps on the device (``vs_set_scoresel_staging_bytes``; below one
    query's bitmap it acts as that bitmap).  The same bits under every value."""
    nbytes = int(nbytes)
    if nbytes < 1:
        raise ValueError("score selector staging bytes must be >= 1")
    check(_lib.load().vs_set_scoresel_staging_bytes(nbytes))


def set_maxsim_staging_bytes(nbytes: int = MAXSIM_STAGING_DEFAULT) -> None:
    """Bound, process-wide, of the per-group table one query block of :meth:`FlatIndex.search_maxsim`'s scan
    keeps on the device (``vs_set_maxsim_staging_bytes``; below one query's table it acts as that table).
    The same bits under every value."""
    nbytes = int(nbytes)
    if nbytes < 1:
        raise ValueError("maxsim staging bytes must be >= 1")
    check(_lib.load().vs_set_maxsim_staging_bytes(nbytes))


def set_kmeans_staging_bytes(nbytes: int = KMEANS_STAGING_DEFAULT) -> None:
    """Bytes of gathered fp32 queries a ``kmeans`` / ``assign_rows`` call may hold at once, process-wide
    (include/vs.h ``vs_set_kmeans_staging_bytes``): any value from 1 up, floored at one 256-row block.
    The results are the same bits under every value."""
    check(_lib.load().vs_set_kmeans_staging_bytes(int(nbytes)))


def kmeans_last_times() -> dict:
    """The last ``vs_kmeans`` call of the process: ms in assignment, grouping and the update kernels
    (HIP events, summed over the passes), passes and updates run."""
    buf = (ctypes.c_double * 5)()
    check(_lib.load().vs_kmeans_last_times(buf, 5))
    return {"assign_ms": float(buf[0]), "group_ms": float(buf[1]), "update_ms": float(buf[2]),
            "passes": int(buf[3]), "updates": int(buf[4])}


def synthesize_device(device: int, seed: int, global_row0: int, n: int, d: int, out_ptr: int, normalize: bool = True,
                      dtype: str = "f32", stream: Optional[int] = None) -> None:
    """Write synthetic rows [global_row0, +n) as row-major fp32 (rounded to ``dtype``) to device
    memory -- the same counter-hash generator as ``FlatIndex.add_synthetic``."""
    L = _lib.load()
    check(L.vs_synthesize(int(device), int(seed), int(global_row0), int(n), int(d), int(bool(normalize)),
                          DTYPE_CODES[dtype], out_ptr, stream or None))


class MultiDeviceFlatIndex:
    """One exact flat index over several GPUs of this process (``vs_multi_*``, include/vs.h).

    The same faiss-IndexFlat-shaped surface as :class:`FlatIndex` (``ntotal``, ``d``,
    ``metric_type``, ``add``, ``search``, ``reconstruct``, ``reconstruct_n``, ``reset`` and the
    persistence hooks), so ``VectorStore`` holds it in ``.index`` unchanged; rows are dealt over the
    devices in chunks of 65,536 ids and every search merges the per-device exact top-k on
    ``devices[0]`` (the result equals one index over all rows).  A device may be listed more than
    once (several shards on one GPU).
    """

    def __init__(self, d: int, metric: str = "ip", dtype: str = "f32", devices=(0,)) -> None:
        self._h = None
        L = _lib.load()
        m = metric.lower()
        if m in ("ip", "cosine", "inner_product"):
            code = METRIC_IP
        elif m in ("l2", "euclidean"):
            code = METRIC_L2
        else:
            raise ValueError(f"unknown metric {metric!r}")
        if dtype not in DTYPE_CODES:
            raise ValueError(f"unknown dtype {dtype!r}")
        devs = [int(x) for x in devices]
        if not devs:
            raise ValueError("devices must name at least one GPU")
        arr = (ctypes.c_int * len(devs))(*devs)
        h = ctypes.c_void_p()
        check(L.vs_multi_create(int(d), code, DTYPE_CODES[dtype], len(devs), arr, ctypes.byref(h)))
        self._h = h
        self._L = L
        self.d = int(d)
        self.metric_type = code
        self.dtype = dtype
        self.devices = devs
        self._prune_copy = None  # (ntotal, FlatIndex on devices[0]) for hnsw_prune

    @property
    def ntotal(self) -> int:
        return int(self._L.vs_multi_ntotal(self._h))

    def shard_rows(self):
        return [int(self._L.vs_multi_shard_rows(self._h, g)) for g in range(len(self.devices))]

    def add(self, x) -> None:
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim != 2 or x.shape[1] != self.d:
            raise ValueError(f"add expects an (n, {self.d}) array, got {x.shape}")
        self._drop_prune_copy()
        check(self._L.vs_multi_add(self._h, _ptr(x), x.shape[0]))

    def search(self, q, k: int, sel=None) -> Tuple[np.ndarray, np.ndarray]:
        """Exact top-``k`` over all devices; ``sel`` (a boolean mask over the global ids, ids, or a
        :class:`MaskSelector` from :meth:`selector`): the exact top-``k`` among the allowed rows
        (``vs_multi_search_sel``)."""
        q = np.ascontiguousarray(q, dtype=np.float32)
        if q.ndim != 2 or q.shape[1] != self.d:
            raise ValueError(f"search expects an (nq, {self.d}) array, got {q.shape}")
        k = int(k)
        if k <= 0:
            raise _lib.VsError(_lib.VS_ERR_ARG, "k must be > 0")
        D = np.empty((q.shape[0], k), dtype=np.float32)
        I = np.empty((q.shape[0], k), dtype=np.int64)
        if sel is None:
            check(self._L.vs_multi_search(self._h, _ptr(q), q.shape[0], k, _ptr(D), _ptr(I)))
        else:  # (per-shard selectors are built per call)
            n = self.ntotal
            if isinstance(sel, MaskSelector):  # rows added after it was made are not selected
                bitmap = np.zeros(((n + 7) // 8,), dtype=np.uint8)
                bitmap[: sel.bitmap.shape[0]] = sel.bitmap[: bitmap.shape[0]]
            else:
                bitmap = np.ascontiguousarray(pack_allowed(n, sel))
            check(self._L.vs_multi_search_sel(self._h, _ptr(bitmap), bitmap.shape[0], _ptr(q), q.shape[0], k,
                                              _ptr(D), _ptr(I)))
        return D, I

    def range_search(self, q, radius, sel=None, max_total: Optional[int] = None):
        """:meth:`FlatIndex.range_search` over all devices (``vs_multi_range_search``): the result
        equals one index over all rows; ``sel`` as in :meth:`search`."""
        q = np.ascontiguousarray(q, dtype=np.float32)
        if q.ndim != 2 or q.shape[1] != self.d:
            raise ValueError(f"range_search expects an (nq, {self.d}) array, got {q.shape}")
        nq = q.shape[0]
        r = range_radius(radius, nq)
        cap = 0 if max_total is None else int(max_total)
        if max_total is not None and cap <= 0:
            raise ValueError("max_total must be > 0")
        bitmap = None
        if sel is not None:
            n = self.ntotal
            if isinstance(sel, MaskSelector):  # rows added after it was made are not selected
                bitmap = np.zeros(((n + 7) // 8,), dtype=np.uint8)
                bitmap[: sel.bitmap.shape[0]] = sel.bitmap[: bitmap.shape[0]]
            else:
                bitmap = np.ascontiguousarray(pack_allowed(n, sel))
        h = ctypes.c_void_p()
        check(self._L.vs_multi_range_search(self._h, _ptr(bitmap) if bitmap is not None else None,
                                            bitmap.shape[0] if bitmap is not None else 0, _ptr(q), nq, _ptr(r), cap,
                                            ctypes.byref(h)))
        return _take_range_result(self._L, h, nq)

    def selector(self, allowed) -> MaskSelector:
        """A reusable filter over the rows present now (mask or ids, ``pack_allowed``)."""
        return MaskSelector(self.ntotal, allowed)

    def _rows_as_queries(self, ids: np.ndarray) -> np.ndarray:
        n = self.ntotal
        if ids.size and (int(ids.min()) < 0 or int(ids.max()) >= n):
            raise _lib.VsError(_lib.VS_ERR_ARG, f"row ids must lie in [0, ntotal = {n})")
        q = np.empty((ids.shape[0], self.d), dtype=np.float32)
        for r0 in range(0, n, 65536):
            here = np.flatnonzero((ids >= r0) & (ids < r0 + 65536))
            if here.size:
                q[here] = self.reconstruct_n(r0, min(65536, n - r0))[ids[here] - r0]
        return q

    def search_rows(self, ids, k: int, sel=None, drop_self: bool = True) -> Tuple[np.ndarray, np.ndarray]:
        """:meth:`FlatIndex.search_rows` over all devices.  This route crosses the host: the rows come
        back through ``reconstruct_n``, go in again as the queries of :meth:`search` (one entry deeper
        under ``drop_self``) and the row itself is dropped on the host.  The bits are those of the
        one-device call, because ``reconstruct_n`` returns the stored values."""
        ids = row_ids(ids, self.ntotal)
        k = int(k)
        if k <= 0:
            raise _lib.VsError(_lib.VS_ERR_ARG, "k must be > 0")
        q = self._rows_as_queries(ids)
        if not drop_self or ids.shape[0] == 0:
            return self.search(q, k, sel=sel)
        D, I = self.search(q, min(k + 1, self.ntotal), sel=sel)
        return drop_self_topk(D, I, ids, k, self.metric_type)

    def range_search_rows(self, radius, ids=None, sel=None, self_mode: str = "above",
                          max_total: Optional[int] = None):
        """:meth:`FlatIndex.range_search_rows` over all devices.  This route crosses the host: the rows
        come back through ``reconstruct_n``, go in again as the queries of :meth:`range_search`, and the
        drop / above filter runs on the host (so ``max_total`` is checked against the filtered count
        here, after the unfiltered search).  Bit-equal to the one-device call."""
        if self_mode not in SELF_MODES:
            raise ValueError(f"unknown self_mode {self_mode!r}")
        if max_total is not None and int(max_total) <= 0:
            raise ValueError("max_total must be > 0")
        ids = np.arange(self.ntotal, dtype=np.int64) if ids is None else row_ids(ids, self.ntotal)
        r = range_radius(radius, ids.shape[0])
        lims, D, I = self.range_search(self._rows_as_queries(ids), r, sel=sel)
        lims, D, I = filter_range_self(lims, D, I, ids, SELF_MODES[self_mode])
        if max_total is not None and int(lims[-1]) > int(max_total):
            raise _lib.VsError(_lib.VS_ERR_ARG,
                               f"range search found {int(lims[-1])} results, max_total is {int(max_total)}")
        return lims, D, I

    def reconstruct_n(self, i0: int, n: int) -> np.ndarray:
        out = np.empty((int(n), self.d), dtype=np.float32)
        if n:
            check(self._L.vs_multi_reconstruct_n(self._h, int(i0), int(n), _ptr(out)))
        return out

    def reconstruct(self, i: int) -> np.ndarray:
        return self.reconstruct_n(int(i), 1)[0]

    def _one_device_copy(self) -> "FlatIndex":
        """A one-device copy of the rows on ``devices[0]`` for the HNSW kernels (they gather rows by
        id from one device's HBM).  Made once and kept until the rows change (a graph build calls
        the kernels several times per level)."""
        n = self.ntotal
        if self._prune_copy is None or self._prune_copy[0] != n:
            self._drop_prune_copy()
            tmp = FlatIndex(self.d, "ip" if self.metric_type == METRIC_IP else "l2", self.dtype, self.devices[0])
            try:
                tmp.reserve(n)
                for r0 in range(0, n, 65536):
                    tmp.add(self.reconstruct_n(r0, min(65536, n - r0)))
            except BaseException:
                tmp.close()
                raise
            self._prune_copy = (n, tmp)
        return self._prune_copy[1]

    def hnsw_prune(self, nodes, cand, W: int) -> np.ndarray:
        """:meth:`FlatIndex.hnsw_prune` on the one-device copy of the rows."""
        if len(nodes) == 0:
            return np.full((0, int(W)), -1, dtype=np.int32)
        return self._one_device_copy().hnsw_prune(nodes, cand, W)

    def kmeans(self, k: int, niter: int = 20, init=None, seed: int = 1234, sel=None, metric=None) -> KMeansResult:
        """:meth:`FlatIndex.kmeans` on the one-device copy of the rows (a multi-GPU k-means is not
        offered); ``sel``: a boolean mask, ids or a :class:`MaskSelector`."""
        kmeans_metric(metric, self.metric_type)
        if int(k) < 1:
            raise ValueError("k must be >= 1")
        if int(niter) < 0:
            raise ValueError("niter must be >= 0")
        kmeans_check_init(init, int(k), self.d)
        return self._one_device_copy().kmeans(k, niter, init, seed, self._copy_sel(sel), metric)

    def assign_rows(self, centroids, sel=None, metric=None) -> Tuple[np.ndarray, np.ndarray]:
        """:meth:`FlatIndex.assign_rows` on the one-device copy of the rows."""
        kmeans_metric(metric, self.metric_type)
        kmeans_centroids(centroids, self.d)
        return self._one_device_copy().assign_rows(centroids, self._copy_sel(sel), metric)

    def search_diverse(self, q, k: int, radius, sel=None) -> DiverseResult:
        """:meth:`FlatIndex.search_diverse` on the one-device copy of the rows (a multi-GPU walk is not
        offered); ``sel``: a boolean mask, ids or a :class:`MaskSelector`."""
        return self._one_device_copy().search_diverse(q, k, radius, self._copy_sel(sel))

    def group_keys(self, keys) -> HostGroups:
        """Reusable group keys over the rows present now (:meth:`FlatIndex.group_keys`)."""
        return HostGroups(self.ntotal, keys)

    def search_groups(self, q, k: int, groups: HostGroups, group_size: int = 1, sel=None) -> GroupedResult:
        """:meth:`FlatIndex.search_groups` on the one-device copy of the rows (a multi-GPU walk is not
        offered); ``sel``: a boolean mask, ids or a :class:`MaskSelector`."""
        if not isinstance(groups, HostGroups):
            raise TypeError("groups must come from this index's group_keys")
        n = self.ntotal
        if groups.n > n:
            raise _lib.VsError(_lib.VS_ERR_ARG, "stale groups (rows were removed after they were made)")
        copy = self._one_device_copy()
        s = self._copy_sel(sel)
        if groups.n < n:  # rows added behind the groups are no members
            mask = np.zeros((n,), dtype=bool)
            mask[:groups.n] = True
            if s is not None:
                mask &= np.unpackbits(pack_allowed(n, s), bitorder="little")[:n].astype(bool)
            s = mask
        return copy.search_groups(q, k, groups.on(copy), group_size, s)

    def range_count(self, q, radius, groups: Optional[HostGroups] = None, sel=None):
        """:meth:`FlatIndex.range_count` on the one-device copy of the rows (as :meth:`search_groups`);
        ``sel``: a boolean mask, ids or a :class:`MaskSelector`.  The columns of ``counts`` are the
        ascending distinct non-negative keys of ``groups``, then the ungrouped rows."""
        q = np.ascontiguousarray(q, dtype=np.float32)
        if q.ndim != 2 or q.shape[1] != self.d:
            raise ValueError(f"range_count expects an (nq, {self.d}) array, got {q.shape}")
        r = range_radius(radius, q.shape[0])
        if groups is not None and not isinstance(groups, HostGroups):
            raise TypeError("groups must come from this index's group_keys")
        n = self.ntotal
        if groups is not None and groups.n > n:
            raise _lib.VsError(_lib.VS_ERR_ARG, "stale groups (rows were removed after they were made)")
        copy = self._one_device_copy()
        s = self._copy_sel(sel)
        if groups is not None and groups.n < n:  # rows added behind the groups are no members
            mask = np.zeros((n,), dtype=bool)
            mask[:groups.n] = True
            if s is not None:
                mask &= np.unpackbits(pack_allowed(n, s), bitorder="little")[:n].astype(bool)
            s = mask
        return copy.range_count(q, r, None if groups is None else groups.on(copy), s)

    def range_components(self, radius, sel=None):
        """:meth:`FlatIndex.range_components` on the one-device copy of the rows (components need the edges
        between shards; a multi-GPU union is not offered); ``sel``: a boolean mask, ids or a
        :class:`MaskSelector`."""
        r = float(range_radius(radius, 1)[0])
        if self.ntotal == 0:
            return np.empty((0,), dtype=np.int64), 0, 0
        return self._one_device_copy().range_components(r, self._copy_sel(sel))

    def range_degrees(self, radius, sel=None):
        """:meth:`FlatIndex.range_degrees` on the one-device copy of the rows (as :meth:`range_components`)."""
        r = float(range_radius(radius, 1)[0])
        if self.ntotal == 0:
            return np.empty((0,), dtype=np.int64), 0
        return self._one_device_copy().range_degrees(r, self._copy_sel(sel))

    def range_dbscan(self, radius, min_samples, sel=None):
        """:meth:`FlatIndex.range_dbscan` on the one-device copy of the rows (as :meth:`range_components`)."""
        r = float(range_radius(radius, 1)[0])
        ms = dbscan_min_samples(min_samples)
        if self.ntotal == 0:
            return (np.empty((0,), dtype=np.int64), np.empty((0,), dtype=np.uint8), np.empty((0,), dtype=np.int64),
                    {"clusters": 0, "core": 0, "border": 0, "noise": 0, "edges": 0})
        return self._one_device_copy().range_dbscan(r, ms, self._copy_sel(sel))

    def _selector_on_copy(self, build, sel) -> MaskSelector:
        if self.ntotal == 0:
            return MaskSelector(0, np.zeros((0,), dtype=bool))
        copy = self._one_device_copy()
        s = build(copy, self._copy_sel(sel))
        try:
            return MaskSelector(s._n, s.to_mask())
        finally:
            s.close()

    def selector_from_range(self, q, radius, mode: str = "any", negate: bool = False, sel=None) -> MaskSelector:
        """:meth:`FlatIndex.selector_from_range` on the one-device copy of the rows (as :meth:`range_count`);
        ``sel``: a boolean mask, ids or a :class:`MaskSelector`.  The bitmap is read back: the result is a
        :class:`MaskSelector` for this index's own calls."""
        q = np.ascontiguousarray(q, dtype=np.float32)
        if q.ndim != 2 or q.shape[1] != self.d:
            raise ValueError(f"selector_from_range expects an (nq, {self.d}) array, got {q.shape}")
        r = range_radius(radius, q.shape[0])
        selq_mode(mode)
        return self._selector_on_copy(lambda c, s: c.selector_from_range(q, r, mode, negate, s), sel)

    def selector_from_range_rows(self, ids, radius, mode: str = "any", negate: bool = False, sel=None) -> MaskSelector:
        """:meth:`FlatIndex.selector_from_range_rows` on the one-device copy of the rows."""
        ids = row_ids(ids, 0)
        r = range_radius(radius, ids.shape[0])
        selq_mode(mode)
        if ids.size and (int(ids.min()) < 0 or int(ids.max()) >= self.ntotal):
            raise _lib.VsError(_lib.VS_ERR_ARG, f"row ids must lie in [0, ntotal = {self.ntotal})")
        return self._selector_on_copy(lambda c, s: c.selector_from_range_rows(ids, r, mode, negate, s), sel)

    def _copy_sel(self, sel):
        """A filter of this index as one over its one-device copy (rows added after a
        :class:`MaskSelector` was made are not selected)."""
        if not isinstance(sel, MaskSelector):
            return sel
        mask = np.zeros((self.ntotal,), dtype=bool)
        n = min(sel.n, mask.shape[0])
        mask[:n] = np.unpackbits(sel.bitmap, bitorder="little")[:n].astype(bool)
        return mask

    def hnsw_search(self, graph: dict, q: np.ndarray, k: int, ef: int) -> np.ndarray:
        """Ids (nq x k, -1 padded) of faiss's HNSW search over ``graph`` on the one-device copy of
        the rows (``hnsw.beam_search``: the insertion beam of a graph save)."""
        from .hnsw import HNSWGraph
        g = HNSWGraph(self._one_device_copy(), graph, ef)
        try:
            return g.search(q, k, ef)[1]
        finally:
            g.close()

    def _drop_prune_copy(self) -> None:
        pc, self._prune_copy = getattr(self, "_prune_copy", None), None
        if pc is not None:
            pc[1].close()

    def reset(self) -> None:
        self._drop_prune_copy()
        check(self._L.vs_multi_reset(self._h))

    def remove_ids(self, ids_or_mask) -> int:
        """:meth:`FlatIndex.remove_ids` over the devices, O(N) through the host: rows are dealt to
        the devices by global id chunk, so the shift crosses devices -- the survivors are read back
        (``reconstruct_n``), the index is reset and they are added again.  The stored values are
        what ``add`` stores of them, so the result equals one index built from the survivors."""
        n = self.ntotal
        remove = np.unpackbits(pack_allowed(n, ids_or_mask), bitorder="little")[:n].astype(bool)
        removed = int(remove.sum())
        if removed == 0:
            return 0
        keep = [self.reconstruct_n(r0, min(65536, n - r0))[~remove[r0:r0 + 65536]] for r0 in range(0, n, 65536)]
        self.reset()
        for rows in keep:
            if rows.shape[0]:
                self.add(np.ascontiguousarray(rows))
        return removed

    def set_screen(self, screen: str) -> None:
        if screen not in FlatIndex.SCREENS:
            raise ValueError(f"unknown screen {screen!r}")
        check(self._L.vs_multi_set_screen(self._h, FlatIndex.SCREENS[screen]))

    def add_from_file(self, path: str, byte_offset: int, n: int) -> None:
        self._drop_prune_copy()
        check(self._L.vs_multi_add_from_file(self._h, os.fsencode(path), int(byte_offset), int(n)))

    def write_rows(self, path: str, byte_offset: int, i0: int, n: int) -> None:
        check(self._L.vs_multi_write_rows_to_file(self._h, os.fsencode(path), int(byte_offset), int(i0), int(n)))

    def close(self) -> None:
        self._drop_prune_copy()
        if self._h is not None and self._h.value:
            self._L.vs_multi_destroy(self._h)
        self._h = None

    def __del__(self) -> None:  # pragma: no cover - interpreter shutdown ordering
        try:
            self.close()
        except Exception:
            pass

"""Drop-in ``VectorStore`` backed by the MI355X flat k-NN library.

Same class name, constructor keywords, methods, attributes, error types/messages and sidecar
files as /root/reference/utils/vector_store.py:15-280, so ``core/indexer.py`` and
``core/searcher.py`` run unchanged.  Integration: replace the reference's
``utils/vector_store.py`` body with ``from photo_search_engine_amd.vector_store import VectorStore``
(INTEGRATION.md).

What changes underneath:
  * ``self.index`` is a :class:`~photo_search_engine_amd.index.FlatIndex` (HBM-resident shard on
    one GPU) instead of a faiss CPU index; searches are exact (see include/vs.h).
  * ``index_type="hnsw"`` is accepted, validated and recorded in the sidecar exactly as before,
    and served by exact flat search by default (recall 1.0 >= HNSW); ``VECTOR_HNSW_SEARCH=graph``
    runs faiss's HNSW search instead, on the GPU (:class:`~photo_search_engine_amd.hnsw.HNSWGraph`)
    with ``efSearch = hnsw_ef_search`` as the reference sets it (utils/vector_store.py:77,135), over
    the graph of the loaded IHNf file or the one ``save()`` writes.  ``save()`` writes an IHNf file
    that the reference's faiss can load back: faiss's level draw, each node's neighbours chosen by
    faiss's selection heuristic (``HNSW::shrink_neighbor_list``, on the GPU) from exact candidates,
    reverse links as faiss's ``add_link`` adds them, + the flat storage (``_build_graph``).
    ``load()`` reads flat and HNSW files.
  * ``_embeddings`` caches only rows added in this process (a dict), not one Python list per row.
  * Bulk additions: :meth:`add` (n x d array) and :meth:`search_batch` (faiss (D, I) layout).

Normalisation stays on the host in numpy, bit-identical to the reference
(utils/vector_store.py:83-90), so stored vectors and query vectors are the same fp32 values.

Environment knobs (new, optional): ``VECTOR_DEVICE`` (GPU ordinal, default 0), ``VECTOR_DEVICES``
(e.g. ``0,1,2,3,4,5,6,7``: one index over those GPUs of this process, include/vs.h vs_multi_*),
``VECTOR_DTYPE`` (f32 | bf16 | f16 storage, default f32 = the reference's storage precision),
``VECTOR_SCREEN`` (int8 | native: the screen in front of the exact refine, either metric; default
int8 -- the certified int8 pre-screen, same exact results) and
``VECTOR_HNSW_SEARCH`` (exact | graph: how an ``index_type="hnsw"`` store searches).
"""
from __future__ import annotations

import json
import math
import os
import struct
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import faiss_format
from . import hnsw as hnsw_mod
from .hnsw import HNSWGraph
from .index import FlatIndex, MultiDeviceFlatIndex, pack_allowed

METRIC_INNER_PRODUCT = 0
METRIC_L2 = 1


def _default_index_factory(dimension: int, metric: str):
    dtype = (os.environ.get("VECTOR_DTYPE", "f32") or "f32").strip().lower()
    kind = "ip" if metric == "cosine" else "l2"
    devices = [d.strip() for d in (os.environ.get("VECTOR_DEVICES", "") or "").split(",") if d.strip()]
    if len(devices) > 1:  # one index over several GPUs of this process (rows dealt in 64k-id chunks)
        index = MultiDeviceFlatIndex(dimension, metric=kind, dtype=dtype, devices=[int(d) for d in devices])
    else:
        device = int(devices[0]) if devices else int(os.environ.get("VECTOR_DEVICE", "0") or 0)
        index = FlatIndex(dimension, metric=kind, dtype=dtype, device=device)
    # the certified int8 pre-screen unless VECTOR_SCREEN=native: results are exact either way (the
    # refine scores every candidate canonically and a certificate covers the rest), and the index
    # routes batches back to the native screen by itself on data denser than the int8 margins
    screen = (os.environ.get("VECTOR_SCREEN", "") or "").strip().lower() or "int8"
    index.set_screen(screen)
    return index


# Module-level hook: tests may substitute a checker-backed index with the same surface.
_index_factory = _default_index_factory


def _hnsw_graph_max_rows() -> int:
    """Rows of an ``index_type="hnsw"`` store whose graph is built at once from exact candidates
    (:meth:`VectorStore._build_graph`); rows beyond it are inserted into that graph in batches,
    faiss's way (:func:`hnsw.insert_rows`), so every save writes an IHNf file whatever the size."""
    return int(os.environ.get("VECTOR_HNSW_GRAPH_MAX_ROWS", "200000") or 200000)


_HNSW_EF_MAX = 2048  # largest max(efSearch, k) of the GPU graph search (include/vs.h)
# graph mode rebuilds the graph once the store holds this many times the rows the graph covers
_GRAPH_REBUILD_GROWTH = 1.25


def _merge_topk(D1: np.ndarray, I1: np.ndarray, D2: np.ndarray, I2: np.ndarray, k: int,
                higher_is_better: bool) -> Tuple[np.ndarray, np.ndarray]:
    """Per query, the best k of two (D, I) result lists (faiss layout, -1 padded): by score (IP:
    larger first; L2: smaller first), ties to the lower id, padding last.  The merge sees the fp32
    distances only, so two rows whose canonical fp64 scores differ but round to the same fp32 value
    are ordered by id here, where an exact search orders them by the fp64 score.  Only graph mode
    merges (its graph results with the exactly searched rows added behind the graph), and graph
    search is approximate to begin with."""
    D = np.concatenate([D1, D2], axis=1)
    I = np.concatenate([I1, I2], axis=1)
    key = -D if higher_is_better else D.copy()
    key = np.where(I >= 0, key, np.inf)
    order = np.lexsort((np.where(I >= 0, I, np.iinfo(np.int64).max), key), axis=1)[:, :k]
    Do = np.take_along_axis(D, order, axis=1)
    Io = np.take_along_axis(I, order, axis=1)
    if Do.shape[1] < k:  # fewer candidates than k: faiss padding
        pad = k - Do.shape[1]
        fill = np.float32(-np.finfo(np.float32).max if higher_is_better else np.finfo(np.float32).max)
        Do = np.concatenate([Do, np.full((Do.shape[0], pad), fill, dtype=Do.dtype)], axis=1)
        Io = np.concatenate([Io, np.full((Io.shape[0], pad), -1, dtype=Io.dtype)], axis=1)
    Do = np.where(Io >= 0, Do, np.float32(-np.finfo(np.float32).max if higher_is_better else np.finfo(np.float32).max))
    return Do.astype(np.float32), Io.astype(np.int64)


def hybrid_adjustment(keyword_score: Optional[float], boost: float, vector_weight: float,
                      keyword_weight: float) -> Tuple[float, float]:
    """``(scale, bias)`` of one item of :meth:`VectorStore.search_hybrid`, in cosine units: with a
    keyword hit ``A = b (wv D + wk (2 ks - 1)) + (b - 1)``, without ``A = b D + (b - 1)``; ``(1, 0)``
    for an item with no hit and ``b = 1``.  Python floats (the index rounds them to fp32)."""
    b = float(boost)
    if keyword_score is None:
        return b, b - 1.0
    return b * vector_weight, b * keyword_weight * (2.0 * float(keyword_score) - 1.0) + (b - 1.0)


def _hnsw_graph_search() -> bool:
    return (os.environ.get("VECTOR_HNSW_SEARCH", "exact") or "exact").strip().lower() == "graph"


class VectorStore:
    """
    向量存储与检索封装 (vector storage and retrieval).

    Attributes:
        dimension (Optional[int]): 向量维度
        index_path (str): 索引文件路径
        metadata_path (str): 元数据文件路径
    """

    def __init__(
        self,
        dimension: Optional[int],
        index_path: str,
        metadata_path: str,
        metric: str = "cosine",
        index_type: str = "flat",
        hnsw_m: int = 32,
        hnsw_ef_construction: int = 200,
        hnsw_ef_search: int = 96,
    ) -> None:
        # utils/vector_store.py:44-62
        self.dimension = dimension
        self.index_path = index_path
        self.metadata_path = metadata_path
        self.meta_path = f"{self.index_path}.meta.json"
        self.metric = metric.lower().strip() if metric else "l2"
        if self.metric not in {"l2", "cosine"}:
            raise ValueError("metric仅支持l2或cosine")
        self.index_type = (index_type or "flat").strip().lower()
        if self.index_type not in {"flat", "hnsw"}:
            raise ValueError("index_type仅支持flat或hnsw")
        self.hnsw_m = max(4, int(hnsw_m))
        self.hnsw_ef_construction = max(8, int(hnsw_ef_construction))
        self.hnsw_ef_search = max(8, int(hnsw_ef_search))

        self.index = self._create_index(dimension) if dimension else None
        self.metadata: List[Dict] = []
        self._normalize = self.metric == "cosine"
        self._embeddings: Dict[int, List[float]] = {}
        self._path_to_index: Dict[str, int] = {}
        # what the index file on disk holds, when it is known to be a prefix of this index
        # (set by save() / load(); None after clear()): lets save() append instead of rewriting
        self._persisted: Optional[Dict[str, Any]] = None
        # VECTOR_HNSW_SEARCH=graph: the graph arrays last loaded or saved, and its GPU copy
        self._graph_arrays: Optional[Dict[str, Any]] = None
        self._hnsw: Optional[HNSWGraph] = None
        self._graph_tail: Optional[FlatIndex] = None  # rows added behind the graph, searched exactly
        # a flat-configured store loaded from an HNSW file: the reference's index object stays an
        # IndexHNSWFlat (utils/vector_store.py:249), so its save() writes an HNSW file again
        self._file_hnsw = False
        # search_grouped: the index's group keys object of the field last grouped by, until the items change
        self._group_cache: Dict[str, Any] = {}

    # ------------------------------------------------------------------ internals
    def _rebuild_path_index(self) -> None:
        path_to_index: Dict[str, int] = {}
        for index, metadata in enumerate(self.metadata):
            photo_path = metadata.get("photo_path")
            if isinstance(photo_path, str) and photo_path:
                path_to_index[photo_path] = index
        self._path_to_index = path_to_index

    def _create_index(self, dimension: int):
        return _index_factory(int(dimension), self.metric)

    def _normalize_vector(self, vector: List[float]) -> List[float]:
        # utils/vector_store.py:83-90, verbatim semantics (fp32, np.linalg.norm, zero passthrough)
        if not self._normalize:
            return vector
        array = np.array(vector, dtype="float32")
        norm = np.linalg.norm(array)
        if norm == 0:
            return vector
        return (array / norm).astype("float32").tolist()

    def _normalize_query(self, vector) -> np.ndarray:
        """``np.array([_normalize_vector(vector)], dtype="float32")`` without the Python-list round trip
        (~0.19 ms of a 0.5 ms call at d=4096): fp32 -> Python float -> fp32 is exact, so the bits
        are the same.  A list of Python numbers is converted by ``struct`` (the same C double ->
        float cast as numpy's, ~3x faster than ``np.array`` on a list: ~24 vs ~70 us at d=1536); a
        value beyond the fp32 range (numpy makes it inf) or anything else takes ``np.array``.
        Anything but a flat vector takes the reference's own expression (whose extra axes the index
        then rejects, as faiss does)."""
        array = None
        if type(vector) is list:
            try:
                array = np.frombuffer(struct.pack(f"{len(vector)}f", *vector), dtype=np.float32)
            except (struct.error, OverflowError, TypeError):
                array = None
        if array is None:
            array = np.array(vector, dtype="float32")
        if array.ndim != 1:
            return np.array([self._normalize_vector(vector)], dtype="float32")
        if self._normalize:
            norm = np.linalg.norm(array)
            if norm != 0:
                array = (array / norm).astype("float32")
        return array.reshape(1, -1)

    def _normalize_rows(self, rows: np.ndarray) -> np.ndarray:
        """Bulk form of ``_normalize_vector``: each row normalised exactly as the single-row path
        (same numpy calls per row, so the stored bits are identical)."""
        rows = np.array(rows, dtype="float32", copy=True)
        if not self._normalize:
            return rows
        for i in range(rows.shape[0]):
            norm = np.linalg.norm(rows[i])
            if norm != 0:
                rows[i] = (rows[i] / norm).astype("float32")
        return rows

    def _write_index_meta(self) -> None:
        payload = {
            "index_type": self.index_type,
            "metric": self.metric,
            "dimension": self.dimension,
            "hnsw_m": self.hnsw_m,
            "hnsw_ef_construction": self.hnsw_ef_construction,
            "hnsw_ef_search": self.hnsw_ef_search,
        }
        with open(self.meta_path, "w", encoding="utf-8") as file:
            json.dump(payload, file, ensure_ascii=False, indent=2)

    def _load_index_meta(self) -> Dict[str, Any]:
        if not os.path.exists(self.meta_path):
            raise ValueError("索引元信息缺失，请重新构建索引")
        with open(self.meta_path, "r", encoding="utf-8") as file:
            payload = json.load(file)
        if not isinstance(payload, dict):
            raise ValueError("索引元信息损坏，请重新构建索引")
        return payload

    def _validate_loaded_index(self, payload: Dict[str, Any], loaded: "faiss_format.FaissFile") -> None:
        # utils/vector_store.py:125-140, rule for rule: the sidecar's index_type and metric must match
        # the configuration; an HNSW configuration needs an HNSW file (IndexHNSWFlat, :137-138) and
        # never checks the file's metric; a flat configuration checks only the file's metric_type
        # (:139-143), so an HNSW file of the configured metric loads too.
        index_type = str(payload.get("index_type") or "").strip().lower()
        metric = str(payload.get("metric") or "").strip().lower()
        if index_type != self.index_type:
            raise ValueError("索引类型与配置不一致，请重新构建索引")
        if metric != self.metric:
            raise ValueError("索引度量与配置不一致，请重新构建索引")
        if self.index_type == "hnsw":
            if loaded.kind != "hnsw":
                raise ValueError("索引结构与配置不一致，请重新构建索引")
        elif self.index_type == "flat":
            want = METRIC_INNER_PRODUCT if self.metric == "cosine" else METRIC_L2
            if loaded.metric_type != want:
                raise ValueError("索引度量与配置不一致，请重新构建索引")

    # ------------------------------------------------------------------ reference API
    # 内部接口：仅允许indexer模块调用，禁止直接暴露给前端
    def add_item(self, embedding: List[float], metadata: Dict) -> None:
        """写入向量与元数据 (utils/vector_store.py:143-169)."""
        if embedding is None:
            raise ValueError("向量不能为空")
        if self.index is None:
            self.dimension = len(embedding)
            self.index = self._create_index(self.dimension)
        if len(embedding) != self.dimension:
            raise ValueError(f"向量维度不匹配: {len(embedding)} != {self.dimension}")

        normalized = self._normalize_vector(embedding)
        vector = np.array([normalized], dtype="float32")
        self._drop_group_cache()
        self.index.add(vector)
        self.metadata.append(metadata)
        self._embeddings[len(self.metadata) - 1] = normalized
        photo_path = metadata.get("photo_path")
        if isinstance(photo_path, str) and photo_path:
            self._path_to_index[photo_path] = len(self.metadata) - 1

    # 内部接口：仅允许searcher模块调用，禁止前端直接访问向量数据库
    def search(self, query_embedding: List[float], top_k: int, allowed=None) -> List[Dict]:
        """相似度检索 (utils/vector_store.py:172-198).

        ``allowed`` (an addition at the boundary; ``None`` = the reference's call, untouched): the
        exact ``top_k`` among the allowed items only -- a :class:`~.index.Selector` from
        :meth:`selector`, a boolean mask over the items, item ids, or a predicate applied to each
        item's metadata.  The reference body (guards, ``k = min(top_k, ntotal)``, normalisation,
        ``-1`` filtering, result dicts) around faiss's ``search(..., params=SearchParameters(sel=
        IDSelectorBitmap(...)))``: a filter matching fewer than ``top_k`` items returns them all,
        and one matching enough never returns fewer than ``top_k`` (what over-fetching and
        post-filtering cannot promise, core/searcher.py:771-820, :573-603).  HNSW stores with
        ``VECTOR_HNSW_SEARCH=graph`` answer filtered calls exactly through the flat path, as
        multi-GPU indexes answer every call."""
        if self.index is None or self.index.ntotal == 0:
            return []
        if len(query_embedding) != self.dimension:
            raise ValueError(f"向量维度不匹配: {len(query_embedding)} != {self.dimension}")

        k = min(top_k, self.index.ntotal)
        if allowed is None:
            distances, indices = self._search_rows(self._normalize_query(query_embedding), k)
        else:
            distances, indices = self.index.search(self._normalize_query(query_embedding), k,
                                                   sel=self._allowed_rows(allowed))

        results: List[Dict] = []
        for distance, index in zip(distances[0].tolist(), indices[0].tolist()):
            if index == -1:
                continue
            results.append({"metadata": self.metadata[index], "distance": float(distance)})
        return results

    def search_diverse(self, query_embedding: List[float], top_k: int, threshold: float, allowed=None) -> List[Dict]:
        """:meth:`search` with look-alikes collapsed (an addition at the boundary): the best ``top_k``
        items, one per group of near-duplicates, each with the number of look-alikes it stands for --
        ``{"metadata", "distance", "similar_hidden": n}``.  The exact ranking is walked best first; an
        item is returned iff it is closer than ``threshold`` (:meth:`duplicate_pairs`' meaning: above
        it for cosine, below it for L2) to no item returned before it, otherwise it is counted under
        the earliest such item.  A burst of twelve frames then fills one slot, not ten, and the page
        needs none of the reference's refill rounds (core/searcher.py:242 merges equal paths only;
        :1157-1211 and :1352-1458 re-search with a larger ``candidate_k``).  The guards, the
        normalisation and the ``k = min(top_k, ntotal)`` clamp are :meth:`search`'s; ``allowed`` as
        there.  HNSW stores answer through the exact flat path, as filtered calls do."""
        if self.index is None or self.index.ntotal == 0:
            return []
        if len(query_embedding) != self.dimension:
            raise ValueError(f"向量维度不匹配: {len(query_embedding)} != {self.dimension}")
        k = min(top_k, self.index.ntotal)
        sel = None if allowed is None else self._allowed_rows(allowed)
        res = self.index.search_diverse(self._normalize_query(query_embedding), k, float(threshold), sel=sel)
        return [{"metadata": self.metadata[index], "distance": float(distance), "similar_hidden": int(hidden)}
                for distance, index, hidden in zip(res.D[0].tolist(), res.I[0].tolist(), res.hidden[0].tolist())
                if index != -1]

    def search_grouped(self, query_embedding: List[float], top_k: int, group_by, group_size: int = 1,
                       allowed=None) -> List[Dict]:
        """:meth:`search` with the items that belong together by a key collapsed (an addition at the
        boundary; Milvus ``group_by_field``, Qdrant ``search_groups``, Elasticsearch ``collapse`` with
        ``inner_hits``): the best ``top_k`` groups -- one per shooting day, folder, event, person or file
        hash -- ordered by their best item, each with its best ``group_size`` items, as
        ``{"group": value, "size": n, "items": [{"metadata", "distance"}, ...]}``; ``size`` is the number
        of items the group has (under ``allowed``), for a "12 photos from this day" label.  The answer
        is exact at any depth and needs none of the reference's over-fetching and refill rounds
        (core/searcher.py:242 merges equal paths after fetching ``candidate_k`` rows; :1157-1211 and
        :1352-1458 re-search to fill the page back up).

        ``group_by``: a metadata field name (an item without the field, or with ``None`` in it, is
        ungrouped: a group of its own, reported with ``"group": None``); a callable ``metadata ->
        hashable | None``; or a sequence of one int per item (negative = ungrouped).  Values are coded
        to int64 in order of first appearance; the device copy of a field's keys is cached until the
        items change.  The guards, the normalisation and the ``k = min(top_k, ntotal)`` clamp are
        :meth:`search`'s; ``allowed`` as there; ``k * group_size`` beyond 3276 (the index's depth
        limit) raises ``ValueError``.  HNSW stores answer through the exact flat path, as filtered
        calls do."""
        if self.index is None or self.index.ntotal == 0:
            return []
        if len(query_embedding) != self.dimension:
            raise ValueError(f"向量维度不匹配: {len(query_embedding)} != {self.dimension}")
        n = int(self.index.ntotal)
        k, g = min(int(top_k), n), int(group_size)
        if k < 1 or g < 1:
            raise ValueError("top_k and group_size must be >= 1")
        if k * g > 3276:
            raise ValueError(f"top_k * group_size = {k * g} exceeds 3276")
        groups, values, own = self._group_keys(group_by, n)
        try:
            sel = None if allowed is None else self._allowed_rows(allowed)
            res = self.index.search_groups(self._normalize_query(query_embedding), k, groups, group_size=g, sel=sel)
        finally:
            if own:
                groups.close()
        out: List[Dict] = []
        for slot in range(k):
            found = int(res.found[0, slot])
            if found == 0:
                break
            key = int(res.keys[0, slot])
            items = [{"metadata": self.metadata[index], "distance": float(distance)}
                     for distance, index in zip(res.D[0, slot, :found].tolist(), res.I[0, slot, :found].tolist())]
            out.append({"group": (key if values is None else values[key]) if key >= 0 else None, "size": int(res.sizes[0, slot]), "items": items})
        return out

    def search_hybrid(self, query_embedding: List[float], top_k: int, keyword_scores: Dict[str, float],
                      vector_weight: float = 0.8, keyword_weight: float = 0.2, boosts=None, allowed=None) -> List[Dict]:
        """:meth:`search` ranked by the fused score of the reference's hybrid search (an addition at the
        boundary; Elasticsearch ``knn`` + ``boost`` / ``function_score``, Milvus's boost ranker, Qdrant's
        score-boosting formula): the vector score mixed with the keyword store's score for the photos
        that store returned, times a metadata boost (core/searcher.py:925-988, ``_compute_metadata_boost``
        :435-449).  The reference fuses only its ``candidate_k`` vector hits, so a photo with a strong
        keyword hit or a boost just outside them is lost, or enters at ``x 0.65`` with no vector score;
        here every item is ranked by its fused score, exactly.

        Cosine stores only (``ValueError`` on an L2 store: the reference's L2 map is an exponential, not
        affine).  In cosine units, with ``D`` the cosine, ``ks`` an item's keyword score and ``b`` its
        boost: ``A = b (wv D + wk (2 ks - 1)) + (b - 1)`` with a keyword hit, ``A = b D + (b - 1)``
        without; an item with no hit and ``b = 1`` keeps ``A = D``, so a typical query adjusts only the
        keyword store's hits and the boosted items.  Each result is ``{"metadata", "score": (A + 1) / 2,
        "vector_score": (D + 1) / 2, "keyword_score": ks or None}``.  This is the linear part of the
        reference's ``_distance_to_score``: its stretch above 0.7 and its rounding are not reproduced.

        ``keyword_scores``: ``{photo_path: score}``; paths the store does not hold are ignored, as the
        reference ignores keyword hits absent from the local index (:943-946).  ``boosts``: ``{photo_path:
        factor}`` or a callable ``metadata -> factor`` (``None`` = 1).  Weights and factors must be finite
        and ``>= 0``.  The guards, the normalisation and the ``k = min(top_k, ntotal)`` clamp are
        :meth:`search`'s; ``allowed`` as there."""
        if self.metric != "cosine":
            raise ValueError("search_hybrid needs a cosine store (the L2 score map is not affine)")
        wv, wk = float(vector_weight), float(keyword_weight)
        if not (math.isfinite(wv) and math.isfinite(wk) and wv >= 0 and wk >= 0):
            raise ValueError("vector_weight and keyword_weight must be finite and >= 0")
        if self.index is None or self.index.ntotal == 0:
            return []
        if len(query_embedding) != self.dimension:
            raise ValueError(f"向量维度不匹配: {len(query_embedding)} != {self.dimension}")
        if not hasattr(self.index, "score_adjust_sparse"):
            raise NotImplementedError("search_hybrid needs a one-device flat index")
        n = int(self.index.ntotal)
        k = min(int(top_k), n)
        if k < 1:
            raise ValueError("top_k must be >= 1")
        hits: Dict[int, float] = {}
        for path, ks in (keyword_scores or {}).items():
            row = self._path_to_index.get(path)
            if row is not None and row < n:
                hits[row] = float(ks)
        factor: Dict[int, float] = {}
        if callable(boosts):
            for row, metadata in enumerate(self.metadata[:n]):
                b = boosts(metadata)
                if b is not None and float(b) != 1.0:
                    factor[row] = float(b)
        elif boosts:
            for path, b in boosts.items():
                row = self._path_to_index.get(path)
                if row is not None and row < n and float(b) != 1.0:
                    factor[row] = float(b)
        rows = sorted(set(hits) | set(factor))
        scale = np.empty((len(rows),), dtype=np.float32)
        bias = np.empty((len(rows),), dtype=np.float32)
        for j, row in enumerate(rows):
            scale[j], bias[j] = hybrid_adjustment(hits.get(row), factor.get(row, 1.0), wv, wk)
        if not (np.all(np.isfinite(scale)) and np.all(np.isfinite(bias)) and np.all(scale >= 0)):
            raise ValueError("keyword scores must be finite, boosts finite and >= 0")
        adjust = self.index.score_adjust_sparse(np.asarray(rows, dtype=np.int64), scale, bias)
        try:
            sel = None if allowed is None else self._allowed_rows(allowed)
            A, I, D = self.index.search_adjusted(self._normalize_query(query_embedding), k, adjust, sel=sel,
                                                 return_raw=True)
        finally:
            adjust.close()
        return [{"metadata": self.metadata[index], "score": (float(a) + 1.0) / 2.0,
                 "vector_score": (float(d) + 1.0) / 2.0, "keyword_score": hits.get(index)}
                for a, index, d in zip(A[0].tolist(), I[0].tolist(), D[0].tolist()) if index != -1]

    def search_any(self, query_embeddings: List[List[float]], top_k: int, allowed=None) -> List[Dict]:
        """:meth:`search` with several embeddings of one request -- its alternative wordings (an addition at
        the boundary; Milvus ``hybrid_search``, Qdrant prefetch + fusion, Elasticsearch's multiple ``knn``
        clauses): every item ranked by its best score over the embeddings, exactly, in one call.  It is
        what the reference assembles from one :meth:`search` per wording and a merge in Python that keeps
        a photo's higher score (core/searcher.py ``_maybe_expand_query_results`` :1352-1458,
        ``_maybe_reflect_query_results`` :1219-1298, ``_deduplicate_results`` :242-261).  Each result is
        :meth:`search`'s dict (``distance`` = the best score) plus ``"matched_query"``, the index of the
        first embedding that gives that score, and ``"distances"``, the item's score under every
        embedding.  Each embedding is normalised as :meth:`search` normalises its one; the guards and the
        ``k = min(top_k, ntotal)`` clamp are :meth:`search`'s; ``allowed`` as there.  An empty list of
        embeddings raises ``ValueError``; at most 8 embeddings, and ``top_k`` at most
        ``min(3276, 8192 // len(query_embeddings))``."""
        return self._search_fused(query_embeddings, top_k, "any", allowed)

    def search_all(self, query_embeddings: List[List[float]], top_k: int, allowed=None) -> List[Dict]:
        """:meth:`search_any` for a compound request ("dog *and* beach"): every item ranked by its worst
        score over the embeddings, so an item is as good as its weakest concept.  No merge of per-concept
        lists gives this ranking -- an item good on every concept can be outside each concept's list --
        but the index ranks every item.  Results as :meth:`search_any` (``distance`` = the worst score,
        ``matched_query`` = the concept that gives it)."""
        return self._search_fused(query_embeddings, top_k, "all", allowed)

    def _search_fused(self, query_embeddings, top_k: int, mode: str, allowed) -> List[Dict]:
        embeddings = list(query_embeddings)
        if not embeddings:
            raise ValueError("query_embeddings must hold at least one embedding")
        if self.index is None or self.index.ntotal == 0:
            return []
        for embedding in embeddings:
            if len(embedding) != self.dimension:
                raise ValueError(f"向量维度不匹配: {len(embedding)} != {self.dimension}")
        if not hasattr(self.index, "search_fused"):
            raise NotImplementedError("search_any / search_all need a one-device flat index")
        k = min(int(top_k), int(self.index.ntotal))
        q = np.stack([self._normalize_query(embedding)[0] for embedding in embeddings])[None, :, :]
        sel = None if allowed is None else self._allowed_rows(allowed)
        D, I, W, U = self.index.search_fused(q, k, mode=mode, sel=sel, return_sub=True)
        return [{"metadata": self.metadata[index], "distance": float(distance), "matched_query": int(which),
                 "distances": [float(s) for s in sub]}
                for distance, index, which, sub in zip(D[0].tolist(), I[0].tolist(), W[0].tolist(), U[0].tolist())
                if index != -1]

    def search_multivector(self, query_embeddings: List[List[float]], top_k: int, group_by, allowed=None) -> List[Dict]:
        """Groups ranked by several embeddings at once (an addition at the boundary; Qdrant multivectors
        ``max_sim``, Milvus embedding lists, Weaviate multi-vector, Vespa tensors): "the trip with mountains,
        a lake and a campfire" -- each concept matched by *some* item of the group.  A group's score is the
        sum over the embeddings of the best score any of its items reaches (MaxSim, late interaction),
        exact: a group mediocre on every concept can be outside every per-concept top-k list and still win,
        so no merge of :meth:`search` results gives this ranking.  Returns the best ``top_k`` groups as
        ``{"group": value, "score": float, "size": n, "matches": [{"metadata", "distance"}, ...]}`` with one
        match per embedding, the group's best item under it (the earliest item among equals); ``size`` is
        the number of items the group has (under ``allowed``).

        ``group_by`` as in :meth:`search_grouped` (ungrouped items are groups of their own, reported with
        ``"group": None``); each embedding is normalised as :meth:`search` normalises its one; the guards
        and the ``k = min(top_k, ntotal)`` clamp are :meth:`search`'s; ``allowed`` as there.  An empty list
        of embeddings raises ``ValueError``; at most 8 embeddings, and ``k`` beyond
        ``min(3276, 8192 // len(query_embeddings))`` raises ``ValueError``.  HNSW stores answer through the
        exact flat path, as filtered calls do."""
        embeddings = list(query_embeddings)
        if not embeddings:
            raise ValueError("query_embeddings must hold at least one embedding")
        if len(embeddings) > 8:
            raise ValueError(f"search_multivector takes at most 8 embeddings, got {len(embeddings)}")
        if self.index is None or self.index.ntotal == 0:
            return []
        for embedding in embeddings:
            if len(embedding) != self.dimension:
                raise ValueError(f"向量维度不匹配: {len(embedding)} != {self.dimension}")
        if not hasattr(self.index, "search_maxsim"):
            raise NotImplementedError("search_multivector needs a one-device flat index")
        n = int(self.index.ntotal)
        k, limit = min(int(top_k), n), min(3276, 8192 // len(embeddings))
        if k < 1:
            raise ValueError("top_k must be >= 1")
        if k > limit:
            raise ValueError(f"top_k = {k} exceeds {limit} at {len(embeddings)} embeddings")
        q = np.stack([self._normalize_query(embedding)[0] for embedding in embeddings])[None, :, :]
        groups, values, own = self._group_keys(group_by, n)
        try:
            sel = None if allowed is None else self._allowed_rows(allowed)
            res = self.index.search_maxsim(q, k, groups, sel=sel)
        finally:
            if own:
                groups.close()
        out: List[Dict] = []
        for slot in range(k):
            size = int(res.sizes[0, slot])
            if size == 0:
                break
            key = int(res.keys[0, slot])
            matches = [{"metadata": self.metadata[index], "distance": float(distance)}
                       for distance, index in zip(res.sub_scores[0, slot].tolist(), res.sub_ids[0, slot].tolist())]
            out.append({"group": (key if values is None else values[key]) if key >= 0 else None,
                        "score": float(res.scores[0, slot]), "size": size, "matches": matches})
        return out

    def search_page(self, query_embedding: List[float], top_k: int, after=None, allowed=None) -> List[Dict]:
        """:meth:`search` continued (an addition at the boundary; Elasticsearch ``search_after``, Qdrant and
        Milvus ``offset``, Weaviate ``after``): the ``top_k`` items that follow ``after`` in the exact
        ranking -- a "load more" page at any depth, with no ``top_k = offset + page`` re-search and no limit
        at 3276.  ``after`` is the photo path of the last item shown, or that item's result dict from the
        previous page (its ``"rank"`` then tells the index where the page lies); ``None`` starts from the
        top, where the page is :meth:`search`'s.  Each result is :meth:`search`'s dict plus ``"rank"``, the
        item's 0-based position in the ranking (among the ``allowed`` items).  The item ``after`` names need
        not pass ``allowed``: its position in the ranking is defined either way.  Pages chained this way
        never repeat or skip an item, ties included; a page shorter than ``top_k`` is the last.  The same
        ``query_embedding`` and ``allowed`` must be passed on every page.  The guards, the normalisation and
        the ``k = min(top_k, ntotal)`` clamp are :meth:`search`'s; ``allowed`` as there; a path the store does
        not hold raises ``ValueError``.  HNSW stores answer through the exact flat path, as filtered calls
        do."""
        if self.index is None or self.index.ntotal == 0:
            return []
        if len(query_embedding) != self.dimension:
            raise ValueError(f"向量维度不匹配: {len(query_embedding)} != {self.dimension}")
        if not hasattr(self.index, "search_after"):
            raise NotImplementedError("search_page needs a one-device flat index")
        n = int(self.index.ntotal)
        k = min(int(top_k), n)
        cursor, hint = -1, 0
        if after is not None:
            path, hint = after, -1
            if isinstance(after, dict):
                metadata = after.get("metadata")
                path = metadata.get("photo_path") if isinstance(metadata, dict) else None
                if isinstance(after.get("rank"), int):
                    hint = int(after["rank"]) + 1
            row = self._path_to_index.get(path) if isinstance(path, str) else None
            if row is None or row >= n:
                raise ValueError(f"search_page: no item with photo path {path!r}")
            cursor = int(row)
        sel = None if allowed is None else self._allowed_rows(allowed)
        D, I, rank = self.index.search_after(self._normalize_query(query_embedding), k, cursor, sel=sel,
                                             rank_hint=hint, return_rank=True)
        return [{"metadata": self.metadata[index], "distance": float(distance), "rank": int(rank[0]) + j}
                for j, (distance, index) in enumerate(zip(D[0].tolist(), I[0].tolist())) if index != -1]

    def iter_search(self, query_embedding: List[float], page_size: int, allowed=None):
        """Generator over :meth:`search_page`: pages of ``page_size`` items from the top of the ranking until
        it ends (the last page is the first shorter than ``page_size``; an empty store yields nothing).
        ``allowed`` is resolved once, so a predicate runs over the metadata once, not per page."""
        if int(page_size) < 1:
            raise ValueError("page_size must be >= 1")
        if self.index is None or self.index.ntotal == 0:
            return
        own = allowed is not None and not hasattr(allowed, "close")  # (a caller's selector stays the caller's)
        sel = self.index.selector(self._allowed_rows(allowed)) if own else allowed
        try:
            after = None
            while True:
                page = self.search_page(query_embedding, page_size, after=after, allowed=sel)
                if page:
                    yield page
                if len(page) < int(page_size):
                    return
                after = page[-1]
        finally:
            if own:
                sel.close()

    def _group_keys(self, group_by, n: int):
        """``(groups, values, own)`` of a ``group_by``: the index's group keys object, the value each
        non-negative key stands for (``None``: the key itself), and whether the caller closes the object (a cached one stays)."""
        if isinstance(group_by, str):
            hit = self._group_cache.get(group_by)
            if hit is not None and hit[0] is self.index and hit[1] == n:
                return hit[2], hit[3], False
            raw = [m.get(group_by) if isinstance(m, dict) else None for m in self.metadata[:n]]
        elif callable(group_by):
            raw = [group_by(m) for m in self.metadata[:n]]
        else:
            keys = np.asarray(group_by)
            if keys.ndim != 1 or keys.shape[0] != n or keys.dtype.kind not in "iu":
                raise ValueError(f"group_by must be a field name, a callable or {n} ints (one per item)")
            return self.index.group_keys(keys.astype(np.int64)), None, True
        codes: Dict[Any, int] = {}
        values: List[Any] = []
        keys = np.empty((n,), dtype=np.int64)
        for i, value in enumerate(raw):
            if value is None:
                keys[i] = -1
                continue
            code = codes.get(value)
            if code is None:
                code = codes[value] = len(values)
                values.append(value)
            keys[i] = code
        groups = self.index.group_keys(keys)
        if isinstance(group_by, str):
            self._drop_group_cache()  # (one field at a time: a page groups by one key)
            self._group_cache[group_by] = (self.index, n, groups, values)
            return groups, values, False
        return groups, values, True

    def _drop_group_cache(self) -> None:
        cache, self._group_cache = self._group_cache, {}
        for _, _, groups, _ in cache.values():
            groups.close()

    def search_range(self, query_embedding: List[float], radius: float, allowed=None,
                     max_results: Optional[int] = None) -> List[Dict]:
        """Every item within a score radius, best first (an addition at the boundary; faiss's
        ``IndexFlat.range_search``): the items whose ``distance`` -- the value :meth:`search` reports
        -- is above ``radius`` (inner product / cosine) or below it (L2), exactly, however many there
        are.  It replaces the reference's cut of a guessed top-``candidate_k`` at its score floors
        (core/searcher.py:771-843): one call per floor, no ``candidate_k`` to guess.  The guards,
        the normalisation and the result dicts are :meth:`search`'s; ``allowed`` as there;
        ``max_results`` keeps the best ``max_results`` of them.  HNSW stores and multi-GPU stores answer
        through the exact flat path, as filtered calls do."""
        if self.index is None or self.index.ntotal == 0:
            return []
        if len(query_embedding) != self.dimension:
            raise ValueError(f"向量维度不匹配: {len(query_embedding)} != {self.dimension}")
        if max_results is not None and int(max_results) <= 0:
            return []
        sel = None if allowed is None else self._allowed_rows(allowed)
        lims, distances, indices = self.index.range_search(self._normalize_query(query_embedding), float(radius),
                                                           sel=sel)
        n = int(lims[1]) if max_results is None else min(int(lims[1]), int(max_results))
        return [{"metadata": self.metadata[index], "distance": float(distance)}
                for distance, index in zip(distances[:n].tolist(), indices[:n].tolist())]

    def count_matches(self, query_embedding: List[float], threshold: float, allowed=None) -> int:
        """How many items :meth:`search_range` would return for ``radius = threshold`` -- "about 1,240
        photos" -- without producing one of them (an addition at the boundary; Elasticsearch's count API,
        Qdrant ``count``).  The reference derives such figures from its over-fetched ``candidate_k`` rows
        (core/searcher.py:627-770); this count is exact over every item.  The guards, the normalisation and
        ``allowed`` are :meth:`search_range`'s."""
        if self.index is None or self.index.ntotal == 0:
            return 0
        if len(query_embedding) != self.dimension:
            raise ValueError(f"向量维度不匹配: {len(query_embedding)} != {self.dimension}")
        sel = None if allowed is None else self._allowed_rows(allowed)
        totals, _ = self.index.range_count(self._normalize_query(query_embedding), float(threshold), sel=sel)
        return int(totals[0])

    def facet_counts(self, query_embedding: List[float], threshold: float, group_by, allowed=None) -> Dict[str, Any]:
        """How the items :meth:`search_range` would return for ``radius = threshold`` split over a key --
        "2019 (12) · 2020 (40) · 2021 (7)" -- exactly, without producing one of them (an addition at the
        boundary; Elasticsearch ``terms`` aggregations, Qdrant's facet API, Typesense / Meilisearch
        ``facet_by``): ``{"total": n, "counts": {value: n, ...}, "ungrouped": n}``.  ``counts`` holds only
        the values with ``n > 0``, in ascending key order (a field's or a callable's values are keyed in
        order of first appearance, integer keys by themselves); ``ungrouped`` counts the matching items
        without the field.  ``group_by`` and its cache are :meth:`search_grouped`'s; ``threshold``,
        ``allowed``, the guards and the normalisation are :meth:`search_range`'s."""
        if self.index is None or self.index.ntotal == 0:
            return {"total": 0, "counts": {}, "ungrouped": 0}
        if len(query_embedding) != self.dimension:
            raise ValueError(f"向量维度不匹配: {len(query_embedding)} != {self.dimension}")
        n = int(self.index.ntotal)
        groups, values, own = self._group_keys(group_by, n)
        try:
            sel = None if allowed is None else self._allowed_rows(allowed)
            totals, counts = self.index.range_count(self._normalize_query(query_embedding), float(threshold),
                                                    groups=groups, sel=sel)
        finally:
            if own:
                groups.close()
        if values is None:  # integer keys: the columns are the distinct non-negative ones, ascending
            given = np.asarray(group_by)
            cols = np.unique(given[given >= 0]).tolist()
        else:
            cols = values
        row = counts[0]
        return {"total": int(totals[0]), "counts": {cols[g]: int(row[g]) for g in range(len(cols)) if row[g] > 0},
                "ungrouped": int(row[len(cols)])}

    def similar_to(self, query_embedding: List[float], threshold: float, allowed=None, negate: bool = False):
        """The items :meth:`search_range` would return for ``radius = threshold`` as a selector, built on
        the device without producing one of them (an addition at the boundary): pass it as ``allowed=`` to
        any method -- "beach, not people" is
        ``store.search(q_beach, 20, allowed=store.similar_to(q_people, 0.25, negate=True))``.
        ``negate`` selects the items that do *not* match instead.  ``allowed`` restricts the items on both
        sides: the result is always a subset of it.  The guards, the normalisation and the threshold
        convention are :meth:`search_range`'s / :meth:`count_matches`': cosine / inner product above the
        threshold, L2 below it, strictly.  An empty store raises ``RuntimeError`` (there is nothing to
        select from).  Selectors combine with ``&``, ``|``, ``-`` and ``~`` on a one-GPU store."""
        if self.index is None or self.index.ntotal == 0:
            raise RuntimeError("the store holds no items to select from")
        if len(query_embedding) != self.dimension:
            raise ValueError(f"向量维度不匹配: {len(query_embedding)} != {self.dimension}")
        sel = None if allowed is None else self._allowed_rows(allowed)
        return self.index.selector_from_range(self._normalize_query(query_embedding), float(threshold), mode="any",
                                              negate=bool(negate), sel=sel)

    def similar_to_items(self, photo_paths, threshold: float, allowed=None, negate: bool = False, mode: str = "any"):
        """:meth:`similar_to` with photos the store holds as the queries, their stored rows gathered on the
        device: the items within ``threshold`` of at least one of ``photo_paths`` (``mode="all"``: of every
        one).  A photo matches itself like any other item, so "drop everything near these rejected shots"
        (``negate=True``) drops the shots too.  A path the store does not hold raises ``ValueError``."""
        if self.index is None or self.index.ntotal == 0:
            raise RuntimeError("the store holds no items to select from")
        ids = []
        for path in ([photo_paths] if isinstance(photo_paths, str) else list(photo_paths)):
            index = self._path_to_index.get(path)
            if index is None or index >= self.index.ntotal:
                raise ValueError(f"未找到图片: {path}")
            ids.append(index)
        sel = None if allowed is None else self._allowed_rows(allowed)
        return self.index.selector_from_range_rows(np.asarray(ids, dtype=np.int64), float(threshold), mode=mode,
                                                   negate=bool(negate), sel=sel)

    def search_similar(self, photo_path: str, top_k: int, allowed=None) -> List[Dict]:
        """The ``top_k`` items most similar to a photo the store holds, the photo itself left out (an
        addition at the boundary): :meth:`search`'s result dicts for the stored row of ``photo_path``
        as the query.  It replaces the reference's ``Searcher.search_by_image_path``
        (core/searcher.py:1751-1814: the row reconstructed to a Python list, ``max(k + 1, 5 k)``
        results fetched and the photo's own path filtered out afterwards) with one call in which the
        query never leaves the device and the photo is removed by its id -- exact under ties: a copy
        of the photo with a lower id stays and comes first.  ``top_k`` is clamped to ``ntotal - 1``;
        an empty store returns ``[]``; a path the store does not hold raises ``ValueError``;
        ``allowed`` as in :meth:`search`.  HNSW stores answer through the exact flat path, as filtered
        calls do.  One difference from the reference's route: the stored row is the query as it is
        and is not normalised a second time (the reference sends it through ``search``, which
        divides the already normalised row by its norm again)."""
        if self.index is None or self.index.ntotal == 0:
            return []
        index = self._path_to_index.get(photo_path)
        if index is None or index >= self.index.ntotal:
            raise ValueError(f"未找到图片: {photo_path}")
        k = min(int(top_k), int(self.index.ntotal) - 1)
        if k <= 0:
            return []
        sel = None if allowed is None else self._allowed_rows(allowed)
        distances, indices = self.index.search_rows(np.asarray([index], dtype=np.int64), k, sel=sel, drop_self=True)
        return [{"metadata": self.metadata[i], "distance": float(distance)}
                for distance, i in zip(distances[0].tolist(), indices[0].tolist()) if i != -1]

    def _allowed_mask(self, allowed) -> np.ndarray:
        """``allowed`` (a boolean mask, item ids or a predicate over the metadata) as a boolean mask."""
        n = int(self.index.ntotal)
        rows = self._allowed_rows(allowed)
        if hasattr(rows, "to_mask"):  # a selector (similar_to): its rows, none behind them
            got = np.asarray(rows.to_mask(), dtype=bool)[:n]
            return np.concatenate([got, np.zeros((n - got.shape[0],), dtype=bool)])
        return np.unpackbits(pack_allowed(n, rows), bitorder="little")[:n].astype(bool)

    def duplicate_pairs(self, threshold: float, allowed=None, max_pairs: Optional[int] = None):
        """Every pair of items closer than ``threshold`` -- ``distance`` above it (cosine) or below it
        (L2), the value :meth:`search` reports -- as arrays ``(i, j, distance)`` with ``i < j``, each
        pair once, ordered by ``i`` and best first within it.  One self-join on the device
        (``range_search_rows(..., self_mode="above")``): no row crosses the host, no pair comes twice.
        ``allowed`` (a boolean mask, item ids or a predicate over the metadata) restricts both sides
        of a pair; ``max_pairs`` bounds the answer (beyond it the call raises, naming the count)."""
        empty = (np.empty((0,), dtype=np.int64), np.empty((0,), dtype=np.int64), np.empty((0,), dtype=np.float32))
        if self.index is None or self.index.ntotal == 0:
            return empty
        ids = mask = None
        if allowed is not None:
            mask = self._allowed_mask(allowed)
            ids = np.flatnonzero(mask).astype(np.int64)
            if ids.shape[0] < 2:
                return empty
        lims, distances, indices = self.index.range_search_rows(float(threshold), ids=ids, sel=mask, self_mode="above",
                                                                max_total=max_pairs)
        first = np.arange(int(self.index.ntotal), dtype=np.int64) if ids is None else ids
        return np.repeat(first, np.diff(lims)), indices, distances

    def find_duplicates(self, threshold: float, allowed=None) -> List[List[int]]:
        """Groups of near-duplicate items: the connected components of :meth:`duplicate_pairs` (a chain
        a-b, b-c is one group even when a and c are further apart than ``threshold``) as lists of
        item ids, each ascending, ordered by their first id; items without a duplicate are left out.
        The union-find runs on the host over the pair list."""
        first, second, _ = self.duplicate_pairs(threshold, allowed=allowed)
        parent: Dict[int, int] = {}

        def find(x: int) -> int:
            root = x
            while parent.setdefault(root, root) != root:
                root = parent[root]
            while parent[x] != root:  # path compression
                parent[x], x = root, parent[x]
            return root

        for a, b in zip(first.tolist(), second.tolist()):
            ra, rb = find(a), find(b)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)  # (the root is the group's smallest id)
        groups: Dict[int, List[int]] = {}
        for x in sorted(parent):
            groups.setdefault(find(x), []).append(x)
        return [groups[root] for root in sorted(groups)]

    def duplicate_labels(self, threshold: float, allowed=None) -> np.ndarray:
        """One label per item for :meth:`find_duplicates`' grouping (an addition at the boundary; DBSCAN
        with ``min_samples = 1``, single linkage cut at ``threshold``): int64 of length ``ntotal``, an
        item's label the smallest id of its group -- its own id when it has no duplicate -- and ``-1`` for
        an item ``allowed`` leaves out.  The groups form on the device (``index.range_components``): no
        pair list is made, so a burst of a thousand copies costs a thousand labels, not half a million
        pairs.  Without ``allowed`` the labels are valid ``group_by`` keys for :meth:`search_grouped`
        ("one result per burst") and :meth:`facet_counts` ("matches per burst")."""
        if self.index is None or self.index.ntotal == 0:
            return np.empty((0,), dtype=np.int64)
        sel = None if allowed is None else self._allowed_mask(allowed)
        labels, _, _ = self.index.range_components(float(threshold), sel=sel)
        return labels

    def duplicate_groups(self, threshold: float, allowed=None, min_size: int = 2) -> List[List[int]]:
        """:meth:`find_duplicates` without the pair list: the same groups in the same format -- lists of
        item ids, each ascending, ordered by their first id -- built from :meth:`duplicate_labels`; groups
        of fewer than ``min_size`` items are left out (``1`` keeps the items without a duplicate)."""
        labels = self.duplicate_labels(threshold, allowed=allowed)
        order = np.argsort(labels, kind="stable")  # by label, ascending ids within one
        order = order[labels[order] >= 0]
        if order.shape[0] == 0:
            return []
        starts = np.flatnonzero(np.diff(labels[order], prepend=-1))
        return [g.tolist() for g in np.split(order, starts[1:]) if g.shape[0] >= int(min_size)]

    @staticmethod
    def _density_args(threshold, min_samples=1):
        """``threshold`` as one non-NaN float, ``min_samples`` as an integer >= 1 (``ValueError`` otherwise),
        checked before the index is touched."""
        t = np.asarray(threshold, dtype=np.float64)
        if t.ndim != 0:
            raise ValueError(f"threshold must be one scalar, got shape {t.shape}")
        if np.isnan(t):
            raise ValueError("threshold must not be NaN")
        if isinstance(min_samples, (bool, np.bool_)) or not isinstance(min_samples, (int, np.integer)) \
                or int(min_samples) < 1:
            raise ValueError(f"min_samples must be an integer >= 1, got {min_samples!r}")
        return float(t), int(min_samples)

    def neighbor_counts(self, threshold: float, allowed=None) -> np.ndarray:
        """How many other items lie within ``threshold`` of each item (an addition at the boundary): int64 of
        length ``ntotal``, ``-1`` for an item ``allowed`` leaves out; ``allowed`` restricts both ends, as in
        :meth:`duplicate_pairs`, whose pairs these counts are the bincount of.  Counted on the device
        (``index.range_degrees``): no pair list is made."""
        t, _ = self._density_args(threshold)
        if self.index is None or self.index.ntotal == 0:
            return np.empty((0,), dtype=np.int64)
        sel = None if allowed is None else self._allowed_mask(allowed)
        return self.index.range_degrees(t, sel=sel)[0]

    def _density(self, threshold, min_samples, allowed):
        t, ms = self._density_args(threshold, min_samples)
        if self.index is None or self.index.ntotal == 0:
            return np.empty((0,), dtype=np.int64), np.empty((0,), dtype=np.uint8), np.empty((0,), dtype=np.int64)
        sel = None if allowed is None else self._allowed_mask(allowed)
        labels, kinds, degrees, _ = self.index.range_dbscan(t, ms, sel=sel)
        return labels, kinds, degrees

    def density_labels(self, threshold: float, min_samples: int = 3, allowed=None):
        """DBSCAN over the items (an addition at the boundary; ``sklearn.cluster.DBSCAN``'s core points, run on
        the device by ``index.range_dbscan``): an item with at least ``min_samples`` items within
        ``threshold``, itself included, is *core*; clusters are the connected groups of core items; an item
        that is not core but has a core item within ``threshold`` is a *border* item of the cluster of its
        closest core item (ties to the lower id) and bridges nothing; the rest is *noise*.  Returns
        ``(labels, kinds)``: ``labels`` int64, a cluster's label the smallest id of its core items, ``-1`` for
        noise and for items ``allowed`` leaves out; ``kinds`` uint8, ``0`` left out, ``1`` noise, ``2``
        border, ``3`` core.  Unlike :meth:`duplicate_labels` a stray in-between frame does not fuse two
        events.  The labels are valid ``group_by`` keys for :meth:`search_grouped` and
        :meth:`facet_counts`, noise ungrouped."""
        labels, kinds, _ = self._density(threshold, min_samples, allowed)
        return labels, kinds

    def density_clusters(self, threshold: float, min_samples: int = 3, allowed=None) -> List[Dict]:
        """:meth:`density_labels` as one dict per cluster, ordered by label: ``{"label": the smallest core id,
        "items": [the cluster's ids, ascending], "core": [those of them that are core], "cover": id,
        "size": n}``; ``cover`` is the core item with the most items within ``threshold`` (ties: the lower
        id).  Noise is left out."""
        labels, kinds, degrees = self._density(threshold, min_samples, allowed)
        order = np.argsort(labels, kind="stable")  # by label, ascending ids within one
        order = order[labels[order] >= 0]
        if order.shape[0] == 0:
            return []
        starts = np.flatnonzero(np.diff(labels[order], prepend=-1))
        out = []
        for g in np.split(order, starts[1:]):
            core = g[kinds[g] == 3]
            cover = int(core[np.argmax(degrees[core])])  # (argmax takes the first of equals: the lower id)
            out.append({"label": int(labels[g[0]]), "items": g.tolist(), "core": core.tolist(), "cover": cover,
                        "size": int(g.shape[0])})
        return out

    def cluster_items(self, n_clusters: int, allowed=None, niter: int = 20, seed: int = 1234) -> List[Dict]:
        """The items sorted into ``n_clusters`` visual groups, one cover photo each (an addition at the
        boundary; faiss's ``Kmeans`` over the rows the index holds): exact k-means on the device
        (``index.kmeans``) under L2 assignment -- unit-norm cosine rows cluster properly under it --
        from ``n_clusters`` items drawn with ``np.random.default_rng(seed)``.  Returns one dict per
        non-empty cluster, ``{"items": [item ids, ascending], "representative": id, "size": n}``,
        largest first (ties: the lower cluster id); ``representative`` is the item closest to its
        cluster's centroid (ties: the lower id).  ``allowed`` (a boolean mask, item ids or a predicate
        over the metadata) restricts the items; fewer allowed items than ``n_clusters`` clamp the
        cluster count; an empty store, or nothing allowed, gives ``[]``.  The result is reproducible
        to the bit."""
        if self.index is None or self.index.ntotal == 0:
            return []
        if int(n_clusters) < 1:
            raise ValueError("n_clusters must be >= 1")
        if allowed is None:
            mask = None
            members = np.arange(int(self.index.ntotal), dtype=np.int64)
        else:
            mask = self._allowed_mask(allowed)
            members = np.flatnonzero(mask).astype(np.int64)
        if members.shape[0] == 0:
            return []
        k = min(int(n_clusters), int(members.shape[0]))
        res = self.index.kmeans(k, niter=int(niter), seed=seed, sel=mask, metric="l2")
        labels = np.asarray(res.labels)
        dist = np.asarray(res.distances)
        clusters = []
        for c in range(k):
            pos = np.flatnonzero(labels == c)
            if pos.shape[0] == 0:
                continue
            best = pos[np.argmin(dist[pos])]  # (argmin: the first of equal distances, the lower id)
            clusters.append((-int(pos.shape[0]), c, {"items": members[pos].tolist(),
                                                     "representative": int(members[best]),
                                                     "size": int(pos.shape[0])}))
        clusters.sort(key=lambda t: (t[0], t[1]))
        return [t[2] for t in clusters]

    def _allowed_rows(self, allowed):
        """A predicate over the metadata as a boolean mask over the items; selectors, masks and ids pass."""
        if callable(allowed):
            n = int(self.index.ntotal)
            return np.fromiter((bool(allowed(m)) for m in self.metadata[:n]), dtype=bool, count=n)
        return allowed

    def selector(self, allowed):
        """A reusable selector for :meth:`search`'s ``allowed`` (the searcher's relaxation rounds repeat
        one filter): a boolean mask, item ids, or a predicate applied to each ``self.metadata[i]``.
        It covers the items present now and is stale after :meth:`clear` or a removal."""
        if self.index is None:
            raise RuntimeError("the store has no index yet")
        return self.index.selector(self._allowed_rows(allowed))

    def get_embedding_by_photo_path(self, photo_path: str) -> Optional[List[float]]:
        index = self._path_to_index.get(photo_path)
        if index is None:
            return None
        if index < len(self.metadata) and self.index is not None and index < self.index.ntotal:
            cached = self._embeddings.get(index)
            if cached is None:
                vector = self.index.reconstruct(index)
                cached = vector.astype("float32").tolist()
                self._embeddings[index] = cached
            if cached is not None:
                return list(cached)
        return None

    def has_photo_path(self, photo_path: str) -> bool:
        return photo_path in self._path_to_index

    def save(self) -> None:
        """索引持久化 (utils/vector_store.py:217-237)."""
        if self.index is None:
            raise ValueError("索引未初始化")

        index_dir = os.path.dirname(self.index_path)
        metadata_dir = os.path.dirname(self.metadata_path)
        if index_dir:
            os.makedirs(index_dir, exist_ok=True)
        if metadata_dir:
            os.makedirs(metadata_dir, exist_ok=True)

        # The reference rewrites the whole index per indexer batch (utils/vector_store.py:234,
        # core/indexer.py:945): O(N) per save.  Rows never change once added, so when the file on
        # disk is the one this store last wrote or loaded, only the new rows and the header are
        # written -- the bytes are identical to a full rewrite.  Payload bytes stream HBM -> file.
        n, d, mt = int(self.index.ntotal), int(self.index.d), int(self.index.metric_type)
        old = self._appendable_rows(d, mt)
        if self.index_type == "hnsw" or self._file_hnsw:
            # an IHNf file the reference's faiss can load (rollback), at every size; a graph loaded
            # from file is kept (rows added since are inserted into it), with efSearch as configured
            # (the reference sets hnsw.efSearch after every load of an HNSW configuration,
            # utils/vector_store.py:135, and faiss writes it back; a flat configuration keeps the
            # file's)
            ef = self.hnsw_ef_search if self.index_type == "hnsw" else None
            if self._graph_covers(n):
                graph = dict(self._graph_arrays)
                if ef is not None:
                    graph["efSearch"] = ef
            else:
                graph = self._build_graph(n)
            faiss_format.write_hnsw(self.index_path, graph, d, n, mt, lambda path, off: self.index.write_rows(path, off, 0, n))
            self._graph_arrays = graph
            self._persisted = None
            self._write_index_meta()
            with open(self.metadata_path, "w", encoding="utf-8") as file:
                json.dump(self.metadata, file, ensure_ascii=False, indent=2)
            return
        if old is not None and old <= n:
            faiss_format.append_flat_rows(self.index_path, d, old, n, mt,
                                          lambda path, off: self.index.write_rows(path, off, old, n - old))
        else:
            faiss_format.write_flat_rows(self.index_path, d, n, mt,
                                         lambda path, off: self.index.write_rows(path, off, 0, n))
        self._persisted = self._file_state(n, d, mt)
        self._write_index_meta()
        with open(self.metadata_path, "w", encoding="utf-8") as file:
            json.dump(self.metadata, file, ensure_ascii=False, indent=2)

    def load(self) -> bool:
        """加载索引与元数据 (utils/vector_store.py:239-260)."""
        if not os.path.exists(self.index_path) or not os.path.exists(self.metadata_path):
            return False

        loaded = faiss_format.read_index(self.index_path)
        index = self._create_index_with_metric(loaded.d, loaded.metric_type)
        if loaded.ntotal:  # payload streamed file -> pinned chunks -> HBM (no host copy of the matrix)
            index.add_from_file(self.index_path, loaded.payload_offset, loaded.ntotal)
        self._drop_graph()
        self._drop_group_cache()
        self.index = index
        self._persisted = (self._file_state(loaded.ntotal, loaded.d, loaded.metric_type)
                           if loaded.kind == "flat" else None)
        payload = self._load_index_meta()
        self._validate_loaded_index(payload, loaded)
        # a flat configuration keeps an HNSW file's graph: save() writes it back (extended by the
        # rows added since), as the reference's IndexHNSWFlat would be
        self._file_hnsw = loaded.kind == "hnsw" and self.index_type == "flat"
        if loaded.kind == "hnsw" and (self._file_hnsw or _hnsw_graph_search()):
            self._graph_arrays = faiss_format.read_hnsw_graph(self.index_path)

        with open(self.metadata_path, "r", encoding="utf-8") as file:
            self.metadata = json.load(file)
        if self.index.ntotal != len(self.metadata):
            raise ValueError("索引与元数据数量不一致，请重新构建索引")
        self.dimension = self.index.d
        self._embeddings = {}
        self._rebuild_path_index()
        return True

    def _create_index_with_metric(self, dimension: int, metric_type: int):
        metric = "cosine" if metric_type == METRIC_INNER_PRODUCT else "l2"
        return _index_factory(int(dimension), metric)

    def get_total_items(self) -> int:
        """获取当前向量数量."""
        if self.index is None:
            return 0
        return int(self.index.ntotal)

    def clear(self) -> None:
        """清空索引与元数据."""
        self._drop_graph()
        self._drop_group_cache()
        self._file_hnsw = False
        self.index = self._create_index(self.dimension) if self.dimension else None
        self.metadata = []
        self._embeddings = {}
        self._path_to_index = {}
        self._persisted = None

    # ------------------------------------------------------------------ HNSW graph search
    def _graph_covers(self, n: int) -> bool:
        g = self._graph_arrays
        return g is not None and int(np.asarray(g["levels"]).shape[0]) == n

    def _drop_graph(self) -> None:
        self._drop_graph_search()
        self._graph_arrays = None

    def _search_rows(self, q: np.ndarray, k: int) -> Tuple[np.ndarray, np.ndarray]:
        """``index.search``, or with ``VECTOR_HNSW_SEARCH=graph`` on an HNSW store, faiss's HNSW
        search on the GPU over the graph of the loaded file or the graph ``save()`` writes
        (:meth:`_build_graph`).  The graph is rebuilt only once the store has grown by
        ``_GRAPH_REBUILD_GROWTH`` since it was built; rows added behind it meanwhile are searched
        exactly (a flat index of those rows) and merged with the graph's results, so alternating
        ``add_item`` / ``search`` does not pay a whole-graph build per search.  Stores above
        ``VECTOR_HNSW_GRAPH_MAX_ROWS`` (their graph is still saved: :meth:`save`), beams wider than
        the GPU search takes (max(efSearch, k) > 2048) and multi-GPU indexes search exactly."""
        n = int(self.index.ntotal)
        if (self.index_type != "hnsw" or not _hnsw_graph_search() or not isinstance(self.index, FlatIndex)
                or max(k, self.hnsw_ef_search) > _HNSW_EF_MAX or n > _hnsw_graph_max_rows()):
            return self.index.search(q, k)
        if self._hnsw is not None and self._hnsw.index is not self.index:
            self._drop_graph_search()
        covered = self._hnsw.ntotal if self._hnsw is not None else 0
        if self._hnsw is None or n > covered * _GRAPH_REBUILD_GROWTH:
            self._drop_graph_search()
            g = self._graph_arrays
            if g is None or not 0 < int(np.asarray(g["levels"]).shape[0]) <= n or \
                    n > int(np.asarray(g["levels"]).shape[0]) * _GRAPH_REBUILD_GROWTH:
                self._graph_arrays = self._build_graph(n)
            self._hnsw = HNSWGraph(self.index, self._graph_arrays, self.hnsw_ef_search)
            covered = self._hnsw.ntotal
        D, I = self._hnsw.search(q, k, self.hnsw_ef_search)
        if covered == n:
            return D, I
        # rows [covered, n): exact search over a flat index of just those rows, then a merge
        tail = self._graph_tail
        if tail is None:
            tail = self._graph_tail = self._create_index(self.dimension)
        have = covered + int(tail.ntotal)
        if have < n:
            tail.add(np.ascontiguousarray(self.index.reconstruct_n(have, n - have)))
        Dt, It = tail.search(q, min(k, n - covered))
        It = np.where(It >= 0, It + covered, -1)
        return _merge_topk(D, I, Dt, It, k, int(self.index.metric_type) == METRIC_INNER_PRODUCT)

    def _drop_graph_search(self) -> None:
        """Release the GPU graph and the exactly-searched tail behind it (the arrays stay)."""
        if self._hnsw is not None:
            self._hnsw.close()
        self._hnsw = None
        if self._graph_tail is not None:
            self._graph_tail.close()
        self._graph_tail = None

    def _build_graph(self, n: int) -> Dict[str, Any]:
        """The faiss-layout HNSW graph over the n stored rows.  A graph already covering the first
        m < n rows (the one last saved or loaded, a faiss-built file's included) is extended by
        inserting rows [m, n) the way faiss's ``IndexHNSWFlat.add`` does, batched
        (:func:`hnsw.insert_rows`: an efConstruction beam over the existing graph + the batch's
        exact candidates, the selection heuristic, reverse links); otherwise the first
        ``VECTOR_HNSW_GRAPH_MAX_ROWS`` rows are built at once from exact candidates
        (:meth:`_build_graph_exact`) and the rest inserted.  Cost per save: the new rows only."""
        g = self._graph_arrays
        make = lambda: self._create_index(self.dimension)  # noqa: E731
        if g is not None and 0 < int(np.asarray(g["levels"]).shape[0]) < n:
            # (a flat configuration over an HNSW file inserts with the file's efConstruction, as the
            # reference's loaded IndexHNSWFlat would)
            efc = int(g["efConstruction"]) if self._file_hnsw else int(self.hnsw_ef_construction)
            return hnsw_mod.insert_rows(self.index, g, int(np.asarray(g["levels"]).shape[0]), n, efc, make)
        n0 = min(n, max(1, _hnsw_graph_max_rows()))
        g = self._build_graph_exact(n0)
        if n0 < n:
            g = hnsw_mod.insert_rows(self.index, g, n0, n, int(self.hnsw_ef_construction), make)
        return g

    def _build_graph_exact(self, n: int) -> Dict[str, Any]:
        """A faiss-layout HNSW graph over the first n stored rows built at once: node levels drawn
        as faiss's ``HNSW::random_level`` does (``set_default_probas(M, 1/ln M)``; numpy's
        generator, seed 12345, not faiss's: :func:`hnsw.draw_levels`); on every level each node's
        candidates are its exact max(efConstruction, width) nearest nodes of that level (the flat
        search, ties -> lower id) and its neighbours (2M on level 0, M above) are chosen from them
        by faiss's heuristic, reverse links included (:func:`hnsw.select_level`, on the GPU); the
        entry point is the first node of the top level (oracle/hnsw_oracle.py ``heuristic_graph``
        restates it)."""
        M = self.hnsw_m
        probas, cum = faiss_format.hnsw_default_probas(M)
        lev = hnsw_mod.draw_levels(n, probas)
        levels = (lev + 1).astype(np.int32)
        offsets = np.zeros(n + 1, dtype=np.uint64)
        offsets[1:] = np.cumsum(cum[levels].astype(np.uint64))
        nb = np.full(int(offsets[-1]), -1, dtype=np.int32)
        top = int(lev.max()) if n else -1
        for level in range(top + 1):
            members = np.nonzero(lev >= level)[0]
            width = int(cum[level + 1] - cum[level])
            C = min(max(int(self.hnsw_ef_construction), width), hnsw_mod.HP_C_MAX)
            cand = self._knn_graph(C, None if level == 0 and n == int(self.index.ntotal) else members)
            sel = hnsw_mod.select_level(self.index, members, cand, width)
            base = offsets[members].astype(np.int64) + int(cum[level])
            for j in range(members.shape[0]):
                row = sel[j][sel[j] >= 0]
                nb[base[j]:base[j] + len(row)] = row
        return {"assign_probas": probas, "cum_nneighbor_per_level": cum, "levels": levels, "offsets": offsets,
                "neighbors": nb, "entry_point": int(np.nonzero(lev == top)[0][0]) if n else -1, "max_level": top,
                "efConstruction": int(self.hnsw_ef_construction), "efSearch": int(self.hnsw_ef_search),
                "upper_beam": 1}

    def _knn_graph(self, width: int, members: Optional[np.ndarray] = None) -> np.ndarray:
        """Exact top-``width`` neighbours (itself excluded, -1 padded) of every stored row, or of
        every row of ``members`` among ``members`` only (global ids; a temporary index over their
        stored values), by the GPU flat search."""
        n = int(self.index.ntotal)
        index, ids = self.index, None
        if members is not None:
            ids = np.asarray(members, dtype=np.int64)
            index = self._create_index(self.dimension)
            for r0 in range(0, n, 65536):
                rows = self.index.reconstruct_n(r0, min(65536, n - r0))
                sel = ids[(ids >= r0) & (ids < r0 + rows.shape[0])] - r0
                if sel.size:
                    index.add(np.ascontiguousarray(rows[sel]))
        m = int(index.ntotal)
        out = np.full((m, width), -1, dtype=np.int32)
        kk = min(m, width + 1)
        try:
            for r0 in range(0, m, 4096):
                rows = index.reconstruct_n(r0, min(4096, m - r0))
                _, I = index.search(rows, kk)
                own = np.arange(r0, r0 + I.shape[0])[:, None]
                ok = (I >= 0) & (I != own)
                pos = np.cumsum(ok, axis=1) - 1  # order kept, itself dropped
                ok &= pos < width
                r, c = np.nonzero(ok)
                nbr = I[r, c] if ids is None else ids[I[r, c]]
                out[r0 + r, pos[r, c]] = nbr
        finally:
            if ids is not None and hasattr(index, "close"):
                index.close()
        return out

    # ------------------------------------------------------------------ persistence state
    def _file_state(self, rows: int, d: int, metric_type: int) -> Optional[Dict[str, Any]]:
        try:
            st = os.stat(self.index_path)
        except OSError:
            return None
        return {"path": os.path.abspath(self.index_path), "rows": int(rows), "d": int(d), "metric_type": int(metric_type),
                "stat": (st.st_dev, st.st_ino, st.st_size, st.st_mtime_ns)}

    def _appendable_rows(self, d: int, metric_type: int) -> Optional[int]:
        """Rows of the index file if it is still exactly what this store last wrote or loaded."""
        p = self._persisted
        if not p or p["path"] != os.path.abspath(self.index_path) or p["d"] != d or p["metric_type"] != metric_type:
            return None
        try:
            st = os.stat(self.index_path)
        except OSError:
            return None
        if (st.st_dev, st.st_ino, st.st_size, st.st_mtime_ns) != p["stat"]:
            return None
        if st.st_size != faiss_format.FLAT_HEADER_BYTES + p["rows"] * d * 4:
            return None
        return p["rows"]

    # ------------------------------------------------------------------ batched additions
    def add(self, embeddings: np.ndarray, metadatas: Sequence[Dict]) -> None:
        """Bulk ``add_item``: n x d rows + n metadata dicts in one device transfer."""
        rows = np.asarray(embeddings, dtype="float32")
        if rows.ndim != 2:
            raise ValueError("embeddings must be an (n, d) array")
        if len(metadatas) != rows.shape[0]:
            raise ValueError("metadatas must have one entry per row")
        if rows.shape[0] == 0:
            return
        if self.index is None:
            self.dimension = rows.shape[1]
            self.index = self._create_index(self.dimension)
        if rows.shape[1] != self.dimension:
            raise ValueError(f"向量维度不匹配: {rows.shape[1]} != {self.dimension}")
        self._drop_group_cache()
        self.index.add(self._normalize_rows(rows))
        base = len(self.metadata)
        self.metadata.extend(metadatas)
        for i, md in enumerate(metadatas):
            photo_path = md.get("photo_path") if isinstance(md, dict) else None
            if isinstance(photo_path, str) and photo_path:
                self._path_to_index[photo_path] = base + i

    # ------------------------------------------------------------------ removal
    def remove_ids(self, ids) -> int:
        """Remove items by id (an addition at the boundary; faiss's ``IndexFlat.remove_ids``): a boolean
        mask over the items or item ids.  The surviving items keep their order and take ids
        ``0..n-1`` in the index and in ``metadata`` alike, which is the shift the reference's
        id-indexed ``metadata`` list needs.  Returns the number removed.  An HNSW graph is dropped,
        not edited (the next save or graph search builds one over the survivors, as a fresh store
        would), and the next :meth:`save` rewrites the whole index file: a shrink in place could not
        keep the header-last guarantee of the append path."""
        if self.index is None:
            return 0
        n = int(self.index.ntotal)
        remove = np.unpackbits(pack_allowed(n, ids), bitorder="little")[:n].astype(bool)  # (validates ids / mask)
        if not remove.any():
            return 0
        self._drop_group_cache()
        removed = int(self.index.remove_ids(remove))
        new_id = np.cumsum(~remove) - 1  # surviving item i -> its new id
        self.metadata = [m for m, gone in zip(self.metadata, remove.tolist()) if not gone]
        self._embeddings = {int(new_id[i]): v for i, v in self._embeddings.items() if i < n and not remove[i]}
        self._rebuild_path_index()
        self._drop_graph()
        self._persisted = None
        return removed

    def remove_items(self, photo_paths) -> int:
        """Remove the items with these ``photo_path`` values (unknown paths are ignored); returns the
        number removed.  The indexer's prune of files that vanished from disk."""
        ids = sorted({self._path_to_index[p] for p in photo_paths if p in self._path_to_index})
        return self.remove_ids(np.asarray(ids, dtype=np.int64)) if ids else 0

    def update_item(self, embedding: List[float], metadata: Dict) -> None:
        """Replace the item with ``metadata["photo_path"]`` if the store holds one, then
        :meth:`add_item`: the new row goes to the end, as faiss's remove + add leaves it."""
        if embedding is None:
            raise ValueError("向量不能为空")
        if self.dimension is not None and len(embedding) != self.dimension:
            raise ValueError(f"向量维度不匹配: {len(embedding)} != {self.dimension}")
        photo_path = metadata.get("photo_path")
        if isinstance(photo_path, str) and photo_path in self._path_to_index:
            self.remove_items([photo_path])
        self.add_item(embedding, metadata)

    def search_batch(self, queries: np.ndarray, top_k: int) -> Tuple[np.ndarray, np.ndarray]:
        """Batched search in faiss layout: (D nq x k float32, I nq x k int64), rows normalised
        exactly like ``search``; k is clamped to ntotal as ``search`` does."""
        q = np.asarray(queries, dtype="float32")
        if q.ndim != 2:
            raise ValueError("queries must be an (nq, d) array")
        if self.index is None or self.index.ntotal == 0:
            return np.zeros((q.shape[0], 0), dtype=np.float32), np.zeros((q.shape[0], 0), dtype=np.int64)
        if q.shape[1] != self.dimension:
            raise ValueError(f"向量维度不匹配: {q.shape[1]} != {self.dimension}")
        k = min(top_k, self.index.ntotal)
        return self._search_rows(self._normalize_rows(q), k)

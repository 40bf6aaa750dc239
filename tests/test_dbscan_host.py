"""Density clusters without a GPU: the recipe on hand-made cases and against sklearn's DBSCAN, the wrappers'
argument checks, and ``VectorStore.neighbor_counts`` / ``density_labels`` / ``density_clusters`` over the
oracle index."""
import numpy as np
import pytest

from oracle import oracle as O
from oracle_components_index import components_reference
from oracle_dbscan_index import (BORDER, CORE, NOISE, NONE, dbscan_pairs, dbscan_reference, degrees_reference,
                                 oracle_dbscan_factory)
from oracle_diverse_index import burst_corpus
from photo_search_engine_amd import index as idxmod

N, D_ = 256, 72
COS = 0.95  # a chain's step: cos(theta); rows are near iff their angle is below arccos(0.9) = 1.42 theta
THETA = np.arccos(COS)
RADIUS = {"ip": 0.9, "l2": 0.2}  # (unit rows: squared L2 = 2 - 2 cos)


def _plane(angles, d=8, extra=0):
    """Unit rows at the given multiples of theta in the plane of the first two axes, then ``extra`` rows on axes
    of their own, far from everything."""
    x = np.zeros((len(angles) + extra, d), dtype=np.float32)
    for i, a in enumerate(angles):
        x[i, 0], x[i, 1] = np.cos(a * THETA), np.sin(a * THETA)
    for j in range(extra):
        x[len(angles) + j, 2 + j] = 1.0
    return x


# ---- the recipe --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_reference_chain(metric):
    x = _plane([0, 1, 2, 3, 4], extra=2)
    r = RADIUS[metric]
    deg, ne = degrees_reference(x, r, metric)
    assert deg.tolist() == [1, 2, 2, 2, 1, 0, 0] and ne == 4 and int(deg.sum()) == 2 * ne
    # min_samples = 3: the three inner rows are core, the ends are border rows of the one cluster
    labels, kinds, degrees, counts = dbscan_reference(x, r, metric, 3)
    assert labels.tolist() == [1, 1, 1, 1, 1, -1, -1]
    assert kinds.tolist() == [BORDER, CORE, CORE, CORE, BORDER, NOISE, NOISE]
    assert degrees.tolist() == deg.tolist()
    assert counts == {"clusters": 1, "core": 3, "border": 2, "noise": 2, "edges": 4}
    # min_samples = 4: nobody is core
    labels, kinds, _, counts = dbscan_reference(x, r, metric, 4)
    assert (labels == -1).all() and (kinds == NOISE).all()
    assert counts == {"clusters": 0, "core": 0, "border": 0, "noise": 7, "edges": 4}
    # min_samples = 1: the duplicate groups, every member core
    comp = components_reference(x, r, metric)[0]
    labels, kinds, _, counts = dbscan_reference(x, r, metric, 1)
    assert labels.tolist() == comp.tolist() == [0, 0, 0, 0, 0, 5, 6] and (kinds == CORE).all()
    assert counts["clusters"] == 3 and counts["core"] == 7
    # min_samples = 2: the groups of two or more, the singletons noise, no border row
    labels, kinds, _, counts = dbscan_reference(x, r, metric, 2)
    assert labels.tolist() == [0, 0, 0, 0, 0, -1, -1] and kinds.tolist() == [CORE] * 5 + [NOISE] * 2
    assert counts == {"clusters": 1, "core": 5, "border": 0, "noise": 2, "edges": 4}


@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("bridge,want", [(0.95, 0), (1.05, 5)])
def test_reference_non_core_bridge_does_not_join(metric, bridge, want):
    """Two dense groups, rows 0-3 and 5-8; row 4 is near one row of each (3 and 5) and nothing else.  As a core
    row it would fuse them (the duplicate groups do); as a border row it goes to the nearer of the two."""
    x = _plane([-0.9, -0.9, -0.9, 0, bridge, 2, 2.9, 2.9, 2.9])
    r = RADIUS[metric]
    assert components_reference(x, r, metric)[1] == 1  # (single linkage chains through the bridge)
    labels, kinds, degrees, counts = dbscan_reference(x, r, metric, 4)
    assert degrees.tolist() == [3, 3, 3, 4, 2, 4, 3, 3, 3]
    assert kinds.tolist() == [CORE] * 4 + [BORDER] + [CORE] * 4
    assert labels.tolist() == [0, 0, 0, 0, want, 5, 5, 5, 5]
    assert counts == {"clusters": 2, "core": 8, "border": 1, "noise": 0, "edges": 14}
    # at min_samples = 3 the bridge is core and the clusters are one
    labels, kinds, _, counts = dbscan_reference(x, r, metric, 3)
    assert (labels == 0).all() and (kinds == CORE).all() and counts["clusters"] == 1


@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("flip", [False, True])
def test_reference_exact_tie_goes_to_the_lower_core_id(metric, flip):
    """x = e0 between a = (c, s) and b = (c, -s): both scores are c (ip) or (1 - c)^2 + s^2 (l2) bit for bit.
    a and b are core through two copies each further out; x is a border row of both and takes the lower id."""
    c, s = np.float32(np.cos(THETA)), np.float32(np.sin(THETA))
    c2, s2 = np.float32(np.cos(1.9 * THETA)), np.float32(np.sin(1.9 * THETA))
    x = np.zeros((7, 8), dtype=np.float32)
    a, b = (4, 1) if flip else (1, 4)  # the group around +s sits at the lower or at the higher ids
    x[0, 0] = 1.0
    x[a, :2] = (c, s)
    x[a + 1, :2] = x[a + 2, :2] = (c2, s2)
    x[b, :2] = (c, -s)
    x[b + 1, :2] = x[b + 2, :2] = (c2, -s2)
    S = O.canon_scores(x[[a, b]], x[[0]], metric)
    assert np.float32(S[0, 0]) == np.float32(S[0, 1])
    labels, kinds, degrees, counts = dbscan_reference(x, RADIUS[metric], metric, 4)
    assert degrees.tolist() == [2, 3, 2, 2, 3, 2, 2]
    assert kinds.tolist() == [BORDER, CORE, BORDER, BORDER, CORE, BORDER, BORDER]
    assert labels.tolist() == [1, 1, 1, 1, 4, 4, 4]
    assert counts == {"clusters": 2, "core": 2, "border": 5, "noise": 0, "edges": 8}


def test_reference_non_member_core_neighbour():
    x = _plane([0, 1, 2, 3, 4], extra=2)
    mask = np.array([True, True, False, True, True, True, True])
    labels, kinds, degrees, counts = dbscan_reference(x, 0.9, "ip", 3, mask)
    # row 2 -- core when a member -- neither counts for rows 1 and 3 nor attaches them
    assert degrees.tolist() == [1, 1, -1, 1, 1, 0, 0]
    assert kinds.tolist() == [NOISE, NOISE, NONE, NOISE, NOISE, NOISE, NOISE]
    assert (labels == -1).all() and counts == {"clusters": 0, "core": 0, "border": 0, "noise": 6, "edges": 2}
    labels, kinds, _, counts = dbscan_reference(x, 0.9, "ip", 2, mask)
    assert labels.tolist() == [0, 0, -1, 3, 3, -1, -1] and counts["clusters"] == 2 and counts["border"] == 0
    # a mask shorter than the rows: the later rows are no members
    labels, kinds, degrees, counts = dbscan_reference(x, 0.9, "ip", 3, np.ones(4, dtype=bool))
    assert degrees.tolist() == [1, 2, 2, 1, -1, -1, -1] and kinds.tolist() == [BORDER, CORE, CORE, BORDER, 0, 0, 0]
    assert labels.tolist() == [1, 1, 1, 1, -1, -1, -1]
    # nothing allowed
    labels, kinds, degrees, counts = dbscan_reference(x, 0.9, "ip", 1, np.zeros(7, dtype=bool))
    assert (labels == -1).all() and (kinds == NONE).all() and (degrees == -1).all() and counts["edges"] == 0


# ---- sklearn -----------------------------------------------------------------------------------------------
# burst_corpus: burst b has 1 + (5 b) % 12 members base + 0.05 noise at d = 72, so two members of a burst meet at
# cos = 1 / (1 + 0.05^2) = 0.9975 on average.  Radius 0.9 makes every burst a clique (no border row can exist:
# the rows of a clique have one degree; bursts of one or two rows are noise from min_samples = 3); radius 0.9975
# cuts about half of a burst's pairs, so degrees differ within a burst: border rows at min_samples 3 and 6.
@pytest.mark.parametrize("min_samples", [2, 3, 6])
@pytest.mark.parametrize("radius", [0.9, 0.9975])
def test_reference_against_sklearn(radius, min_samples):
    cluster = pytest.importorskip("sklearn.cluster")
    x, _ = burst_corpus()
    xs = O.round_dtype(x, "bf16") if radius == 0.9 else np.array(x)
    n = xs.shape[0]
    pairs = dbscan_pairs(xs, radius, "ip")
    _, first, second, _ = pairs
    labels, kinds, degrees, counts = dbscan_reference(xs, radius, "ip", min_samples, pairs=pairs)
    assert counts["noise"] >= 1 and counts["clusters"] >= 5
    if radius != 0.9 and min_samples > 2:
        assert counts["border"] >= 1
    M = np.ones((n, n), dtype=np.float64)  # 0 where the pair passes, else 1: eps = 0.5 cannot round either way
    M[first, second] = M[second, first] = 0.0
    np.fill_diagonal(M, 0.0)
    sk = cluster.DBSCAN(eps=0.5, min_samples=min_samples, metric="precomputed").fit(M)
    core = np.flatnonzero(kinds == CORE)
    np.testing.assert_array_equal(np.sort(sk.core_sample_indices_), core)
    # the partition of the core rows
    ours = {}
    theirs = {}
    for i in core.tolist():
        ours.setdefault(int(labels[i]), []).append(i)
        theirs.setdefault(int(sk.labels_[i]), []).append(i)
    assert sorted(ours.values()) == sorted(theirs.values()) and -1 not in theirs
    np.testing.assert_array_equal(np.flatnonzero(sk.labels_ == -1), np.flatnonzero(kinds == NOISE))
    # a border row lands in a cluster that holds one of its core neighbours
    for i in np.flatnonzero(kinds == BORDER).tolist():
        near = np.flatnonzero(M[i] == 0.0)
        assert labels[i] in set(labels[near[kinds[near] == CORE]].tolist())
        assert sk.labels_[i] != -1


# ---- the wrappers ------------------------------------------------------------------------------------------
def test_wrappers_validate_before_any_library_call():
    ix = idxmod.FlatIndex.__new__(idxmod.FlatIndex)
    ix.d, ix._h, ix._L = 8, None, None
    mi = idxmod.MultiDeviceFlatIndex.__new__(idxmod.MultiDeviceFlatIndex)
    mi.d, mi._h, mi._L, mi._prune_copy = 8, None, None, None
    for obj in (ix, mi):
        with pytest.raises(ValueError):
            obj.range_degrees(np.nan)
        with pytest.raises(ValueError):
            obj.range_degrees([0.5, 0.6])  # one scalar radius
        with pytest.raises(ValueError):
            obj.range_dbscan(np.nan, 3)
        with pytest.raises(ValueError):
            obj.range_dbscan([0.5, 0.6], 3)
        for bad in (0, -1, 2.5, None, True):
            with pytest.raises(ValueError):
                obj.range_dbscan(0.5, bad)


# ---- the store ---------------------------------------------------------------------------------------------
def _store(tmp_path, monkeypatch, metric, fill=True):
    from photo_search_engine_amd import vector_store as vsmod
    monkeypatch.setattr(vsmod, "_index_factory", oracle_dbscan_factory)
    x, q = burst_corpus()
    meta = [{"photo_path": f"/p/{i}.jpg", "year": 2019 + i % 6} for i in range(N)]
    store = vsmod.VectorStore(dimension=D_, index_path=str(tmp_path / "idx"), metadata_path=str(tmp_path / "meta.json"),
                              metric=metric, index_type="flat")
    if fill:
        store.add(np.array(x), meta)
    return store, q


@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_store_density_methods(tmp_path, monkeypatch, metric):
    store, q = _store(tmp_path, monkeypatch, metric)
    threshold = 0.9975 if metric == "cosine" else 2 - 2 * 0.9975
    # the counts are the bincount of the pairs
    first, second, _ = store.duplicate_pairs(threshold)
    want = np.bincount(first, minlength=N) + np.bincount(second, minlength=N)
    counts = store.neighbor_counts(threshold)
    assert counts.dtype == np.int64 and counts.tolist() == want.tolist() and want.max() >= 5
    labels, kinds = store.density_labels(threshold, min_samples=3)
    assert labels.shape == kinds.shape == (N,) and labels.dtype == np.int64 and kinds.dtype == np.uint8
    assert ((kinds == CORE) == (counts + 1 >= 3)).all()
    assert (kinds == BORDER).any() and (kinds == NOISE).any() and ((labels == -1) == (kinds == NOISE)).all()
    clusters = store.density_clusters(threshold, min_samples=3)
    assert [c["label"] for c in clusters] == sorted(set(labels[labels >= 0].tolist())) and len(clusters) >= 5
    for c in clusters:
        assert c["items"] == np.flatnonzero(labels == c["label"]).tolist() and c["size"] == len(c["items"])
        assert c["core"] == [i for i in c["items"] if kinds[i] == CORE] and c["core"][0] == c["label"]
        top = max(counts[i] for i in c["core"])
        assert c["cover"] == min(i for i in c["core"] if counts[i] == top)
    # min_samples = 1: the duplicate groups
    labels1, kinds1 = store.density_labels(threshold, min_samples=1)
    assert labels1.tolist() == store.duplicate_labels(threshold).tolist() and (kinds1 == CORE).all()
    # allowed: a predicate restricts both ends of every pair
    pred = lambda m: m["year"] != 2020  # noqa: E731
    out = np.array([(2019 + i % 6) == 2020 for i in range(N)])
    first, second, _ = store.duplicate_pairs(threshold, allowed=pred)
    want = np.bincount(first, minlength=N) + np.bincount(second, minlength=N)
    want[out] = -1
    counts_f = store.neighbor_counts(threshold, allowed=pred)
    assert counts_f.tolist() == want.tolist() and counts_f.tolist() != counts.tolist()
    labels_f, kinds_f = store.density_labels(threshold, min_samples=3, allowed=pred)
    assert (kinds_f[out] == NONE).all() and (labels_f[out] == -1).all() and (kinds_f[~out] != NONE).all()
    assert ((kinds_f == CORE) == (counts_f + 1 >= 3)).all()
    for c in store.density_clusters(threshold, min_samples=3, allowed=pred):
        assert not out[c["items"]].any()
    # nothing is near anything: all noise, no cluster
    nothing = float("inf") if metric == "cosine" else float("-inf")
    assert store.density_clusters(nothing) == [] and (store.neighbor_counts(nothing) == 0).all()
    # the arguments are checked before the index is asked
    for call in (lambda: store.neighbor_counts(float("nan")), lambda: store.neighbor_counts([0.5, 0.6]),
                 lambda: store.density_labels(float("nan")), lambda: store.density_labels(0.9, min_samples=0),
                 lambda: store.density_clusters(0.9, min_samples=1.5)):
        with pytest.raises(ValueError):
            call()


def test_store_density_labels_are_group_keys(tmp_path, monkeypatch):
    store, q = _store(tmp_path, monkeypatch, "cosine")
    labels, kinds = store.density_labels(0.9975, min_samples=3)
    page = store.search_grouped(q[0].tolist(), 6, labels.tolist())
    ranked = store.search(q[0].tolist(), N)
    seen, heads = set(), []
    for r in ranked:  # a noise row is a group of its own
        i = int(r["metadata"]["photo_path"].split("/")[-1].split(".")[0])
        if labels[i] < 0 or labels[i] not in seen:
            seen.add(labels[i])
            heads.append((r["metadata"]["photo_path"], None if labels[i] < 0 else int(labels[i])))
    assert [(p["items"][0]["metadata"]["photo_path"], p["group"]) for p in page] == heads[:6]
    threshold = ranked[60]["distance"]
    got = store.facet_counts(q[0].tolist(), threshold, labels.tolist())
    hit = [labels[int(r["metadata"]["photo_path"].split("/")[-1].split(".")[0])] for r in ranked[:60]]
    assert got["total"] == 60 and got["ungrouped"] == sum(1 for k in hit if k < 0) > 0
    assert got["counts"] == {int(k): hit.count(k) for k in sorted(set(hit)) if k >= 0}


def test_store_density_of_an_empty_store(tmp_path, monkeypatch):
    store, _ = _store(tmp_path, monkeypatch, "cosine", fill=False)
    assert store.neighbor_counts(0.9).shape == (0,)
    labels, kinds = store.density_labels(0.9)
    assert labels.shape == kinds.shape == (0,)
    assert store.density_clusters(0.9) == []
    with pytest.raises(ValueError):
        store.density_labels(0.9, min_samples=0)

"""The streaming scans on either side of their query-in-LDS boundary (MI355X only).

A scan workgroup keeps two k-lists and a batch in LDS and, when it still fits the 148 KiB budget, the query as
fp64 beside them (QLDS); a longer query stays in global memory.  Each scan kernel is instantiated for both, with
and without an id list (SEL), and the launcher picks one.  These cases put every launcher on both sides of the
boundary, so a launcher that picks the wrong instantiation (and with it the wrong LDS layout) shows up here.

At a launched depth of 2049..4096 the lists take 4096 * 24 + 512 * 12 = 104448 B, which leaves 47104 B = 736
groups of 8 elements: d = 5888 is staged in LDS, d = 5896 is not.  The forced scan tiers launch at depth
min(k, members); N = 4608 rows and k = 2100 keep that at 2100 with and without a selector of exactly half the
rows (2304 members).  The small-corpus full scan (1-2 queries, k <= 64) keeps 64-entry lists: 64 * 24 + 512 * 12
= 7680 B leave 143872 B = 2248 groups, so d = 17984 is staged and d = 17992 is not.

Every answer is compared bit for bit, ids and scores, with the CPU oracle of the job's own test file.
"""
import numpy as np
import pytest

from oracle import oracle as O
from oracle_adjust_index import adjust_reference
from oracle_after_index import after_reference, full_ranking
from oracle_sel_index import filtered_reference
from test_gpu_adjust import _eq as adjust_eq
from test_gpu_after import _eq as after_eq

pytestmark = pytest.mark.gpu

PAIRS = [("f32", "ip"), ("bf16", "l2")]
N, K, NQ = 4608, 2100, 2
D_LDS, D_GLOBAL = 5888, 5896            # the last d staged in LDS and the first that is not, lists of 4096
SMALL_D_LDS, SMALL_D_GLOBAL = 17984, 17992  # the same for the small-corpus scan's lists of 64


@pytest.fixture(scope="module", params=[(dt, m, d) for dt, m in PAIRS for d in (D_LDS, D_GLOBAL)],
                ids=lambda p: f"{p[0]}-{p[1]}-d{p[2]}")
def world(request):
    """One index per (dtype, metric, d), shared by the three jobs: rows as stored, queries, the half mask."""
    from photo_search_engine_amd.index import FlatIndex
    dtype, metric, d = request.param
    rng = np.random.default_rng(d + len(dtype))
    x = rng.standard_normal((N, d)).astype(np.float32)
    q = rng.standard_normal((NQ, d)).astype(np.float32)
    mask = np.zeros(N, dtype=bool)
    mask[rng.choice(N, size=N // 2, replace=False)] = True
    xs = O.round_dtype(x, dtype)
    for a in (xs, q, mask):
        a.setflags(write=False)
    ix = FlatIndex(d, metric, dtype)
    ix.add(x)
    sel = ix.selector(mask)
    assert sel.count == N // 2 >= K  # (the launched depth min(k, members) stays k: lists of 4096)
    yield {"ix": ix, "sel": sel, "xs": xs, "q": q, "mask": mask, "metric": metric}
    sel.close()
    ix.close()


def test_sel_scan(world):
    w = world
    Dref, Iref = filtered_reference(w["xs"], w["q"], w["mask"], K, w["metric"])
    w["ix"].set_sel_mode("scan")
    try:
        D, I = w["ix"].search(w["q"], K, sel=w["sel"])
    finally:
        w["ix"].set_sel_mode("auto")
    assert w["ix"].sel_last_stats()["tier"] == "scan"
    np.testing.assert_array_equal(I, Iref)
    np.testing.assert_array_equal(D.view(np.uint32), Dref.view(np.uint32))


@pytest.mark.parametrize("masked", [False, True], ids=["rows", "selector"])
def test_adjust_scan(world, masked):
    w = world
    rng = np.random.default_rng(7)
    scale = rng.uniform(0.5, 1.5, N).astype(np.float32)
    bias = (rng.standard_normal(N) * 8).astype(np.float32)
    ref = adjust_reference(w["xs"], w["q"], scale, bias, K, w["metric"], w["mask"] if masked else None)
    adj = w["ix"].score_adjust(scale, bias)
    w["ix"].set_adjust_mode("scan")
    try:
        out = w["ix"].search_adjusted(w["q"], K, adj, sel=w["sel"] if masked else None, return_raw=True)
    finally:
        w["ix"].set_adjust_mode("auto")
        adj.close()
    st = w["ix"].adjust_last_stats()
    assert st["tier"] == "scan" and st["scan"] == NQ, st
    adjust_eq(out, ref, "adjusted scan")


@pytest.mark.parametrize("masked", [False, True], ids=["rows", "selector"])
def test_after_scan(world, masked):
    w = world
    mask = w["mask"] if masked else None
    # a cursor in mid-ranking: the row a quarter of the way down each query's ranking of every row
    after = np.array([order[N // 4] for _, order in full_ranking(w["xs"], w["q"], w["metric"])], dtype=np.int64)
    ref = after_reference(w["xs"], w["q"], after, K, w["metric"], mask)
    # (hundreds of members before the cursor and over a thousand behind it; under the selector the page ends padded)
    assert (ref[2] > 100).all() and (ref[1][:, 1000] >= 0).all()
    w["ix"].set_after_mode("scan")
    try:
        out = w["ix"].search_after(w["q"], K, after, sel=w["sel"] if masked else None, return_rank=True)
    finally:
        w["ix"].set_after_mode("auto")
    st = w["ix"].after_last_stats()
    assert st["tier"] == "scan" and st["scan"] == NQ, st
    after_eq(out, ref, "paged scan")


@pytest.mark.parametrize("d", [SMALL_D_LDS, SMALL_D_GLOBAL])
@pytest.mark.parametrize("dtype,metric", PAIRS)
def test_small_full_scan(dtype, metric, d):
    from photo_search_engine_amd.index import FlatIndex
    n, k = 128, 10
    ix = FlatIndex(d, metric, dtype)
    ix.add_synthetic(O.SEED_CORPUS, 0, n, True)
    q = O.synth_rows(O.SEED_QUERIES, 5, 1, d, True, "f32")
    ix.set_timing(True)
    D, I = ix.search(q, k)
    ix.set_timing(False)
    assert ix.timing_fetch()[1] == "full_scan"
    assert ix.full_scan_count() == 0 and ix.uncertified_count() == 0
    S, Ie = O.knn_exact(ix.reconstruct_n(0, n), q, k, metric)
    np.testing.assert_array_equal(I, Ie)
    np.testing.assert_array_equal(D.view(np.uint32), S.astype(np.float32).view(np.uint32))
    ix.close()

"""The exact row scorer (csrc/vs_device.h ``exact_score_rows``) against the oracle, bit for bit, at every
dimension where its loop takes another path (MI355X only).

Lane l of a wave owns the 8-element groups l, l + 64, ...; three groups per lane make a pass.  A pass whose
groups all exist (and d % 8 == 0) runs unguarded with one fp64 FMA per element; the rest keeps element
guards.  The d values below cover: element guards (d % 8 != 0), fewer groups than lanes, exactly one
group per lane, a partial last pass, one full pass (d = 1536), a full pass plus a remainder, and several
full passes.

Each case searches one small corpus on three routes, so that every dtype reaches
* the full scan (one query, a small corpus),
* ``k_refine`` (3-8 queries on the native screen: the GEMV screen's refine),
* ``k_refine_wide`` (a 16-query batch on the int8 screen -- the int8 screen takes batches of more than
  8 queries only; ``refine_rows_count`` must move there),
and compares the returned fp64 scores with ``oracle.canon_scores`` of the returned ids as int64 bit
patterns, and the ids with ``oracle.knn_exact``.  k is 1, 3, 5 or 10 and the corpora are no multiple of a
scoring round, so the last wave-round of a refine has absent rows.
"""
import functools

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

DS = [1, 7, 9, 100, 1535,   # remainder element guards
      8, 64,                # fewer groups than lanes
      512,                  # exactly one group per lane
      520, 1528,            # partial last pass
      1536,                 # one full pass (the cfg3 shape)
      1544,                 # full pass + remainder
      3072, 4096]           # several passes
DTYPES = ["bf16", "f16", "f32"]
METRICS = ["ip", "l2"]
KS = (1, 3, 5, 10)
NQ_WIDE = 16


def _shape(d, dtype, metric):
    """(rows, native-screen queries, k) of a case: 2k-6k rows, 3-8 queries, k in KS -- spread over the cases."""
    i = DS.index(d) if d in DS else 5
    j = i + DTYPES.index(dtype)
    return 2049 + 577 * (j % 7), 3 + j % 6, KS[(j + METRICS.index(metric)) % 4]


@functools.lru_cache(maxsize=4)
def _rows(d, dtype, n):
    return O.synth_rows(O.SEED_CORPUS, 0, n, d, True, dtype)


@functools.lru_cache(maxsize=4)
def _queries(d):
    return O.synth_rows(O.SEED_QUERIES, 0, NQ_WIDE, d, True, "f32")


@functools.lru_cache(maxsize=4)
def _reference(d, dtype, n, k, metric):
    """The oracle's exact top-k of all NQ_WIDE queries, computed once per case and shared by its routes."""
    return O.knn_exact(_rows(d, dtype, n), _queries(d), k, metric)


def _search(ix, q, k):
    import torch
    qd = torch.from_numpy(np.ascontiguousarray(q)).cuda()
    nq = q.shape[0]
    I = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    S = torch.empty((nq, k), dtype=torch.float64, device="cuda")
    ix.search_device_exact(qd.data_ptr(), nq, k, None, I.data_ptr(), S.data_ptr(), 0,
                           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return S.cpu().numpy(), I.cpu().numpy()


def _check(x, q, S, I, Se, Ie, metric, what):
    np.testing.assert_array_equal(I, Ie, err_msg=f"{what}: ids differ from the oracle")
    for a in range(q.shape[0]):
        want = O.canon_scores(x[I[a]], q[a:a + 1], metric)[0]
        assert np.array_equal(S[a].view(np.int64), want.view(np.int64)), \
            f"{what}: query {a}: scores are not the canonical scores of the returned ids, bit for bit"
    assert np.array_equal(S.view(np.int64), Se.view(np.int64)), f"{what}: scores differ from the oracle's"


def _run_case(d, dtype, metric, wide=True):
    from photo_search_engine_amd.index import FlatIndex
    n, nq, k = _shape(d, dtype, metric)
    x, q = _rows(d, dtype, n), _queries(d)
    Se, Ie = _reference(d, dtype, n, k, metric)
    ix = FlatIndex(d, metric, dtype, device=0)
    try:
        ix.add_synthetic(O.SEED_CORPUS, 0, n, True)
        # one query over a small corpus: the exact full scan alone
        S, I = _search(ix, q[:1], k)
        _check(x, q[:1], S, I, Se[:1], Ie[:1], metric, "full scan")
        # 3-8 queries, native screen: the GEMV screen, then k_refine
        S, I = _search(ix, q[:nq], k)
        _check(x, q[:nq], S, I, Se[:nq], Ie[:nq], metric, "k_refine")
        if wide:
            # a 16-query batch on the int8 screen: k_refine_wide
            ix.set_screen("int8")
            rows0 = ix.refine_rows_count()
            S, I = _search(ix, q, k)
            _check(x, q, S, I, Se, Ie, metric, "k_refine_wide")
            print(f"d={d} {dtype} {metric}: n={n} nq={nq} k={k} refine rows {ix.refine_rows_count() - rows0} "
                  f"uncertified {ix.uncertified_count()}")
            assert ix.refine_rows_count() > rows0, "the int8 batch did not reach k_refine_wide"
    finally:
        ix.close()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", DS)
def test_scores_bit_exact(d, dtype, metric):
    _run_case(d, dtype, metric)


@pytest.mark.parametrize("dtype", DTYPES)
def test_query_too_long_for_lds(dtype):
    # k_refine_wide keeps the fp64 query in LDS up to d = 6656; at d = 6912 the scorer reads it from global
    # memory (864 groups: four full passes, then a partial one for half the lanes)
    _run_case(6912, dtype, "ip")

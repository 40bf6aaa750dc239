"""The int8 screen's query credit on the GPU (``vs_set_i8_query_credit``).

A query whose own int8 rounding error is below the share every row's bound word carries for it gets
the difference back: its refine margin ``qeps`` goes negative and ``k_refine_wide`` scores fewer rows.
Both margins are proven, so the results must be the oracle's ids and canonical scores with the
credit on and off, for inner product and L2, above the GEMV limit (nq 9 and 64), k 10 and 100, on
the small-shard tiled form (16,384 x 512 bf16) and the smallest seeded direct form (262,144 x 512:
1024 tiles).  One batch holds Gaussian queries, a zero query (no credit), a flat query (all
``|q_i|`` equal: codes +-127, error ~0, the largest credit) and a spiky one (one coordinate 50x the
rest: error above the rows' share, the excess branch).  The small corpus carries adversarial rows for
the flat query, ``x_i = s (c_i + sign(q_i) / 4)`` with s a power of two, ``|c_i| <= 31`` and one
coordinate at 127 s pinning the scale (bf16-exact): their int8 error is parallel to the query, so
their true scores sit on their bounds, and their scores straddle the k-th best at k = 10 and 100 --
an over-claimed credit drops a true neighbour.  The scored-row counter (``vs_refine_rows_count``)
must fall with the credit on (Gaussian batch, 262,144 rows, k = 100) and stay equal where a zero row
leaves no credit.
"""
import functools
import math

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

D = 512
N_SMALL, N_BIG = 16384, 262144
N_ADV = 256
NQ_MAX, K_MAX = 64, 100
N_SPECIAL = 3  # zero, flat, spiky lead the query set; Gaussian queries follow


def _flat_signs():
    return np.random.default_rng(41).choice([-1.0, 1.0], size=D)


@functools.lru_cache(maxsize=None)
def _queries():
    """[zero, flat, spiky, 64 Gaussian]: a mixed batch of nq is rows [0, nq), a Gaussian one [3, 3 + nq)."""
    sig = _flat_signs()
    flat = (sig / math.sqrt(D)).astype(np.float32)
    spiky = np.ones(D)
    spiky[D // 3] = 50.0
    spiky = (spiky / np.linalg.norm(spiky)).astype(np.float32)
    g = O.synth_rows(O.SEED_QUERIES + 9, 0, NQ_MAX, D, True, "f32")
    q = np.concatenate([np.zeros((1, D), np.float32), flat[None], spiky[None], g], axis=0)
    q.setflags(write=False)
    return q


def _adversarial_rows():
    sig = _flat_signs()
    s = 2.0 ** -10
    m = np.random.default_rng(43).integers(0, 32, size=(N_ADV, D)).astype(np.float64)
    x = s * sig[None, :] * (m + 0.25)
    x[:, 0] = 127.0 * s * sig[0]
    x = x.astype(np.float32)
    assert np.array_equal(O.round_dtype(x, "bf16"), x)  # stored as built
    return x


def _adversarial_ids():
    return np.sort(np.random.default_rng(47).choice(N_SMALL, size=N_ADV, replace=False))


def _small_rows():
    x = O.synth_rows(O.SEED_CORPUS + 9, 0, N_SMALL, D, True, "bf16").copy()
    x[_adversarial_ids()] = _adversarial_rows()
    return x


def _make_index(metric, rows=None, n_synth=0):
    from photo_search_engine_amd.index import FlatIndex
    ix = FlatIndex(D, metric, "bf16")
    ix.set_scan_limit(0)
    if rows is not None:
        ix.add(rows)
    else:
        ix.add_synthetic(O.SEED_CORPUS + 9, 0, n_synth, True)
    ix.set_screen("int8")
    return ix


class _Case:
    """An index and the oracle's lists for every query of _queries() at K_MAX, computed once."""

    def __init__(self, metric, ix):
        self.metric, self.ix = metric, ix
        x = ix.reconstruct_n(0, ix.ntotal)
        self.S, self.I = O.knn_exact(x, _queries(), K_MAX, metric)
        self.S.setflags(write=False)
        self.I.setflags(write=False)

    def check(self, q0, nq, k):
        D_, I_ = self.ix.search(_queries()[q0:q0 + nq], k)
        Ie, Se = self.I[q0:q0 + nq, :k], self.S[q0:q0 + nq, :k]
        np.testing.assert_array_equal(I_, Ie)
        np.testing.assert_array_equal(D_, Se.astype(np.float32))
        return D_, I_


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(shape, metric):
        if (shape, metric) not in made:
            ix = _make_index(metric, rows=_small_rows()) if shape == "small" else _make_index(metric, n_synth=N_BIG)
            made[(shape, metric)] = _Case(metric, ix)
        return made[(shape, metric)]
    yield get
    for c in made.values():
        c.ix.close()


@pytest.fixture(autouse=True)
def credit_on_again():
    from photo_search_engine_amd.index import set_i8_query_credit
    yield
    set_i8_query_credit(True)


def test_switch_default_and_roundtrip():
    from photo_search_engine_amd.index import i8_query_credit, set_i8_query_credit
    assert i8_query_credit() is True
    set_i8_query_credit(False)
    assert i8_query_credit() is False
    set_i8_query_credit(True)
    assert i8_query_credit() is True


@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("shape", ["small", "big"])
@pytest.mark.parametrize("nq,k", [(9, 10), (9, 100), (64, 10), (64, 100)])
def test_gaussian_batch_exact_and_clean(cases, shape, metric, nq, k):
    from photo_search_engine_amd.index import set_i8_query_credit
    c = cases(shape, metric)
    before = (c.ix.uncertified_count(), c.ix.full_scan_count())
    D1, I1 = c.check(N_SPECIAL, nq, k)
    after = (c.ix.uncertified_count(), c.ix.full_scan_count())
    print(f"{shape} {metric} nq={nq} k={k}: uncertified, full scan {before} -> {after}")
    assert after == before  # the credit fails no certificate (file order: before == (0, 0))
    set_i8_query_credit(False)
    D0, I0 = c.check(N_SPECIAL, nq, k)
    np.testing.assert_array_equal(I0, I1)
    np.testing.assert_array_equal(D0, D1)
    assert (c.ix.uncertified_count(), c.ix.full_scan_count()) == before


def test_gaussian_counters_are_zero():
    """Gaussian batches only on a fresh index: both counters stay at 0 (inner product, both shapes'
    forms are covered by the unchanged-counter assertions above)."""
    ix = _make_index("ip", rows=_small_rows())
    x = ix.reconstruct_n(0, ix.ntotal)
    q = _queries()[N_SPECIAL:N_SPECIAL + NQ_MAX]
    S, Ie = O.knn_exact(x, q, K_MAX, "ip")
    for nq, k in [(9, 10), (64, 100)]:
        D_, I_ = ix.search(q[:nq], k)
        np.testing.assert_array_equal(I_, Ie[:nq, :k])
        np.testing.assert_array_equal(D_, S[:nq, :k].astype(np.float32))
    assert ix.uncertified_count() == 0 and ix.full_scan_count() == 0
    ix.close()


@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("shape", ["small", "big"])
@pytest.mark.parametrize("nq,k", [(9, 10), (9, 100), (64, 10), (64, 100)])
def test_mixed_batch_exact_switch_on_and_off(cases, shape, metric, nq, k):
    """zero + flat + spiky + Gaussian queries in one batch; on the small shape the flat query's
    adversarial rows straddle its k-th best."""
    from photo_search_engine_amd.index import set_i8_query_credit
    c = cases(shape, metric)
    if shape == "small" and metric == "ip":
        # the flat query's k best are adversarial rows, with more of them below: they straddle its k-th best
        assert np.isin(c.I[1, :k], _adversarial_ids()).all() and N_ADV > k
    D1, I1 = c.check(0, nq, k)
    set_i8_query_credit(False)
    D0, I0 = c.check(0, nq, k)
    np.testing.assert_array_equal(I0, I1)
    np.testing.assert_array_equal(D0, D1)


def _rows_scored(ix, on, q, k, Ie, Se):
    """Rows k_refine_wide scores for one exact search of q with the credit on / off, on the int8
    screen at its default union depth (a batch with failed certificates would deepen it)."""
    from photo_search_engine_amd.index import set_i8_query_credit
    set_i8_query_credit(on)
    st = ix.screen_state()
    assert st["i8_union_log2"] == 0 and st["i8_routed_searches"] == 0
    r0 = ix.refine_rows_count()
    D_, I_ = ix.search(q, k)
    np.testing.assert_array_equal(I_, Ie)
    np.testing.assert_array_equal(D_, Se.astype(np.float32))
    return ix.refine_rows_count() - r0


def test_credit_scores_fewer_rows(cases):
    """Gaussian batch, 262,144 rows, k = 100, on an index of its own: the mixed batches above leave
    the shared one with a deeper int8 union or routed to the native screen (their zero query fails the
    int8 certificate; the screen-health feedback)."""
    c = cases("big", "ip")  # the same rows: its oracle lists serve
    ix = _make_index("ip", n_synth=N_BIG)
    q = _queries()[N_SPECIAL:N_SPECIAL + NQ_MAX]
    Ie, Se = c.I[N_SPECIAL:N_SPECIAL + NQ_MAX], c.S[N_SPECIAL:N_SPECIAL + NQ_MAX]
    off = _rows_scored(ix, False, q, K_MAX, Ie, Se)
    on = _rows_scored(ix, True, q, K_MAX, Ie, Se)
    print(f"rows scored per query, 262144 x 512, k = 100: credit off {off / NQ_MAX:.1f}, on {on / NQ_MAX:.1f}")
    assert ix.uncertified_count() == 0 and ix.full_scan_count() == 0
    ix.close()
    assert 0 < on < off


@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_zero_row_leaves_no_credit(metric):
    x = _small_rows()
    x[12345] = 0.0
    ix = _make_index(metric, rows=x)
    S, Ie = O.knn_exact(ix.reconstruct_n(0, ix.ntotal), _queries(), K_MAX, metric)
    g = slice(N_SPECIAL, N_SPECIAL + NQ_MAX)
    counts = [_rows_scored(ix, on, _queries()[g], K_MAX, Ie[g], S[g]) for on in (False, True)]
    print(f"{metric}, one zero row: rows scored with the credit off / on {counts}")
    assert counts[0] == counts[1] > 0
    # and the mixed batch (zero, flat and spiky queries) stays exact
    D_, I_ = ix.search(_queries()[:NQ_MAX], K_MAX)
    np.testing.assert_array_equal(I_, Ie[:NQ_MAX])
    np.testing.assert_array_equal(D_, S[:NQ_MAX].astype(np.float32))
    ix.close()

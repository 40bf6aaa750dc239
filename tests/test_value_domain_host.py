"""The premises of tests/test_gpu_value_domain.py, on the oracle alone (no GPU).

* Scaling rows by 2^a and queries by 2^b commutes with every rounding of the canonical fp64 score
  and of the f32 / bf16 storage formats while nothing underflows or overflows: ``O.knn_exact``,
  ``ivf_oracle.search`` and ``filtered_reference`` return the unit-scale ids, with scores times
  2^(a+b) (inner product) or 2^(2a) (L2, a == b), bit for bit, at every pair of group A.
* Every input of groups B to E is finite as stored and its reference top-k holds no two equal fp64
  scores, so the ids the GPU must return are decided by the scores alone.
"""
import numpy as np
import pytest

import value_domain_case as V
from oracle import ivf_oracle as IO
from oracle import oracle as O
from oracle_sel_index import filtered_reference


def _reference(path, x_st, q, metric):
    """(S fp64 nq x k, I) of a path's oracle: the flat search, the filtered one, or IVF."""
    family = V.PATHS[path][0]
    k = V.shape_of(path)[1]
    if family == "sel":
        ids = np.flatnonzero(V.sel_mask(path))
        S, Il = O.np_topk(O.canon_scores(x_st[ids], q, metric), k, metric)
        D, I = filtered_reference(x_st, q, V.sel_mask(path), k, metric)
        np.testing.assert_array_equal(I, ids[Il])
        np.testing.assert_array_equal(D, S.astype(np.float32))
        return S, I
    if family == "ivf":
        nlist, nprobe = V.IVF_LISTS[path]
        c = IO.sample_centroids(x_st, nlist, V.IVF_CENTROID_SEED)
        return IO.search(x_st, np.arange(x_st.shape[0]), IO.assign(x_st, c, metric), c, q, k, nprobe, metric)
    return O.knn_exact(x_st, q, k, metric)


_unit = {}


def _unit_reference(path, dtype, metric):
    key = (path, dtype, metric)
    if key not in _unit:
        x, q = V.base(V.shape_of(path))
        _unit[key] = _reference(path, O.round_dtype(x, dtype), q, metric)
    return _unit[key]


def _dedup(cases):
    # paths that share (family, shape, lists) share their oracle problem
    seen, out = set(), []
    for c in cases:
        fam = V.PATHS[c[0]][0]
        key = ("flat" if fam == "plain" else fam, V.shape_of(c[0]), V.IVF_LISTS.get(c[0]), c[1:])
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


@pytest.mark.parametrize("path,dtype,metric,a,b", _dedup([c for c in V.CASES_A if V.covariant(*c[2:])]))
def test_power_of_two_scaling_commutes_with_the_oracle(path, dtype, metric, a, b):
    x, q = V.scaled(V.shape_of(path), a, b)
    x_st = O.round_dtype(x, dtype)
    # the storage rounding itself commutes
    np.testing.assert_array_equal(x_st, O.round_dtype(V.base(V.shape_of(path))[0], dtype) * V.pow2(a))
    S, I = _reference(path, x_st, q, metric)
    S1, I1 = _unit_reference(path, dtype, metric)
    np.testing.assert_array_equal(I, I1)
    f = V.factor(metric, a, b)
    np.testing.assert_array_equal(S, S1 * f)
    np.testing.assert_array_equal(S.astype(np.float32), S1.astype(np.float32) * np.float32(f))
    assert np.isfinite(S).all() and (np.abs(S.astype(np.float32)) >= np.finfo(np.float32).tiny).all()


def _finite_and_tie_free(path, dtype, metric, x, q):
    x_st = O.round_dtype(x, dtype)
    assert np.isfinite(x_st).all() and np.isfinite(q).all()
    S, I = _reference(path, x_st, q, metric)
    assert (I >= 0).all() and np.isfinite(S).all()
    assert (np.diff(S, axis=1) != 0).all(), "fp64 ties inside the compared top-k"
    return x_st


@pytest.mark.parametrize("path,dtype,metric,a,b", _dedup(V.CASES_B + V.CASES_C))
def test_scaled_inputs_are_finite_and_tie_free(path, dtype, metric, a, b):
    x, q = V.scaled(V.shape_of(path), a, b)
    _finite_and_tie_free(path, dtype, metric, x, q)


def test_f16_cases_cross_the_subnormal_boundary():
    # what group C is for: at 2^-12 nearly every stored element is an f16 subnormal (|v| < 2^-14),
    # at 2^-20 most are subnormal and the rest round to zero
    x, _ = V.scaled(V.shape_of("mfma16_tiled"), -12, 0)
    st = O.round_dtype(x, "f16")
    sub = (st != 0) & (np.abs(st) < 2.0 ** -14)
    assert sub.mean() > 0.99
    x, _ = V.scaled(V.shape_of("mfma16_tiled"), -20, 0)
    st = O.round_dtype(x, "f16")
    sub = (st != 0) & (np.abs(st) < 2.0 ** -14)
    assert 0.6 < sub.mean() < 0.85 and 0.15 < (st == 0).mean() < 0.4


@pytest.mark.parametrize("path,dtype,metric", _dedup(V.CASES_D))
def test_norm_spread_inputs_are_finite_and_tie_free(path, dtype, metric):
    x, q = V.spread(V.shape_of(path), dtype)
    x_st = _finite_and_tie_free(path, dtype, metric, x, q)
    n = np.linalg.norm(x_st.astype(np.float64), axis=1)
    lo, hi = (-12, 12) if dtype == "f16" else (-20, 20)
    assert n.min() < 2.0 ** (lo + 1) and n.max() > 2.0 ** (hi - 1)


@pytest.mark.parametrize("path,dtype,metric", _dedup(V.CASES_E))
def test_outlier_inputs_are_finite_and_tie_free(path, dtype, metric):
    x, q = V.outliers(V.shape_of(path))
    _finite_and_tie_free(path, dtype, metric, x, q)
    x0, q0 = V.base(V.shape_of(path))
    assert ((x != x0).sum(axis=1) == (np.arange(x.shape[0]) % 97 == 0)).all()
    assert ((q != q0).sum(axis=1) == (np.arange(q.shape[0]) % 5 == 0)).all()


@pytest.mark.parametrize("metric,s", V.CASES_F)
def test_two_phase_shard_inputs_are_tie_free(metric, s):
    nq, k, N, d = V.F_SHAPE
    x, q = V.scaled(V.F_SHAPE, s, s)
    S, I = O.knn_exact(O.round_dtype(x, "bf16"), q, k, metric)
    assert np.isfinite(S).all() and (np.diff(S, axis=1) != 0).all()

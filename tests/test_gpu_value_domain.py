"""Exactness off unit scale (MI355X only): input magnitudes, f16 subnormals, norm spread.

Every other GPU test feeds unit-norm rows and queries (the widest departure: row norms in
[0.25, 4)).  The screens' margins are hand-derived error bounds with a few absolute constants inside
relative terms, ``sqn`` / ``maxsq`` are fp32 sums of squares, f16 rows may be stored as subnormals,
and the L2 margins use the global max ||x||: all of it value-dependent, none of it driven before.

Bar of every case (``_check_exact`` of tests/test_gpu_parity.py): on a fresh index, ids bit-equal and
D bit-equal to the fp32 rounding of the canonical fp64 score of ``oracle.knn_exact`` (IVF:
``ivf_oracle.search``; selectors: ``filtered_reference``) over the rows read back from the index,
which must themselves equal ``O.round_dtype`` of the input.  Inputs, groups A to F and the path
table: tests/value_domain_case.py; their premises (power-of-two scaling commutes with the oracle,
no fp64 ties in any compared top-k): tests/test_value_domain_host.py.

Group A, where the scaled problem is the unit-scale problem times a power of two (inner product at
every pair; L2 when rows and queries share the scale), adds: ids equal to the unit-scale ids, D equal
to the unit-scale D times 2^(a+b) (L2: 2^(2a)) bit for bit, D within 1e-5 times that factor of the
faiss fp32 restatement, and -- for a + b >= -40 -- the unit-scale ``uncertified_count`` /
``full_scan_count`` (every margin term is scale-covariant except the absolute constants, ~1e-30,
which reach ~10 % of the margin only at 2^-80).  L2 with a != b is another problem (||q||^2 or
||x||^2 swamps the cross term): the oracle bar alone, counters recorded.

Counters that are recorded and not asserted are printed as ``VALUE_DOMAIN {json}`` lines.

Kernel kinds: the last timed kernel of the search must be the path's (``timing_fetch``).  A query
whose first-pass certificate fails is re-searched alone, 4x deeper per round, on the GEMV screen
(``vs_search``), which is then the last timed kernel: ``gemv`` is accepted in place of the path's kind
only with ``uncertified_count() > 0`` and at least two timed launches.  The int8 GEMV of groups D and
E may also hand over to the native GEMV by design: its depth estimate (``i8_gemv_depth``) grows with
the rows' largest code error relative to max ||x||, which one outlier element per row makes large.

Found by this file and fixed: ``i8_gemv_depth`` took the largest row error norm as an absolute
number, so rows scaled by 2^12 or more never reached the int8 GEMV (cases A at a = 40, B at (12, 0)
and C at (14, 0) of the ``i8_gemv`` path reported ``gemv``) and rows scaled by 2^-40 got the minimum
depth; it is now taken relative to max ||x||.

Found by group D and fixed: the L2 certificate of ``refine`` bounded every unlisted row's key error
by the global max ||x||: gamma (max||x||^2 + 2 max||x|| ||q||) ~ 1.5e-5 * 2^40 with row norms up
to 2^20, against distances of ~1.  Every L2 query of the flat paths went through the re-searches
(mfma16_tiled: 40 of 40 to the exact full scan), and ``vs_ivf_search``, which has no scan behind its
deepest screen, returned VS_ERR_UNCERTIFIED for all 40 queries of ``ivf_mfma`` (20,000 probed rows,
4,096 listed at most).  A row of norm above ||q|| + sqrt(D_k) is farther than the k-th best by the
triangle inequality, so the margin now stops at that norm (``test_l2_margin_stops_at_reachable_norms``).
"""
import json

import numpy as np
import pytest

import value_domain_case as V
from oracle import ivf_oracle as IO
from oracle import oracle as O
from oracle_sel_index import filtered_reference

pytestmark = pytest.mark.gpu


def _emit(**kw):
    print("VALUE_DOMAIN " + json.dumps(kw, sort_keys=True))


def _screened(d, metric, dtype, plain=False):
    # (the Screened subclass of the other GPU files: calls of 1-2 queries on a small corpus would
    # otherwise take the exact full scan, which is the "small_scan" path's own subject)
    from photo_search_engine_amd.index import FlatIndex

    class Screened(FlatIndex):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.set_scan_limit(0)
    return (FlatIndex if plain else Screened)(d, metric, dtype)


def _kind_ok(want, ran, uncertified, lenient, timed):
    if ran == want:
        return True
    if lenient and want == "gemv_i8" and ran == "gemv":
        return True
    # re-searched queries: the first pass and at least one single-query GEMV were timed
    return uncertified > 0 and ran == "gemv" and timed >= 2


def _run_flat(tag, path, dtype, metric, x, q, faiss_bound, lenient):
    family, screen, (nq, k, N, d), want = V.PATHS[path]
    ix = _screened(d, metric, dtype, plain=family == "plain")
    try:
        ix.add(x)
        if screen == "int8":
            ix.set_screen("int8")
        x_st = ix.reconstruct_n(0, N)
        np.testing.assert_array_equal(x_st, O.round_dtype(x, dtype))  # (f16: subnormals stored RNE)
        info, timed = {}, 0
        if family == "sel":
            mask = V.sel_mask(path)
            ix.set_sel_mode(screen)
            D, I = ix.search(q, k, sel=mask)
            st = ix.sel_last_stats()
            ran, info["rescanned"] = st["tier"], st["rescanned"]
            Dexp, Iexp = filtered_reference(x_st, q, mask, k, metric)
        else:
            ix.set_timing(True)
            D, I = ix.search(q, k)
            ix.set_timing(False)
            ms, ran = ix.timing_fetch()
            timed = len(ms)
            S, Iexp = O.knn_exact(x_st, q, k, metric)
            Dexp = S.astype(np.float32)
        state = ix.screen_state()
        info.update(uncertified=ix.uncertified_count(), full_scan=ix.full_scan_count(), ran=ran,
                    i8_union_log2=state["i8_union_log2"], i8_routed=state["i8_routed_searches"],
                    native_seed_log2=state["native_seed_log2"])
        _emit(case=tag, path=path, dtype=dtype, metric=metric, **info)
        np.testing.assert_array_equal(I, Iexp)
        np.testing.assert_array_equal(D, Dexp)
        assert _kind_ok(want, ran, info["uncertified"], lenient, timed), (want, ran, timed)
        if faiss_bound is not None and family in ("flat", "plain"):
            Df, _ = O.knn_faiss_fp32(x_st, q, k, metric)
            err = float(np.max(np.abs(D.astype(np.float64) - Df)))
            _emit(case=tag, path=path, dtype=dtype, metric=metric, faiss_err=err, faiss_bound=faiss_bound)
            assert err <= faiss_bound
        return [(D, I, info)]
    finally:
        ix.close()


def _run_ivf(tag, path, dtype, metric, x, q):
    from photo_search_engine_amd.ivf import IVFFlatIndex
    _, scan, (nq, k, N, d), _ = V.PATHS[path]
    nlist, nprobe = V.IVF_LISTS[path]
    x_st = O.round_dtype(x, dtype)
    ix = IVFFlatIndex(d, nlist, metric, dtype)
    try:
        # centroids drawn from the scaled rows: they carry the rows' scale
        ix.set_centroids(IO.sample_centroids(x_st, nlist, V.IVF_CENTROID_SEED))
        c = ix.centroids()
        ix.add(x)
        for i in (0, N // 2, N - 1):
            np.testing.assert_array_equal(ix.reconstruct(i), x_st[i])
        S, Iexp = IO.search(x_st, np.arange(N), IO.assign(x_st, c, metric), c, q, k, nprobe, metric)
        assert (Iexp >= 0).all()
        out = []
        # the GEMV scan is the library's own choice at 5 queries; the MFMA scan is forced, on split
        # (hi, lo) query tiles and on plain ones (d = 256: the direct mapped form, d16_direct_ok)
        for tiles in ((None,) if scan == "gemv" else ("split", "plain")):
            if tiles:
                ix.set_scan("mfma")
                ix.set_query_tiles(tiles)
            D, I = ix.search(q, k, nprobe)
            scans, redone = ix.last_search_stats()
            info = {"mfma_lists": scans, "uncertified": redone, "tiles": tiles}
            _emit(case=tag, path=path, dtype=dtype, metric=metric, **info)
            np.testing.assert_array_equal(I, Iexp)
            np.testing.assert_array_equal(D, S.astype(np.float32))
            assert scans == 0 if scan == "gemv" else scans > 0
            out.append((D, I, info))
        return out
    finally:
        ix.close()


def _run(tag, path, dtype, metric, x, q, faiss_bound=None, lenient=False):
    """One fresh index over ``x``, one search of ``q`` along ``path`` (IVF MFMA: one per query-tile
    form), held to the oracle bar and to the path's kernel; returns [(D, I, counters)]."""
    if V.PATHS[path][0] == "ivf":
        return _run_ivf(tag, path, dtype, metric, x, q)
    return _run_flat(tag, path, dtype, metric, x, q, faiss_bound, lenient)


_unit_runs = {}


def _unit(path, dtype, metric):
    """The unit-scale run of a case (once per path, dtype and metric; each on its own index)."""
    key = (path, dtype, metric)
    if key not in _unit_runs:
        x, q = V.base(V.shape_of(path))
        _unit_runs[key] = _run("unit", path, dtype, metric, x, q, faiss_bound=1e-5)
    return _unit_runs[key]


@pytest.mark.parametrize("path,dtype,metric,a,b", V.CASES_A)
def test_power_of_two_scaling(path, dtype, metric, a, b):
    x, q = V.scaled(V.shape_of(path), a, b)
    cov = V.covariant(metric, a, b)
    f = V.factor(metric, a, b)
    runs = _run(f"A({a},{b})", path, dtype, metric, x, q, faiss_bound=1e-5 * f if cov else None)
    if not cov:
        return
    for (D, I, info), (D1, I1, info1) in zip(runs, _unit(path, dtype, metric)):
        np.testing.assert_array_equal(I, I1)
        np.testing.assert_array_equal(D, D1 * np.float32(f))
        if a + b >= -40:
            assert info == info1  # counters, tier reached and kernel of the unit-scale run


@pytest.mark.parametrize("a", [-40, 12, 40])
def test_int8_gemv_depth_ignores_the_rows_scale(a):
    # regression: the int8 GEMV's depth estimate took the largest row error norm as an absolute
    # number, so from a row scale of ~2^12 on it exceeded the int8 GEMV's deepest list and every
    # few-query search fell to the native GEMV (still exact, twice the bytes streamed)
    x, q = V.scaled(V.shape_of("i8_gemv"), a, 0)
    (_, _, info), = _run(f"depth({a})", "i8_gemv", "bf16", "ip", x, q)
    assert info["ran"] == "gemv_i8" and info["uncertified"] == 0


@pytest.mark.parametrize("path,dtype,metric,a,b", V.CASES_B)
def test_l2_mismatched_scales(path, dtype, metric, a, b):
    # distances dominated by ||x||^2 (a = 12) or ||q||^2 (b = 12): dozens of equal fp32 D values in a
    # list whose fp64 scores all differ, so only the canonical fp64 order separates the rows
    x, q = V.scaled(V.shape_of(path), a, b)
    _run(f"B({a},{b})", path, dtype, metric, x, q)


@pytest.mark.parametrize("path,dtype,metric,a,b", V.CASES_C)
def test_f16_rows_small_and_large(path, dtype, metric, a, b):
    # a = -12: 99.8 % of the stored elements are f16 subnormals; a = -20: 73 % subnormal, 27 % zero;
    # a = 14: elements up to ~2^13, under the f16 maximum
    x, q = V.scaled(V.shape_of(path), a, b)
    _run(f"C({a},{b})", path, dtype, metric, x, q)


@pytest.mark.parametrize("path,dtype,metric", V.CASES_D)
def test_norm_spread(path, dtype, metric):
    # one global max ||x|| (2^20; f16: 2^12) in every query's margin: the deeper tiers may run
    x, q = V.spread(V.shape_of(path), dtype)
    _run("D", path, dtype, metric, x, q, lenient=True)


@pytest.mark.parametrize("path", ["mfma16_tiled", "ivf_mfma"])
def test_l2_margin_stops_at_reachable_norms(path):
    # regression (see the module docstring): rows of norm 2^20 among rows of norm 2^-20 must not
    # keep the L2 queries from certifying; the unlisted rows that can reach the k-th best distance
    # (~0.97) have norms under ||q|| + sqrt(D_k) ~ 2, where the margin of a re-search (fp32 or split
    # queries) is ~3e-4, below the gap between the 10th and the 24th best distance of every query
    # (oracle: >= 4.7e-3 flat, >= 2.7e-3 in the two lists), so no query needs the exact full scan
    # and the IVF search, which has none, answers
    x, q = V.spread(V.shape_of(path), "bf16")
    for _, _, info in _run("D-margin", path, "bf16", "l2", x, q):
        assert info.get("full_scan", 0) == 0


@pytest.mark.parametrize("path,dtype,metric", V.CASES_E)
def test_outlier_elements(path, dtype, metric):
    # one element 1024 times the others sets the row's (query's) int8 scale: the other elements'
    # codes are 0 or +-1, the row error norm is nearly the row norm
    x, q = V.outliers(V.shape_of(path))
    _run("E", path, dtype, metric, x, q, lenient=True)


@pytest.mark.parametrize("metric,s", V.CASES_F)
def test_two_phase_one_shard_holds_the_global_topk(metric, s):
    """Phase A sizes the shard's int8 union for ceil(k / world) rows; here every other rank
    contributed nothing, so the floor of phase B is the shard's own phase-A list and the shard must
    still return all k rows exactly, without the full scan."""
    import torch
    nq, k, N, d = V.F_SHAPE
    x, q = V.scaled(V.F_SHAPE, s, s)
    ix = _screened(d, metric, "bf16")
    try:
        ix.add(x)
        ix.set_screen("int8")
        assert ix.two_phase_ok(nq, k)
        Se, Ie = O.knn_exact(ix.reconstruct_n(0, N), q, k, metric)
        qd = torch.from_numpy(q).cuda()
        Sa = torch.empty((nq, k), dtype=torch.float64, device="cuda")
        Ia = torch.empty((nq, k), dtype=torch.int64, device="cuda")
        S = torch.empty((nq, k), dtype=torch.float64, device="cuda")
        I = torch.empty((nq, k), dtype=torch.int64, device="cuda")
        D = torch.empty((nq, k), dtype=torch.float32, device="cuda")
        u0 = ix.uncertified_count()
        p = ix.search_phase_a(qd.data_ptr(), nq, k, V.F_WORLD, Sa.data_ptr(), Ia.data_ptr(), 0)
        ix.search_phase_b(p, Sa.data_ptr(), D.data_ptr(), I.data_ptr(), S.data_ptr())
        torch.cuda.synchronize()
        full = ix.full_scan_count()
        _emit(case=f"F({s},{s})", path="two_phase", dtype="bf16", metric=metric,
              uncertified=ix.uncertified_count() - u0, full_scan=full)
        np.testing.assert_array_equal(I.cpu().numpy(), Ie)
        np.testing.assert_array_equal(S.cpu().numpy(), Se)
        np.testing.assert_array_equal(D.cpu().numpy(), Se.astype(np.float32))
        assert full == 0
    finally:
        ix.close()

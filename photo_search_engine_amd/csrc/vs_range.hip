// vs_range.hip -- exact range search: every row within a score radius (include/vs.h "range search").
//
// faiss answers "which rows score at least this well" with IndexFlat::range_search; the reference
// product cuts a guessed top-k at score floors instead (core/searcher.py:822-843 of the reference).
// A row belongs to query q's answer iff D = (float)S passes the radius (D > r_q inner product,
// D < r_q squared L2), S the canonical fp64 score of exact_score_rows (vs_device.h).  Kernels
// (k_range_scan and k_range_refine live in vs_range_scan.h, templated on what a passing row goes into:
// here the pair buffer, in vs_facet.hip a histogram):
//   * k_range_scan (SCAN tier): streams like fs_scan_body -- workgroup b takes positions
//     [n b / G, n (b + 1) / G) of the row sequence, or of a selector's ascending id list -- scores
//     every row with exact_score_rows and tests it.  The output size is unknown, so this file takes
//     the ONE-PASS design: passing (S, id) pairs are appended to the query's region of a bounded pair
//     buffer through a wave-aggregated atomic (the wave's lane 0 holds its rows' scores and adds
//     their count once); a pair is stored only while its slot is inside the region, the counter
//     keeps counting past the end, and the host reruns an overflowed query with a region of the
//     counted size.  No row is scored twice unless its query overflowed.  Queries taken from stored
//     rows (vs_range_search_rows) carry their row's id: the row itself (VS_SELF_DROP) or every row
//     at or below it (VS_SELF_ABOVE) is rejected before it is counted, and under ABOVE without a
//     selector the workgroups split [row0, n_valid) -- the rows that can still pass -- instead.
//   * k_range_thr + k_range_refine (SCREEN tier): the native MFMA screen (launch_screen_mfma, as
//     vs_search launches it) starts at thr0[q], a key below every key a passing row can get (the
//     proof is at k_range_thr); k_range_refine scores each query's survivors exactly, several rows
//     per wave in flight as the refine does, applies the exact predicate and appends the passing
//     pairs as the scan does.
//   * k_range_emit: one workgroup per query sorts its segment best first in LDS
//     (sort_valid_best_first, up to RS_SORT_MAX pairs) and writes D = (float)S, I and S at the
//     query's offset; longer segments are copied as they are and sorted on the host.
// Every store is bounded by a capacity the host allocated: a pair slot by cap[q], an output slot by
// the segment lengths the host read back.  Plain vector stores and returning atomics only.
#include "vs_range_scan.h"

namespace vs {

// ---- SCAN tier ------------------------------------------------------------------------------------
// (k_range_scan, k_range_refine and their launchers: vs_range_scan.h, here with the pair sink)
static bool pair_args_ok(const RangeArgs& a) {
    return a.off && a.cap && a.cnt && a.psc && a.pid &&
           (a.self_mode == VS_SELF_KEEP || ((a.self_mode == VS_SELF_DROP || a.self_mode == VS_SELF_ABOVE) && a.self));
}

hipError_t launch_range_scan(const RangeArgs& a, int G, int qy, const uint32_t* ids, int64_t m, hipStream_t st) {
    if (!pair_args_ok(a)) return hipErrorInvalidValue;
    if (a.self_mode != VS_SELF_KEEP) return rs_launch_scan<RsPairSink, true>(a, {}, 0, 0, G, qy, ids, m, st);
    return rs_launch_scan<RsPairSink, false>(a, {}, 0, 0, G, qy, ids, m, st);
}

// ---- SCREEN tier: the starting threshold ------------------------------------------------------------
// The screen's key of a row is its fp32 MFMA score over the dtype-rounded query q^ (inner product:
// <x, q^>; L2: 2 <x, q^> - ||x||^2, the transformed score qq - dist up to the constant qq = ||q||^2).
// The refine's certificate (refine(), vs_kernels.hip) rests on the bound  t <= key + eps  for every
// row, t the exact transformed score, with
//   IP:  eps = (gamma ||q^|| + ||q^ - q||) xmax 1.01
//   L2:  eps = 2 (gamma ||q^|| + ||q^ - q||) xe 1.01 + (gamma + 4u)(xe^2 + 2 xe ||q^||) 1.01 + 1e-12 (qq + xe^2),
//        xe an upper bound of the norm of every row that matters: a row at distance < r has
//        ||x|| <= ||q|| + sqrt(r), so xe = min(xmax, (||q|| + sqrt(r)) (1 + 1e-4)).
// Survivors contain the answer: a row in the answer has D past r, hence S past r (r is an fp32 value
// and the rounding is monotonic), hence t > T (T = r for IP, qq - r for L2), hence key >= t - eps >
// T - eps >= key_score(thr0): the screen keeps it (keys > thr0), unless a workgroup compacts -- which
// it reports in drop[q].
__global__ void __launch_bounds__(256) k_range_thr(int metric, const float* __restrict__ radius,
                                                   const float* __restrict__ qinfo, const float* __restrict__ q, int d,
                                                   int nq, float xmax, float gamma, u64* __restrict__ thr0) {
    const int qi = blockIdx.x * 256 + threadIdx.x;
    if (qi >= nq) return;
    const double r = (double)radius[qi];
    const double qh = (double)qinfo[2 * qi], dq = (double)qinfo[2 * qi + 1];
    const double xm = (double)xmax;
    double eps = ((double)gamma * qh + dq) * xm * 1.01 + 1e-30;
    double T = r;
    if (metric == METRIC_L2) {
        double qq = 0.0;
        for (int i = 0; i < d; ++i) {
            const double v = (double)q[(int64_t)qi * d + i];
            qq += v * v;
        }
        const double xe = fmin(xm, (sqrt(qq) + sqrt(fmax(r, 0.0))) * (1.0 + 1e-4));
        eps = ((double)gamma * qh + dq) * xe * 1.01 + 1e-30;
        eps = 2.0 * eps + ((double)gamma + 4.0 * 5.9604644775390625e-08) * (xe * xe + 2.0 * xe * qh) * 1.01 +
              1e-12 * (qq + xe * xe);
        T = qq - r;
    }
    const double lo = T - eps;
    u64 t = 0ull;  // keep every row
    if (lo > -3.0e38) {
        // an fp32 value strictly below lo: the rounded value, two steps down in the key order
        const uint32_t o = ord_f32((float)fmin(lo, 3.4e38));
        t = (u64)(o - 2u) << 32;
    }
    thr0[qi] = t;
}

hipError_t launch_range_thr(int metric, const float* radius, const float* qinfo, const float* q, int d, int nq,
                            float xmax, float gamma, u64* thr0, hipStream_t st) {
    if (!radius || !qinfo || !q || !thr0 || nq <= 0 || d <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_range_thr, dim3((nq + 255) / 256), dim3(256), 0, st, metric, radius, qinfo, q, d, nq, xmax,
                       gamma, thr0);
    return hipGetLastError();
}

// ---- SCREEN tier: exact refine of the survivors ------------------------------------------------------
hipError_t launch_range_refine(const RangeArgs& a, const u64* glist, const int* gcnt, int lcap, int ny,
                               hipStream_t st) {
    if (!pair_args_ok(a)) return hipErrorInvalidValue;
    if (a.self_mode != VS_SELF_KEEP) return rs_launch_refine<RsPairSink, true>(a, {}, glist, gcnt, lcap, ny, st);
    return rs_launch_refine<RsPairSink, false>(a, {}, glist, gcnt, lcap, ny, st);
}

// ---- emit ------------------------------------------------------------------------------------------
template <int METRIC>
__global__ void __launch_bounds__(FS_THREADS) k_range_emit(RangeEmitArgs a) {
    __shared__ double sc[RS_SORT_MAX];
    __shared__ uint32_t ids[RS_SORT_MAX];
    const int tid = threadIdx.x;
    const RangeSeg sg = a.seg[blockIdx.x];
    if (sg.n <= 0) return;
    const double* ps = a.psc[sg.buf & 1] + sg.src;
    const uint32_t* pi = a.pid[sg.buf & 1] + sg.src;
    if (sg.n > RS_SORT_MAX) {  // as it is: the host sorts it
        for (int64_t j = tid; j < sg.n; j += FS_THREADS) {
            const double s = ps[j];
            a.S[sg.dst + j] = s;
            a.D[sg.dst + j] = (float)s;
            a.I[sg.dst + j] = (int64_t)pi[j] + a.id_offset;
        }
        return;
    }
    const int n = (int)sg.n;
    int n2 = 64;
    while (n2 < n) n2 <<= 1;
    for (int j = tid; j < n2; j += FS_THREADS) {
        sc[j] = j < n ? ps[j] : (METRIC == METRIC_IP ? -INFINITY : INFINITY);
        ids[j] = j < n ? pi[j] : 0xFFFFFFFFu;
    }
    __syncthreads();
    sort_valid_best_first<METRIC>(sc, ids, n, n2);
    for (int j = tid; j < n; j += FS_THREADS) {
        a.S[sg.dst + j] = sc[j];
        a.D[sg.dst + j] = (float)sc[j];
        a.I[sg.dst + j] = (int64_t)ids[j] + a.id_offset;
    }
}

hipError_t launch_range_emit(const RangeEmitArgs& a, int nq, hipStream_t st) {
    if (nq <= 0 || !a.seg || !a.D || !a.I || !a.S || !a.psc[0] || !a.pid[0]) return hipErrorInvalidValue;
    const bool known = with_metric(a.metric, [&](auto metric) {
        launch_kernel(k_range_emit<metric>, 0, dim3(nq), dim3(FS_THREADS), 0, st, a);
    });
    return known ? hipGetLastError() : hipErrorInvalidValue;
}

}  // namespace vs

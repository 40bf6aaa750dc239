// vs_facet.hip -- exact facet counts: matching rows per group within a radius (include/vs.h "facet
// counts").
//
// The kernels are the range search's (vs_range_scan.h) with another sink: the scan's K loop, its
// exact_score_rows call and its predicate are the same code, and a row that passes is counted into
// hist[q][bin] instead of being appended to a pair buffer.
//   * k_range_scan with the count sink (SCAN tier), global form: lane 0 of a wave holds its R rows'
//     scores, merges equal bins among them and sends one 64-bit device atomic per distinct bin.
//   * the same, LDS form: G + 1 uint32 bins sit in dynamic LDS behind the fp64 query (at most 48 KiB
//     + 32 KiB: two workgroups per CU).  Per query: zero the bins, barrier, scan the workgroup's slice
//     with LDS atomics, barrier, every thread sweeps the bins and adds the non-zero ones to hist with one
//     device atomic each, barrier before the next query zeroes.
//   * k_range_refine with the count sink (SCREEN tier): the range refine over the screen's survivors,
//     global form (a workgroup scores a few dozen rows of a list: a sweep of the bins never pays).
// Every store is an atomic into a table the host sized: the bin is < bins by the sink's own clamp, the
// row < nq.
#include "vs_range_scan.h"

namespace vs {

// the range kernels with the count sink
template <int DT, int METRIC, bool QLDS, bool SEL, bool LDS>
constexpr auto k_facet_scan = k_range_scan<DT, METRIC, QLDS, SEL, false, RsCountSink<LDS>>;
template <int DT, int METRIC, bool QLDS>
constexpr auto k_facet_refine = k_range_refine<DT, METRIC, QLDS, false, RsCountSink<false>>;

template <int DT, int METRIC, bool QLDS, bool LDS>
static void launch_facet_scan_one(const RangeArgs& a, const FacetArgs& f, int G, int qy, size_t qbytes,
                                  const uint32_t* ids, int64_t m, hipStream_t st) {
    const dim3 grid(G, qy), block(FS_THREADS);
    const size_t lds = qbytes + (LDS ? (size_t)f.bins * sizeof(unsigned) : 0);
    const typename RsCountSink<LDS>::Args sa{f, (int)qbytes};
    if constexpr (LDS) {
        set_lds_attr((const void*)k_facet_scan<DT, METRIC, QLDS, true, true>, (int)(RS_QLDS_MAX + FACET_LDS_BINS * 4));
        set_lds_attr((const void*)k_facet_scan<DT, METRIC, QLDS, false, true>, (int)(RS_QLDS_MAX + FACET_LDS_BINS * 4));
    }
    if (ids) hipLaunchKernelGGL((k_facet_scan<DT, METRIC, QLDS, true, LDS>), grid, block, lds, st, a, ids, m, sa);
    else hipLaunchKernelGGL((k_facet_scan<DT, METRIC, QLDS, false, LDS>), grid, block, lds, st, a, ids, m, sa);
}

template <int DT>
static void launch_facet_scan_dt(const RangeArgs& a, const FacetArgs& f, bool lds, int G, int qy, const uint32_t* ids,
                                 int64_t m, hipStream_t st) {
    const size_t qb = (size_t)((a.d + 7) >> 3) * 64;
    const bool qlds = qb <= RS_QLDS_MAX;
    const size_t qbytes = qlds ? qb : 0;
    const bool ip = a.metric == METRIC_IP;
#define VS_FACET_SCAN(M, Q, L) launch_facet_scan_one<DT, M, Q, L>(a, f, G, qy, qbytes, ids, m, st)
    if (ip && qlds && lds) VS_FACET_SCAN(METRIC_IP, true, true);
    else if (ip && qlds) VS_FACET_SCAN(METRIC_IP, true, false);
    else if (ip && lds) VS_FACET_SCAN(METRIC_IP, false, true);
    else if (ip) VS_FACET_SCAN(METRIC_IP, false, false);
    else if (qlds && lds) VS_FACET_SCAN(METRIC_L2, true, true);
    else if (qlds) VS_FACET_SCAN(METRIC_L2, true, false);
    else if (lds) VS_FACET_SCAN(METRIC_L2, false, true);
    else VS_FACET_SCAN(METRIC_L2, false, false);
#undef VS_FACET_SCAN
}

static bool facet_args_ok(const RangeArgs& a, const FacetArgs& f) {
    return a.corpus && a.q && a.radius && a.nq > 0 && a.d > 0 && a.n_valid > 0 &&
           (a.metric == METRIC_IP || a.metric == METRIC_L2) && a.self_mode == VS_SELF_KEEP && a.row0 == 0 && f.hist &&
           f.bins >= 1 && (f.gid || f.bins == 1) && f.n_cov > 0;
}

hipError_t launch_facet_scan(const RangeArgs& a, const FacetArgs& f, bool lds, int G, int qy, const uint32_t* ids,
                             int64_t m, hipStream_t st) {
    if (!facet_args_ok(a, f) || G < 1 || qy < 1 || qy > a.nq || qy > 65535 || m < 0 || (ids && m == 0) || (!ids && m != 0) ||
        (lds && f.bins > FACET_LDS_BINS))
        return hipErrorInvalidValue;
    if (a.dt == DT_F32) launch_facet_scan_dt<DT_F32>(a, f, lds, G, qy, ids, m, st);
    else if (a.dt == DT_BF16) launch_facet_scan_dt<DT_BF16>(a, f, lds, G, qy, ids, m, st);
    else if (a.dt == DT_F16) launch_facet_scan_dt<DT_F16>(a, f, lds, G, qy, ids, m, st);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

template <int DT>
static void launch_facet_refine_dt(const RangeArgs& a, const FacetArgs& f, const u64* glist, const int* gcnt, int lcap,
                                   int ny, hipStream_t st) {
    const size_t qbytes = (size_t)((a.d + 7) >> 3) * 64;
    const bool qlds = qbytes <= RS_QLDS_MAX;
    const size_t lds = qlds ? qbytes : 0;
    const dim3 grid(a.nq, ny), block(FS_THREADS);
    const bool ip = a.metric == METRIC_IP;
    const RsCountSink<false>::Args sa{f, 0};
#define VS_FACET_REFINE(M, Q) hipLaunchKernelGGL((k_facet_refine<DT, M, Q>), grid, block, lds, st, a, glist, gcnt, lcap, sa)
    if (ip && qlds) VS_FACET_REFINE(METRIC_IP, true);
    else if (ip) VS_FACET_REFINE(METRIC_IP, false);
    else if (qlds) VS_FACET_REFINE(METRIC_L2, true);
    else VS_FACET_REFINE(METRIC_L2, false);
#undef VS_FACET_REFINE
}

hipError_t launch_facet_refine(const RangeArgs& a, const FacetArgs& f, const u64* glist, const int* gcnt, int lcap,
                               int ny, hipStream_t st) {
    if (!facet_args_ok(a, f) || !glist || !gcnt || lcap <= 0 || ny < 1 || ny > 65535) return hipErrorInvalidValue;
    if (a.dt == DT_BF16) launch_facet_refine_dt<DT_BF16>(a, f, glist, gcnt, lcap, ny, st);
    else if (a.dt == DT_F16) launch_facet_refine_dt<DT_F16>(a, f, glist, gcnt, lcap, ny, st);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace vs

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

static bool count_args_ok(const RangeArgs& a, const FacetArgs& f) {
    return a.self_mode == VS_SELF_KEEP && a.row0 == 0 && f.hist && f.bins >= 1 && (f.gid || f.bins == 1) && f.n_cov > 0;
}

hipError_t launch_facet_scan(const RangeArgs& a, const FacetArgs& f, bool lds, int G, int qy, const uint32_t* ids,
                             int64_t m, hipStream_t st) {
    if (!count_args_ok(a, f) || (lds && f.bins > FACET_LDS_BINS)) return hipErrorInvalidValue;
    const int bins_off = (int)rs_query_lds(a.d);
    if (lds)
        return rs_launch_scan<RsCountSink<true>, false>(a, {f, bins_off}, (size_t)f.bins * sizeof(unsigned),
                                                        (int)(RS_QLDS_MAX + FACET_LDS_BINS * 4), G, qy, ids, m, st);
    return rs_launch_scan<RsCountSink<false>, false>(a, {f, bins_off}, 0, 0, G, qy, ids, m, st);
}

hipError_t launch_facet_refine(const RangeArgs& a, const FacetArgs& f, const u64* glist, const int* gcnt, int lcap,
                               int ny, hipStream_t st) {
    if (!count_args_ok(a, f)) return hipErrorInvalidValue;
    return rs_launch_refine<RsCountSink<false>, false>(a, {f, 0}, glist, gcnt, lcap, ny, st);
}

}  // namespace vs

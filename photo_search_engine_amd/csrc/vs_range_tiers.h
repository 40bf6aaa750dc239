// vs_range_tiers.h -- what the jobs built on "which rows pass a radius" share on the host (vs_range_host.hip,
// vs_facet_host.hip, vs_scoresel_host.hip, vs_components_host.hip, vs_dbscan_host.hip; DESIGN §5 "Range search", §7m-§7p):
// the grid rules of the two kernels, the index part of their arguments, the head of the block's small device
// arrays, the readback of the screen's overflow flags and the driver that gives every query of a block to one
// of the two tiers.
//
// One road, and why no sink needs an undo.  The SCREEN tier answers a query from its survivor list, which
// holds every passing row unless a workgroup of the screen had to compact the query's buffer (drop[q] >
// thr0[q]); such a list may be incomplete and the SCAN tier has to answer the query.  The two flags are
// written by range_screen's kernels alone -- launch_pack_qtile zeroes drop, launch_range_thr sets thr0,
// launch_screen_mfma raises drop; the refine reads glist / gcnt only -- so they are read back before the
// refine is launched, and the refine and the scan get complementary masks: a query is answered by exactly
// one tier, every passing row reaches the sink once, and nothing a sink did -- a counter, a histogram row,
// a degree -- is ever taken back, whether or not the sink's operation happens to be idempotent.
//
// range_block (vs_range_host.hip, the pair sink) alone keeps the older order -- refine every query, read the
// flags with the counters in one synchronisation, set the counters of the cut queries back and scan them: it
// has to read its counters after the refine anyway (a query whose pairs outgrew its region is rescanned too),
// so reading the flags first would add a synchronisation per block (profiles/refactor_range_tiers_ab.txt).  It
// uses the grid rules, the argument helper, the aux head and the flag readback below, not range_tiers.
#pragma once
#include "vs_walk.h"

namespace vs {

constexpr int kRangeScanRows = 64;  // rows per workgroup of the scan, at least

// the scan's grid over a sequence of nseq rows and a block of nqb queries: G workgroups split the sequence;
// a short sequence, or few workgroups per CU: qy slices of the grid deal the queries
struct RangeScanGrid {
    int G, qy;
};
inline RangeScanGrid range_scan_grid(int num_cu, int64_t nseq, int nqb) {
    const int64_t ranges = (nseq + kRangeScanRows - 1) / kRangeScanRows;
    const int G = (int)std::max<int64_t>(1, std::min<int64_t>(num_cu, ranges));
    return {G, std::max(1, std::min(nqb, 4 * num_cu / G))};
}

// the refine's workgroups per query (they share the query's list)
inline int range_refine_ny(int num_cu, int nqb) { return std::max(1, std::min(32, 2 * num_cu / nqb)); }

// the index part of a block's arguments; the rest is value-initialised (the plain range search)
inline RangeArgs range_index_args(const vs_index* ix) {
    RangeArgs a{};
    a.corpus = ix->data;
    a.d = ix->d;
    a.dpad = ix->dpad;
    a.dt = ix->dtype;
    a.metric = ix->metric;
    return a;
}

// the head of Ctx::rng_aux and its host mirror: the block's radii (the job uploads them) and the two tiers'
// masks (the driver's)
struct RangeAuxHead {
    float radius[MFMA_QB];
    int go_refine[MFMA_QB];
    int go_scan[MFMA_QB];
};
static_assert(offsetof(RangeAuxHead, go_scan) == offsetof(RangeAuxHead, go_refine) + sizeof(int) * MFMA_QB,
              "the two masks travel in one copy");
inline const float* range_aux_radius(Ctx* c) {
    return (const float*)(c->rng_aux.as<uint8_t>() + offsetof(RangeAuxHead, radius));
}

// the screen's overflow flags of a block, read back: cut(q) = a workgroup compacted query q's buffer and may
// have cut rows above the threshold, so its survivor list may be incomplete
struct RangeCut {
    u64 drop[MFMA_QB], thr[MFMA_QB];
    // (the values are there once the stream is synchronised)
    void read(const ScreenArgs& s, int nqb, hipStream_t st) {
        HIP_CHECK(hipMemcpyAsync(drop, s.drop, sizeof(u64) * nqb, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(thr, s.thr0, sizeof(u64) * nqb, hipMemcpyDeviceToHost, st));
    }
    bool cut(int q) const { return drop[q] > thr[q]; }
};

struct RangeTiers {
    bool screened = false;  // the screen ran (the block's tier is VS_RANGE_SCREEN)
    bool scanned = false;   // the scan was launched
    int rescanned = 0;      // queries the scan answered because their list was cut
};

// One block of nqb device queries through the tiers.  a: the block's arguments, radius at range_aux_radius(c),
// go unset; h: the mirror of the aux head, alive until the caller's next stream synchronisation; ids / m: the
// scan's selector sequence (null / 0: the rows [a.row0, a.n_valid)), nseq its length either way; want[q] != 0:
// query q is to be answered (null: every query); sel and mode decide whether the screen applies.
// refine(a, s, ny) and scan(a, G, qy, ids, m) launch the job's kernels; mid is recorded between the tiers.
template <typename Refine, typename Scan>
RangeTiers range_tiers(vs_index* ix, Ctx* c, RangeArgs a, RangeAuxHead& h, int nqb, const uint32_t* ids, int64_t m,
                       int64_t nseq, const unsigned long long* want, const vs_sel* sel, int mode, hipStream_t st,
                       const DevEvent& mid, Refine&& refine, Scan&& scan) {
    RangeTiers out;
    ScreenArgs s{};
    RangeCut flags;
    out.screened = mode != VS_RANGE_SCAN && range_screen_applies(ix, sel, nqb);
    if (out.screened) {
        s = range_screen(ix, c, a.q, nqb, a.radius, st);
        flags.read(s, nqb, st);
        HIP_CHECK(hipStreamSynchronize(st));
    }
    int nrefine = 0, nscan = 0;
    for (int j = 0; j < nqb; ++j) {
        const bool on = !want || want[j] != 0ull;
        h.go_refine[j] = on && out.screened && !flags.cut(j) ? 1 : 0;
        h.go_scan[j] = on && !h.go_refine[j] ? 1 : 0;
        nrefine += h.go_refine[j];
        nscan += h.go_scan[j];
    }
    if (out.screened) out.rescanned = nscan;
    out.scanned = nscan > 0;
    // (a tier that takes every query of the block needs no mask)
    const bool masked = nrefine != nqb && nscan != nqb;
    uint8_t* ad = c->rng_aux.as<uint8_t>();
    if (masked)
        HIP_CHECK(hipMemcpyAsync(ad + offsetof(RangeAuxHead, go_refine), h.go_refine, 2 * sizeof(h.go_refine),
                                 hipMemcpyHostToDevice, st));
    if (nrefine) {
        a.go = masked ? (const int*)(ad + offsetof(RangeAuxHead, go_refine)) : nullptr;
        refine(a, s, range_refine_ny(ix->num_cu, nqb));
    }
    HIP_CHECK(hipEventRecord(mid, st));
    if (nscan) {
        a.go = masked ? (const int*)(ad + offsetof(RangeAuxHead, go_scan)) : nullptr;
        const RangeScanGrid g = range_scan_grid(ix->num_cu, nseq, nqb);
        scan(a, g.G, g.qy, ids, m);
    }
    return out;
}

}  // namespace vs

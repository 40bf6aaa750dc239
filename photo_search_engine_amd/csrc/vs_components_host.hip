// vs_components_host.hip -- host side of the duplicate groups (include/vs.h "duplicate groups"; kernels:
// vs_components.hip over vs_range_scan.h).
//
// The members, in ascending id, are the queries of a self-join under VS_SELF_ABOVE, staged in blocks of
// MFMA_QB as vs_range_search_rows stages them (gathered on the device from their own rows).  A block runs
// the range search's tiers (range_tiers, vs_range_tiers.h) with the union sink: nothing is appended, sorted
// or shipped per pair; a pair costs one union in parent[] and one count.  What crosses the host per block is
// its edge counters (and the screen's overflow flags); the labels come back once, after the last block.
#include "vs_range_tiers.h"

using namespace vs;

namespace {

struct CcStats {
    int64_t members = 0, edges = 0, components = 0, tier = VS_RANGE_SCAN, rescanned = 0, blocks = 0;
    double ms[3] = {0, 0, 0};
};

void cc_note(vs_index* ix, const CcStats& s) {
    std::lock_guard<std::mutex> g(ix->cc_mu);
    const int64_t st[6] = {s.members, s.edges, s.components, s.tier, s.rescanned, s.blocks};
    std::copy(st, st + 6, ix->cc_stats);
    std::copy(s.ms, s.ms + 3, ix->cc_times);
}

}  // namespace

extern "C" {

int vs_range_components(vs_index* ix, const vs_sel* sel, float radius, int64_t* labels, int64_t* n_components,
                        int64_t* n_edges) {
    return guarded([&] {
        check_index(ix);
        if (std::isnan(radius)) throw VsError(VS_ERR_ARG, "radius is NaN");
        std::shared_lock<std::shared_mutex> lk(ix->rw);
        if (sel) check_sel(ix, sel);
        const int64_t n = ix->ntotal;
        if (n > 0 && !labels) throw VsError(VS_ERR_ARG, "labels is null");
        if (n_components) *n_components = 0;
        if (n_edges) *n_edges = 0;
        CcStats stt;
        const int64_t m = sel ? sel->m : n;  // (a selector covers rows below n only: check_sel)
        if (m == 0) {                        // an empty index, or nothing allowed: no members
            std::fill(labels, labels + n, (int64_t)-1);
            cc_note(ix, stt);
            return;
        }
        stt.members = m;
        DeviceGuard dg(ix->device);
        CtxLease L(ix, nullptr, true);
        Ctx* c = L.c;
        hipStream_t st = c->stream;
        const int mode = ix->range_mode.load();
        const int64_t nblocks = (m + MFMA_QB - 1) / MFMA_QB;
        DevBuf parent, cnt, labels_d;  // (counted in vs_device_bytes_live, freed when the call returns)
        parent.ensure((size_t)n * sizeof(uint32_t));
        cnt.ensure((size_t)nblocks * MFMA_QB * sizeof(unsigned long long));
        labels_d.ensure((size_t)n * sizeof(int64_t));
        HIP_CHECK(launch_cc_init(parent.as<uint32_t>(), n, st));
        HIP_CHECK(hipMemsetAsync(cnt.p, 0, (size_t)nblocks * MFMA_QB * sizeof(unsigned long long), st));
        // the members' ids, ascending: the queries' rows and their self ids
        c->row_ids.ensure((size_t)m * sizeof(int64_t));
        int64_t* mem = c->row_ids.as<int64_t>();
        HIP_CHECK(launch_km_members(sel ? sel->ids : nullptr, m, mem, st));
        c->qdev.ensure((size_t)std::min<int64_t>(m, MFMA_QB) * ix->d * sizeof(float));
        c->rng_aux.ensure(sizeof(RangeAuxHead));
        RangeAuxHead h{};
        std::fill(h.radius, h.radius + MFMA_QB, radius);
        // (h outlives every copy from it: each change of h below follows a stream synchronisation)
        HIP_CHECK(hipMemcpyAsync(c->rng_aux.p, h.radius, sizeof(h.radius), hipMemcpyHostToDevice, st));
        DevEvent e0(hipEventDefault), e1(hipEventDefault), e2(hipEventDefault);
        unsigned long long cnt_h[MFMA_QB];
        for (int64_t q0 = 0; q0 < m; q0 += MFMA_QB) {
            const int nqb = (int)std::min<int64_t>(MFMA_QB, m - q0);
            unsigned long long* cnt_b = cnt.as<unsigned long long>() + stt.blocks * MFMA_QB;  // (zeroed above)
            ++stt.blocks;
            HIP_CHECK(hipEventRecord(e0, st));
            HIP_CHECK(launch_gather_rows(ix->dtype, ix->data, mem + q0, nqb, ix->d, ix->dpad, c->qdev.as<float>(), st));
            RangeArgs a = range_index_args(ix);
            a.n_valid = n;
            a.q = c->qdev.as<float>();
            a.nq = nqb;
            a.radius = range_aux_radius(c);
            a.cnt = cnt_b;
            a.self = mem + q0;
            a.self_mode = VS_SELF_ABOVE;
            // without a selector the members are the rows themselves: the block's smallest id is q0, and no
            // row below it passes for any of its queries
            a.row0 = sel ? 0 : q0;
            // with a selector the scan's sequence is the tail of its ascending list from the block's own first
            // position: the entries before it are below every self id of the block
            const RangeTiers t = range_tiers(
                ix, c, a, h, nqb, sel ? sel->ids + q0 : nullptr, sel ? m - q0 : 0, sel ? m - q0 : n - q0, nullptr, sel,
                mode, st, e1,
                [&](const RangeArgs& r, const ScreenArgs& s, int ny) {
                    HIP_CHECK(launch_cc_refine(r, parent.as<uint32_t>(), s.glist, s.gcnt, s.lcap, ny, st));
                },
                [&](const RangeArgs& r, int G, int qy, const uint32_t* ids, int64_t mseq) {
                    HIP_CHECK(launch_cc_scan(r, parent.as<uint32_t>(), G, qy, ids, mseq, st));
                });
            if (t.screened) stt.tier = VS_RANGE_SCREEN;
            stt.rescanned += t.rescanned;
            HIP_CHECK(hipEventRecord(e2, st));
            HIP_CHECK(hipMemcpyAsync(cnt_h, cnt_b, sizeof(cnt_h[0]) * nqb, hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            stt.ms[0] += ms_between(e0, e1);
            stt.ms[1] += ms_between(e1, e2);
            for (int j = 0; j < nqb; ++j) stt.edges += (int64_t)cnt_h[j];
        }
        // flatten: every member's root, over a -1 fill (rows that are no members)
        HIP_CHECK(hipEventRecord(e0, st));
        HIP_CHECK(hipMemsetAsync(labels_d.p, 0xFF, (size_t)n * sizeof(int64_t), st));
        HIP_CHECK(launch_cc_labels(parent.as<uint32_t>(), sel ? sel->ids : nullptr, m, n, labels_d.as<int64_t>(), st));
        HIP_CHECK(hipMemcpyAsync(labels, labels_d.p, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipEventRecord(e1, st));
        HIP_CHECK(hipStreamSynchronize(st));
        stt.ms[2] = ms_between(e0, e1);
        for (int64_t i = 0; i < n; ++i) stt.components += labels[i] == i ? 1 : 0;
        if (n_components) *n_components = stt.components;
        if (n_edges) *n_edges = stt.edges;
        cc_note(ix, stt);
    });
}

int vs_components_last_stats(vs_index* ix, int64_t* out, int cap) {
    return guarded([&] {
        check_index(ix);
        copy_last(ix->cc_mu, ix->cc_stats, 6, out, cap, "stats");
    });
}

int vs_components_last_times(vs_index* ix, double* out, int cap) {
    return guarded([&] {
        check_index(ix);
        copy_last(ix->cc_mu, ix->cc_times, 3, out, cap, "times");
    });
}

}  // extern "C"

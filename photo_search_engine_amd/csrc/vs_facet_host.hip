// vs_facet_host.hip -- host side of the facet counts (include/vs.h "facet counts"; kernels: vs_facet.hip
// over vs_range_scan.h).
//
// Queries are staged in blocks as the range search stages them; a block's answers are one table of
// nqb x bins 64-bit counters on the device, zeroed before the block, read back after it and widened into
// the caller's counts / totals.  The SCREEN tier is the range search's (range_screen, then the refine with
// the count sink); a query whose survivor list a workgroup had to cut gets its row of the table zeroed and
// is re-answered by the scan, so no query is counted from an incomplete list and no row twice.
#include "vs_walk.h"

using namespace vs;

namespace {

constexpr int kFacetScanRows = 64;  // rows per workgroup of the scan, at least (the range scan's figure)

std::atomic<int64_t> g_facet_staging{64ll << 20};  // vs_set_facet_staging_bytes

// the block's small device arrays and their host mirror
struct FacetAuxH {
    float radius[MFMA_QB];
    int go[MFMA_QB];
};

struct FacetStats {
    int64_t total = 0, tier = VS_RANGE_SCAN, rescanned = 0, form = 0, blocks = 0;
    double ms[3] = {0, 0, 0};
};

void facet_note(vs_index* ix, const FacetStats& s) {
    std::lock_guard<std::mutex> g(ix->facet_mu);
    const int64_t st[5] = {s.total, s.tier, s.rescanned, s.form, s.blocks};
    std::copy(st, st + 5, ix->facet_stats);
    std::copy(s.ms, s.ms + 3, ix->facet_times);
}

// AUTO: the LDS form when the bins fit and the workgroup's share of the rows outweighs the sweep of the
// bins that ends every query: a thread reads bins / FS_THREADS of them, a wave scores
// rows / FS_NW rows, so while bins <= 128 rows the sweep stays at or below two LDS reads per row a wave
// scores.  Short sequences (a small selector) over many groups take the global form.
bool facet_lds_form(int form, int64_t bins, int64_t rows_per_wg) {
    if (form == VS_FACET_HIST_LDS) return true;
    if (form == VS_FACET_HIST_GLOBAL) return false;
    return bins <= FACET_LDS_BINS && bins <= 128 * rows_per_wg;
}

}  // namespace

extern "C" {

int vs_range_count(vs_index* ix, const vs_groups* gr, const vs_sel* sel, const float* q, int64_t nq, const float* radius,
                   int64_t* counts, int64_t* totals) {
    return guarded([&] {
        check_index(ix);
        if (nq < 0) throw VsError(VS_ERR_ARG, "nq must be >= 0");
        std::shared_lock<std::shared_mutex> lk(ix->rw);
        if (gr) check_groups(ix, gr);
        if (sel) check_sel(ix, sel);
        if (gr && !counts) throw VsError(VS_ERR_ARG, "counts is null (with groups it is the output)");
        if (!gr && counts) throw VsError(VS_ERR_ARG, "counts without groups (totals is the output)");
        if (!counts && !totals) throw VsError(VS_ERR_ARG, "both outputs are null");
        const int64_t bins = gr ? gr->G + 1 : 1;
        const int form = ix->facet_hist.load();
        if (form == VS_FACET_HIST_LDS && bins > FACET_LDS_BINS)
            throw VsError(VS_ERR_ARG, "the LDS histogram holds " + std::to_string(FACET_LDS_BINS) + " bins, G + 1 is " +
                                          std::to_string(bins));
        FacetStats stt;
        if (nq == 0) {
            facet_note(ix, stt);
            return;
        }
        if (!q || !radius) throw VsError(VS_ERR_ARG, "null host buffer");
        check_radii(radius, nq);
        if (counts) std::fill(counts, counts + nq * bins, (int64_t)0);
        if (totals) std::fill(totals, totals + nq, (int64_t)0);
        const int64_t n_cov = gr ? gr->n_cov : ix->ntotal;
        if (n_cov == 0 || (sel && sel->m == 0)) {  // no members
            facet_note(ix, stt);
            return;
        }
        DeviceGuard dg(ix->device);
        CtxLease L(ix, nullptr, true);
        Ctx* c = L.c;
        hipStream_t st = c->stream;
        const int mode = ix->range_mode.load();
        const int64_t row_bytes = 8 * bins;
        const int qb = (int)std::max<int64_t>(1, std::min<int64_t>(MFMA_QB, g_facet_staging.load() / row_bytes));
        DevBuf table;  // (freed when the call returns)
        table.ensure((size_t)std::min<int64_t>(qb, nq) * row_bytes);
        std::vector<unsigned long long> table_h((size_t)std::min<int64_t>(qb, nq) * bins);
        c->rng_aux.ensure(sizeof(FacetAuxH));
        uint8_t* ad = c->rng_aux.as<uint8_t>();
        FacetAuxH h{};
        DevEvent e0(hipEventDefault), e1(hipEventDefault), e2(hipEventDefault), e3(hipEventDefault);
        // the sequence the scan's workgroups split, as range_block sizes it
        const int64_t nseq = sel ? sel->m : n_cov;
        const int64_t ranges = (nseq + kFacetScanRows - 1) / kFacetScanRows;
        const int G = (int)std::max<int64_t>(1, std::min<int64_t>(ix->num_cu, ranges));
        const bool lds = facet_lds_form(form, bins, (nseq + G - 1) / G);
        for (int64_t q0 = 0; q0 < nq; q0 += qb) {
            const int nqb = (int)std::min<int64_t>(qb, nq - q0);
            ++stt.blocks;
            // (the previous block synchronised the stream after its copies from hq and h)
            stage_queries(ix, c, q, q0, nqb, st);
            for (int j = 0; j < nqb; ++j) {
                h.radius[j] = radius[q0 + j];
                h.go[j] = 1;
            }
            HIP_CHECK(hipMemcpyAsync(ad, &h, sizeof(h), hipMemcpyHostToDevice, st));
            HIP_CHECK(hipMemsetAsync(table.p, 0, (size_t)nqb * row_bytes, st));
            RangeArgs a{};
            a.corpus = ix->data;
            a.d = ix->d;
            a.dpad = ix->dpad;
            a.dt = ix->dtype;
            a.metric = ix->metric;
            a.n_valid = n_cov;  // (rows behind the groups are no members: not scanned, not refined)
            a.q = c->qdev.as<float>();
            a.nq = nqb;
            a.radius = (const float*)(ad + offsetof(FacetAuxH, radius));
            a.go = (const int*)(ad + offsetof(FacetAuxH, go));
            a.self_mode = VS_SELF_KEEP;
            FacetArgs f{};
            f.gid = gr ? gr->gid.as<int32_t>() : nullptr;
            f.n_cov = n_cov;
            f.bins = (int)bins;
            f.hist = table.as<unsigned long long>();
            bool scan = true;
            HIP_CHECK(hipEventRecord(e0, st));
            if (mode != VS_RANGE_SCAN && range_screen_applies(ix, sel, nqb)) {
                const ScreenArgs s = range_screen(ix, c, a.q, nqb, a.radius, st);
                RangeArgs r = a;
                r.go = nullptr;
                const int ny = std::max(1, std::min(32, 2 * ix->num_cu / nqb));
                HIP_CHECK(launch_facet_refine(r, f, s.glist, s.gcnt, s.lcap, ny, st));
                std::vector<u64> drop_h((size_t)nqb), thr_h((size_t)nqb);
                HIP_CHECK(hipMemcpyAsync(drop_h.data(), s.drop, sizeof(u64) * nqb, hipMemcpyDeviceToHost, st));
                HIP_CHECK(hipMemcpyAsync(thr_h.data(), s.thr0, sizeof(u64) * nqb, hipMemcpyDeviceToHost, st));
                HIP_CHECK(hipStreamSynchronize(st));
                // a workgroup compacted the query's buffer and may have cut rows above the threshold: the
                // list may be incomplete, so the row starts again from zero and the scan answers it
                scan = false;
                for (int j = 0; j < nqb; ++j) {
                    h.go[j] = drop_h[j] > thr_h[j] ? 1 : 0;
                    if (h.go[j]) {
                        scan = true;
                        ++stt.rescanned;
                        HIP_CHECK(hipMemsetAsync((uint8_t*)table.p + (size_t)j * row_bytes, 0, (size_t)row_bytes, st));
                    }
                }
                if (scan) HIP_CHECK(hipMemcpyAsync(ad, &h, sizeof(h), hipMemcpyHostToDevice, st));
                stt.tier = VS_RANGE_SCREEN;
            }
            HIP_CHECK(hipEventRecord(e1, st));
            if (scan) {
                // a short sequence, or few workgroups per CU: deal the queries over slices of the grid
                const int qy = std::max(1, std::min(nqb, 4 * ix->num_cu / G));
                HIP_CHECK(launch_facet_scan(a, f, lds, G, qy, sel ? sel->ids : nullptr, sel ? sel->m : 0, st));
                stt.form = lds ? VS_FACET_HIST_LDS : VS_FACET_HIST_GLOBAL;
            }
            HIP_CHECK(hipEventRecord(e2, st));
            HIP_CHECK(hipMemcpyAsync(table_h.data(), table.p, (size_t)nqb * row_bytes, hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipEventRecord(e3, st));
            HIP_CHECK(hipStreamSynchronize(st));
            stt.ms[0] += ms_between(e0, e1);
            stt.ms[1] += ms_between(e1, e2);
            stt.ms[2] += ms_between(e2, e3);
            for (int j = 0; j < nqb; ++j) {
                const unsigned long long* row = table_h.data() + (size_t)j * bins;
                int64_t sum = 0;
                for (int64_t b = 0; b < bins; ++b) sum += (int64_t)row[b];
                if (counts) std::copy(row, row + bins, counts + (q0 + j) * bins);
                if (totals) totals[q0 + j] = sum;
                stt.total += sum;
            }
        }
        facet_note(ix, stt);
    });
}

int vs_set_facet_hist(vs_index* ix, int form) {
    return guarded([&] {
        check_index(ix);
        if (form != VS_FACET_HIST_AUTO && form != VS_FACET_HIST_LDS && form != VS_FACET_HIST_GLOBAL)
            throw VsError(VS_ERR_ARG, "facet histogram form must be VS_FACET_HIST_AUTO, _LDS or _GLOBAL");
        ix->facet_hist.store(form);
    });
}

int vs_set_facet_staging_bytes(int64_t bytes) {
    return guarded([&] {
        if (bytes < 1) throw VsError(VS_ERR_ARG, "facet staging bytes must be >= 1");
        g_facet_staging.store(bytes);
    });
}

int vs_facet_last_stats(vs_index* ix, int64_t* out, int cap) {
    return guarded([&] {
        check_index(ix);
        copy_last(ix->facet_mu, ix->facet_stats, 5, out, cap, "stats");
    });
}

int vs_facet_last_times(vs_index* ix, double* out, int cap) {
    return guarded([&] {
        check_index(ix);
        copy_last(ix->facet_mu, ix->facet_times, 3, out, cap, "times");
    });
}

}  // extern "C"

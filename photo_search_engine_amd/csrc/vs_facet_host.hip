// vs_facet_host.hip -- host side of the facet counts (include/vs.h "facet counts"; kernels: vs_facet.hip
// over vs_range_scan.h).
//
// Queries are staged in blocks as the range search stages them; a block's answers are one table of
// nqb x bins 64-bit counters on the device, zeroed before the block, read back after it and widened into
// the caller's counts / totals.  The tiers are the range search's (range_tiers, vs_range_tiers.h) with the
// count sink.
#include "vs_range_tiers.h"

using namespace vs;

namespace {

std::atomic<int64_t> g_facet_staging{64ll << 20};  // vs_set_facet_staging_bytes

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
        c->rng_aux.ensure(sizeof(RangeAuxHead));
        RangeAuxHead h{};
        DevEvent e0(hipEventDefault), e1(hipEventDefault), e2(hipEventDefault), e3(hipEventDefault);
        // the sequence the scan's workgroups split
        const int64_t nseq = sel ? sel->m : n_cov;
        const int G = range_scan_grid(ix->num_cu, nseq, 1).G;
        const bool lds = facet_lds_form(form, bins, (nseq + G - 1) / G);
        for (int64_t q0 = 0; q0 < nq; q0 += qb) {
            const int nqb = (int)std::min<int64_t>(qb, nq - q0);
            ++stt.blocks;
            // (the previous block synchronised the stream after its copies from hq and h)
            stage_queries(ix, c, q, q0, nqb, st);
            std::copy(radius + q0, radius + q0 + nqb, h.radius);
            HIP_CHECK(hipMemcpyAsync(c->rng_aux.p, h.radius, sizeof(h.radius), hipMemcpyHostToDevice, st));
            HIP_CHECK(hipMemsetAsync(table.p, 0, (size_t)nqb * row_bytes, st));
            RangeArgs a = range_index_args(ix);
            a.n_valid = n_cov;  // (rows behind the groups are no members: not scanned, not refined)
            a.q = c->qdev.as<float>();
            a.nq = nqb;
            a.radius = range_aux_radius(c);
            FacetArgs f{};
            f.gid = gr ? gr->gid.as<int32_t>() : nullptr;
            f.n_cov = n_cov;
            f.bins = (int)bins;
            f.hist = table.as<unsigned long long>();
            HIP_CHECK(hipEventRecord(e0, st));
            const RangeTiers t = range_tiers(
                ix, c, a, h, nqb, sel ? sel->ids : nullptr, sel ? sel->m : 0, nseq, nullptr, sel, mode, st, e1,
                [&](const RangeArgs& r, const ScreenArgs& s, int ny) {
                    HIP_CHECK(launch_facet_refine(r, f, s.glist, s.gcnt, s.lcap, ny, st));
                },
                [&](const RangeArgs& r, int g, int qy, const uint32_t* ids, int64_t m) {
                    HIP_CHECK(launch_facet_scan(r, f, lds, g, qy, ids, m, st));
                });
            if (t.screened) stt.tier = VS_RANGE_SCREEN;
            stt.rescanned += t.rescanned;
            if (t.scanned) stt.form = lds ? VS_FACET_HIST_LDS : VS_FACET_HIST_GLOBAL;
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

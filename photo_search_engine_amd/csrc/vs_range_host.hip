// vs_range_host.hip -- host side of range search (include/vs.h "range search"; kernels: vs_range.hip).
#include "vs_range_tiers.h"

using namespace vs;

namespace {

// the block's small device arrays and their host mirror (one upload of the leading part per launch)
struct RangeAuxH {
    RangeAuxHead head;
    unsigned long long cnt[MFMA_QB];
    int64_t off[MFMA_QB];
    int64_t cap[MFMA_QB];
    RangeSeg seg[MFMA_QB];
};
static_assert(sizeof(RangeSeg) == 32 && offsetof(RangeAuxH, head) == 0 && offsetof(RangeAuxH, cnt) == 3072 &&
                  offsetof(RangeAuxH, seg) == 9216,
              "RangeAuxH layout");

constexpr int64_t kRangePairBytes = 32ll << 20;  // first-pass pair buffer of one block (12 B per pair)

}  // namespace

namespace vs {

bool range_screen_applies(const vs_index* ix, const vs_sel* sel, int nqb) {
    return !sel && (ix->dtype == DT_BF16 || ix->dtype == DT_F16) && nqb > GEMV_NQ_MAX && nqb <= MFMA_QB;
}

// (declared in vs_index.h)  the native MFMA screen of the stored rows as search_block launches it unseeded
// at depth MFMA_KP_MAX (the int8 screen setting does not apply), started at the radius' key
ScreenArgs range_screen(vs_index* ix, Ctx* c, const float* qd, int nqb, const float* radius_d, hipStream_t st) {
    ScreenArgs s = mfma_screen_base(ix, false);
    c->qinfo.ensure(sizeof(float) * 2 * MFMA_QB);
    c->qtile.ensure((size_t)MFMA_QB * ix->dpad * ix->es);
    c->thr0.ensure(sizeof(u64) * MFMA_QB);
    mfma_workspace(c, s);
    s.part = s.glist;
    HIP_CHECK(launch_pack_qtile(ix->dtype, qd, nqb, ix->d, ix->dpad, c->qtile.as<uint8_t>(), c->qinfo.as<float>(),
                                c->gcnt.as<int>(), c->drop.as<u64>(), st));
    HIP_CHECK(launch_range_thr(ix->metric, radius_d, c->qinfo.as<float>(), qd, ix->d, nqb, xmax_of(ix), gamma_of(ix->d),
                               c->thr0.as<u64>(), st));
    s.thr0 = c->thr0.as<u64>();
    HIP_CHECK(launch_screen_mfma(ix->dtype, s, c->qtile.as<uint8_t>(), nqb, st));
    return s;
}

// (declared in vs_index.h)  self: the block's queries are stored rows (vs_rows_host.hip); the kernels
// reject the rows it excludes before they are counted, so everything below sees the filtered answer
void range_block(vs_index* ix, Ctx* c, const vs_sel* sel, const float* qd, int nqb, const float* rad, bool screen,
                 bool count_only, hipStream_t st, RangeStats& stt, int64_t* counts, vs_range_result* res,
                 const RangeSelf& self) {
    // (VS_SELF_ABOVE without a selector: no row below row0 can pass, the scan skips them)
    const int64_t row0 = sel ? 0 : self.row0;
    const int64_t nseq = sel ? sel->m : ix->ntotal - row0;
    // every query of the block gets an equal region of the first-pass buffer (all of its rows when
    // they fit); a query that finds more is rerun into a region of the size it counted
    const int64_t capq = count_only ? 0 : std::min<int64_t>(nseq, std::max<int64_t>(1, kRangePairBytes / (12 * nqb)));
    RangeAuxH h{};
    c->rng_aux.ensure(sizeof(RangeAuxH));
    uint8_t* ad = c->rng_aux.as<uint8_t>();
    c->rng_p[0].ensure((size_t)std::max<int64_t>(1, capq * nqb) * 12);
    for (int q = 0; q < nqb; ++q) {
        h.head.radius[q] = rad[q];
        h.cnt[q] = 0;
        h.off[q] = (int64_t)q * capq;
        h.cap[q] = capq;
    }
    // (h outlives every copy from it: each change of h below follows a stream synchronisation)
    HIP_CHECK(hipMemcpyAsync(ad, &h, offsetof(RangeAuxH, seg), hipMemcpyHostToDevice, st));
    RangeArgs a = range_index_args(ix);
    a.n_valid = ix->ntotal;
    a.q = qd;
    a.nq = nqb;
    a.radius = range_aux_radius(c);
    a.cnt = (unsigned long long*)(ad + offsetof(RangeAuxH, cnt));
    a.off = (const int64_t*)(ad + offsetof(RangeAuxH, off));
    a.cap = (const int64_t*)(ad + offsetof(RangeAuxH, cap));
    a.psc = c->rng_p[0].as<double>();
    a.pid = (uint32_t*)(a.psc + capq * nqb);
    a.self = self.ids;
    a.self_mode = self.mode;
    a.row0 = row0;
    auto read_counts = [&] {
        HIP_CHECK(hipMemcpyAsync(h.cnt, a.cnt, sizeof(h.cnt[0]) * nqb, hipMemcpyDeviceToHost, st));
    };
    // The pair sink has a second reason to give a query to the scan, known only after the refine: its passing
    // rows outgrew its region.  Its counters have to be read after the refine in any case, so the block does not
    // take range_tiers (which would put a second synchronisation before the refine): every query is refined, the
    // flags come back with the counters, and the scan answers the cut and the outgrown queries from a counter
    // set back to zero -- the pair sink's own redo, its region is simply written again.
    std::vector<char> need((size_t)nqb, 1);
    int64_t total2 = 0;  // pairs of the second buffer (reruns)
    if (screen) {
        RangeCut flags;
        const ScreenArgs s = range_screen(ix, c, qd, nqb, a.radius, st);
        HIP_CHECK(launch_range_refine(a, s.glist, s.gcnt, s.lcap, range_refine_ny(ix->num_cu, nqb), st));
        read_counts();
        flags.read(s, nqb, st);
        HIP_CHECK(hipStreamSynchronize(st));
        for (int q = 0; q < nqb; ++q) {
            need[q] = (flags.cut(q) || (!count_only && (int64_t)h.cnt[q] > capq)) ? 1 : 0;
            stt.rescanned += need[q];
        }
        stt.tier = VS_RANGE_SCREEN;
    }
    if (std::any_of(need.begin(), need.end(), [](char v) { return v != 0; })) {
        for (int q = 0; q < nqb; ++q) {
            h.head.go_scan[q] = need[q];
            if (need[q]) h.cnt[q] = 0;
        }
        HIP_CHECK(hipMemcpyAsync(ad + offsetof(RangeAuxHead, go_scan), h.head.go_scan,
                                 offsetof(RangeAuxH, off) - offsetof(RangeAuxHead, go_scan), hipMemcpyHostToDevice, st));
        a.go = (const int*)(ad + offsetof(RangeAuxHead, go_scan));
        const RangeScanGrid g = range_scan_grid(ix->num_cu, nseq, nqb);
        const uint32_t* ids = sel ? sel->ids : nullptr;
        const int64_t m = sel ? sel->m : 0;
        HIP_CHECK(launch_range_scan(a, g.G, g.qy, ids, m, st));
        read_counts();
        HIP_CHECK(hipStreamSynchronize(st));
        std::vector<int> over;
        if (!count_only)
            for (int q = 0; q < nqb; ++q)
                if (need[q] && (int64_t)h.cnt[q] > capq) over.push_back(q);
        if (!over.empty()) {
            std::vector<int64_t> want((size_t)nqb, 0);
            for (int q = 0; q < nqb; ++q) h.head.go_scan[q] = 0;
            for (int q : over) {
                want[q] = (int64_t)h.cnt[q];
                h.head.go_scan[q] = 1;
                h.cnt[q] = 0;
                h.off[q] = total2;
                h.cap[q] = want[q];
                total2 += want[q];
                need[q] = 2;  // (its pairs are in the second buffer)
            }
            c->rng_p[1].ensure((size_t)total2 * 12);
            HIP_CHECK(hipMemcpyAsync(ad, &h, offsetof(RangeAuxH, seg), hipMemcpyHostToDevice, st));
            RangeArgs a2 = a;
            a2.psc = c->rng_p[1].as<double>();
            a2.pid = (uint32_t*)(a2.psc + total2);
            HIP_CHECK(launch_range_scan(a2, g.G, g.qy, ids, m, st));
            read_counts();
            HIP_CHECK(hipStreamSynchronize(st));
            for (int q : over)
                if ((int64_t)h.cnt[q] != want[q]) throw VsError(VS_ERR_INTERNAL, "range scan: a rerun counted differently");
        }
    }
    int64_t total = 0;
    for (int q = 0; q < nqb; ++q) {
        counts[q] = (int64_t)h.cnt[q];
        total += counts[q];
    }
    if (count_only || total == 0) return;
    for (int q = 0; q < nqb; ++q) {
        h.seg[q].src = need[q] == 2 ? h.off[q] : (int64_t)q * capq;
        h.seg[q].n = counts[q];
        h.seg[q].dst = q == 0 ? 0 : h.seg[q - 1].dst + h.seg[q - 1].n;
        h.seg[q].buf = need[q] == 2 ? 1 : 0;
        h.seg[q].pad = 0;
    }
    HIP_CHECK(hipMemcpyAsync(ad + offsetof(RangeAuxH, seg), h.seg, sizeof(RangeSeg) * nqb, hipMemcpyHostToDevice, st));
    c->rng_D.ensure((size_t)total * sizeof(float));
    c->rng_I.ensure((size_t)total * sizeof(int64_t));
    c->rng_S.ensure((size_t)total * sizeof(double));
    RangeEmitArgs e{};
    e.psc[0] = c->rng_p[0].as<double>();
    e.pid[0] = (const uint32_t*)(e.psc[0] + capq * nqb);
    e.psc[1] = c->rng_p[1].as<double>();
    e.pid[1] = total2 ? (const uint32_t*)(e.psc[1] + total2) : nullptr;
    e.seg = (const RangeSeg*)(ad + offsetof(RangeAuxH, seg));
    e.metric = ix->metric;
    e.id_offset = 0;
    e.D = c->rng_D.as<float>();
    e.I = c->rng_I.as<int64_t>();
    e.S = c->rng_S.as<double>();
    HIP_CHECK(launch_range_emit(e, nqb, st));
    const size_t base = res->D.size();
    res->D.resize(base + (size_t)total);
    res->I.resize(base + (size_t)total);
    res->S.resize(base + (size_t)total);
    HIP_CHECK(hipMemcpyAsync(res->D.data() + base, e.D, (size_t)total * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(res->I.data() + base, e.I, (size_t)total * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(res->S.data() + base, e.S, (size_t)total * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    // segments past the LDS sort come as they were appended: the same order on the host
    const bool ip = ix->metric == METRIC_IP;
    for (int q = 0; q < nqb; ++q) {
        const int64_t n = counts[q];
        if (n <= RS_SORT_MAX) continue;
        ++stt.host_sorted;
        const size_t o = base + (size_t)h.seg[q].dst;
        std::vector<int64_t> perm((size_t)n);
        for (int64_t j = 0; j < n; ++j) perm[j] = j;
        const double* S = res->S.data() + o;
        const int64_t* I = res->I.data() + o;
        std::sort(perm.begin(), perm.end(), [&](int64_t x, int64_t y) {
            if (S[x] != S[y]) return ip ? S[x] > S[y] : S[x] < S[y];
            return I[x] < I[y];
        });
        std::vector<double> s2((size_t)n);
        std::vector<int64_t> i2((size_t)n);
        for (int64_t j = 0; j < n; ++j) {
            s2[j] = S[perm[j]];
            i2[j] = I[perm[j]];
        }
        for (int64_t j = 0; j < n; ++j) {
            res->S[o + j] = s2[j];
            res->I[o + j] = i2[j];
            res->D[o + j] = (float)s2[j];
        }
    }
}

void range_note_stats(vs_index* ix, const RangeStats& s) {
    std::lock_guard<std::mutex> g(ix->range_mu);
    ix->range_stats[0] = s.total;
    ix->range_stats[1] = s.tier;
    ix->range_stats[2] = s.rescanned;
    ix->range_stats[3] = s.host_sorted;
}


}  // namespace vs

void vs::range_search_host(vs_index* ix, const vs_sel* sel, const float* q, int64_t nq, const float* radius,
                           int64_t max_total, vs_range_result* out) {
    check_index(ix);
    if (nq < 0) throw VsError(VS_ERR_ARG, "nq must be >= 0");
    std::shared_lock<std::shared_mutex> lk(ix->rw);
    if (sel) check_sel(ix, sel);
    out->lims.assign((size_t)nq + 1, 0);
    out->D.clear();
    out->I.clear();
    out->S.clear();
    RangeStats stt;
    if (nq == 0) {
        range_note_stats(ix, stt);
        return;
    }
    if (!q || !radius) throw VsError(VS_ERR_ARG, "null host buffer");
    check_radii(radius, nq);
    if (ix->ntotal == 0 || (sel && sel->m == 0)) {  // nothing to return
        range_note_stats(ix, stt);
        return;
    }
    DeviceGuard dg(ix->device);
    CtxLease L(ix, nullptr, true);
    Ctx* c = L.c;
    hipStream_t st = c->stream;
    // AUTO: the screen where it applies, otherwise the scan.  (vs_set_scan_limit's rule -- one or two
    // queries over a small index take the scan alone -- names blocks the screen never serves.)
    const int mode = ix->range_mode.load();
    int64_t counts[MFMA_QB];
    int64_t total = 0;
    for (int64_t q0 = 0; q0 < nq; q0 += MFMA_QB) {
        const int nqb = (int)std::min<int64_t>(MFMA_QB, nq - q0);
        // (the previous block synchronised the stream after its copy from hq)
        stage_queries(ix, c, q, q0, nqb, st);
        const bool screen = mode != VS_RANGE_SCAN && range_screen_applies(ix, sel, nqb);
        // past the cap only the count is wanted (the error names it)
        const bool count_only = max_total > 0 && total > max_total;
        range_block(ix, c, sel, c->qdev.as<float>(), nqb, radius + q0, screen, count_only, st, stt, counts, out);
        for (int j = 0; j < nqb; ++j) out->lims[(size_t)(q0 + j + 1)] = out->lims[(size_t)(q0 + j)] + counts[j];
        total = out->lims[(size_t)(q0 + nqb)];
    }
    stt.total = total;
    range_note_stats(ix, stt);
    if (max_total > 0 && total > max_total)
        throw VsError(VS_ERR_ARG, "range search found " + std::to_string(total) + " results, max_total is " +
                                      std::to_string(max_total));
}

extern "C" {

int vs_range_search(vs_index* ix, const vs_sel* sel, const float* q, int64_t nq, const float* radius,
                    int64_t max_total, vs_range_result** out) {
    return guarded([&] {
        if (!out) throw VsError(VS_ERR_ARG, "out is null");
        std::unique_ptr<vs_range_result> r(new vs_range_result());
        range_search_host(ix, sel, q, nq, radius, max_total, r.get());
        std::vector<double>().swap(r->S);  // (the fp64 scores serve the multi-device merge only)
        *out = r.release();
    });
}

const int64_t* vs_range_lims(const vs_range_result* r) { return r ? r->lims.data() : nullptr; }
const float* vs_range_D(const vs_range_result* r) { return r ? r->D.data() : nullptr; }
const int64_t* vs_range_I(const vs_range_result* r) { return r ? r->I.data() : nullptr; }
int64_t vs_range_nq(const vs_range_result* r) { return r ? (int64_t)r->lims.size() - 1 : -1; }
void vs_range_free(vs_range_result* r) { delete r; }

int vs_set_range_mode(vs_index* ix, int mode) {
    return guarded([&] {
        check_index(ix);
        if (mode != VS_RANGE_AUTO && mode != VS_RANGE_SCAN && mode != VS_RANGE_SCREEN)
            throw VsError(VS_ERR_ARG, "range mode must be VS_RANGE_AUTO, VS_RANGE_SCAN or VS_RANGE_SCREEN");
        ix->range_mode.store(mode);
    });
}

int vs_range_last_stats(vs_index* ix, int64_t* out, int cap) {
    return guarded([&] {
        check_index(ix);
        copy_last(ix->range_mu, ix->range_stats, 4, out, cap, "stats");
    });
}

}  // extern "C"

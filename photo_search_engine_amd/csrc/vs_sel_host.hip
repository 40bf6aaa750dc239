// vs_sel_host.hip -- host side of the id selectors: exact filtered search (include/vs.h "id
// selectors"; kernels: vs_selscan.hip).
#include "vs_index.h"

using namespace vs;

namespace {

// allowed rows of [0, n_sel) counted on the host, masked as k_sel_compact masks (sel_word)
int64_t sel_host_count(const uint8_t* bitmap, int64_t n_sel) {
    int64_t m = 0;
    const int64_t full = n_sel >> 3;
    for (int64_t i = 0; i < full; ++i) m += __builtin_popcount(bitmap[i]);
    if (n_sel & 7) m += __builtin_popcount(bitmap[full] & ((1u << (n_sel & 7)) - 1u));
    return m;
}


}  // namespace

namespace vs {

void check_sel(const vs_index* ix, const vs_sel* sel) {
    if (!sel) throw VsError(VS_ERR_ARG, "null selector");
    if (sel->ix != ix) throw VsError(VS_ERR_ARG, "selector belongs to another index");
    if (sel->gen != ix->reset_gen.load() || sel->n_sel > ix->ntotal)
        throw VsError(VS_ERR_ARG, "stale selector (the index was reset after it was made)");
}


}  // namespace vs

namespace {

// The tier of one filtered call.  The scan gathers nq * m rows; the overfetch tier runs the exact
// unfiltered search (about one pass over the ntotal stored rows per query block, plus a k'-deep
// refine) and filters its lists.  kSelScanFactor is the nq * m / ntotal up to which AUTO scans: at
// 1 the scan's bytes equal one pass over the stored rows.  Measured (scripts/sel_scan_timing.py,
// profiles/sel_scan_timing.jsonl; 256 queries, k = 10, d = 1536): at nq * m / ntotal = 2.5 the scan
// takes 0.50 ms against the overfetch tier's 2.6 ms on 100k fp32 rows (crossover near 6) and 8.6 ms
// against 7.4 ms on 1M bf16 rows (crossover near 2.2); at 26 the overfetch tier wins 4x and 23x.
// 3 sits between the two crossovers.  DESIGN §5 "Filtered search".
constexpr double kSelScanFactor = 3.0;

}  // namespace

namespace vs {

SelPlan sel_plan(const vs_index* ix, const vs_sel* sel, int64_t nq, int k) {
    const int mode = ix->sel_mode.load();
    // (k > ntotal: a shard of a multi-device index with fewer rows than k; the scan pads)
    if (sel->m == 0 || mode == VS_SEL_SCAN || k > ix->ntotal) return {VS_SEL_SCAN, 0};
    const double want = std::ceil(1.5 * (double)k * (double)ix->ntotal / (double)sel->m) + 32.0;
    const int64_t raw = want >= 1e15 ? (int64_t)1e15 : round_up((int64_t)want, 16);
    // (k <= k': ntotal >= m, k <= ntotal here and the callers keep k <= K_MAX)
    const int kp = (int)std::min<int64_t>(std::min<int64_t>(K_MAX, ix->ntotal), raw);
    if (mode == VS_SEL_OVERFETCH) return {VS_SEL_OVERFETCH, kp};
    if (nq <= 2 || (double)nq * (double)sel->m <= kSelScanFactor * (double)ix->ntotal || raw > K_MAX)
        return {VS_SEL_SCAN, 0};
    return {VS_SEL_OVERFETCH, kp};
}

}  // namespace vs

namespace {

// k_sel_scan over one query block: full_scan_block's sizing with the list length in place of the
// row count (rows_per_wg, the scratch budget, <= CUs and <= FS_B workgroups).  Counted nowhere:
// vs_full_scan_count / vs_uncertified_count speak of the unfiltered screens.
constexpr int kSelScanRows = 64;  // list positions per workgroup, at least
void sel_scan_block(vs_index* ix, Ctx* c, const vs_sel* sel, const float* q, int nqb, int k, const SearchOut& out,
                    hipStream_t st, bool all_queries) {
    const FullScanArgs a = full_scan_args(ix, c, sel->m, kSelScanRows, std::min(ix->num_cu, FS_B), q, nqb, k,
                                          out, all_queries, st);
    // a short list leaves CUs idle: deal the block's queries over as many slices as fill them
    const int qy = std::max(1, std::min(nqb, ix->num_cu / a.G));
    HIP_CHECK(launch_sel_scan(a, sel->ids, sel->m, qy, st));
}

}  // namespace

namespace vs {

// One batch of device queries through the planned tier; outputs device [nq][k].  Returns the
// queries the overfetch tier left short and the scan re-answered.  Synchronises st on that tier.
int64_t sel_search_ctx(vs_index* ix, Ctx* c, const vs_sel* sel, const SelPlan& plan, const float* q, int64_t nq, int k,
                       const SearchOut& out, hipStream_t st) {
    c->selaux.ensure((size_t)nq * 3 * sizeof(int));
    int* cert_u = c->selaux.as<int>();  // the unfiltered search's certificates
    int* found = cert_u + nq;
    int* proven = found + nq;           // the scan's cert: 0 = to be (re-)answered by it
    auto scan_blocks = [&](bool all, const int* proven_h) {
        for (int64_t q0 = 0; q0 < nq; q0 += MFMA_QB) {
            const int nqb = (int)std::min<int64_t>(MFMA_QB, nq - q0);
            if (!all && std::all_of(proven_h + q0, proven_h + q0 + nqb, [](int v) { return v != 0; })) continue;
            SearchOut ob = out.at(q0, k);
            ob.cert = proven + q0;
            sel_scan_block(ix, c, sel, q + q0 * ix->d, nqb, k, ob, st, all);
        }
    };
    if (plan.tier == VS_SEL_SCAN) {
        scan_blocks(true, nullptr);
        return 0;
    }
    // the exact unfiltered top-k' (every screen and fallback of the device-exact path, then the
    // gated full scan), its allowed entries in order, and per query how many there were
    const int kp = plan.kp;
    c->selD.ensure((size_t)nq * kp * sizeof(float));
    c->selI.ensure((size_t)nq * kp * sizeof(int64_t));
    if (out.S64) c->selS.ensure((size_t)nq * kp * sizeof(double));
    const SearchOut wide{c->selD.as<float>(), c->selI.as<int64_t>(), out.S64 ? c->selS.as<double>() : nullptr, cert_u};
    search_all(ix, c, q, nq, kp, screen_depth(kp), wide, st, kOptimisticSeedRank, true);
    SelTakeArgs t{};
    t.bits = sel->bits;
    t.n_sel = sel->n_sel;
    t.I_in = c->selI.as<int64_t>();
    t.D_in = c->selD.as<float>();
    t.S_in = wide.S64;
    t.kp = kp;
    t.k = k;
    t.metric = ix->metric;
    t.D = out.D;
    t.I = out.I;
    t.S64 = out.S64;
    t.cert_in = cert_u;
    t.found = found;
    t.cert_out = proven;
    t.exhaustive = kp >= ix->ntotal ? 1 : 0;
    HIP_CHECK(launch_sel_take(t, (int)nq, st));
    // as vs_search reads certificates back: the queries whose prefix is not proven go to the scan
    std::vector<int> proven_h((size_t)nq);
    HIP_CHECK(hipMemcpyAsync(proven_h.data(), proven, (size_t)nq * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    const int64_t redo = std::count(proven_h.begin(), proven_h.end(), 0);
    if (redo) scan_blocks(false, proven_h.data());
    return redo;
}

void sel_note_stats(vs_index* ix, const vs_sel* sel, const SelPlan& plan, int64_t redo) {
    std::lock_guard<std::mutex> g(ix->sel_mu);
    ix->sel_stats[0] = sel->m;
    ix->sel_stats[1] = plan.tier;
    ix->sel_stats[2] = plan.kp;
    ix->sel_stats[3] = redo;
}


}  // namespace vs

void vs::search_sel_device(vs_index* ix, const vs_sel* sel, const float* q_dev, int64_t nq, int k, float* D_dev,
                           int64_t* I_dev, double* S64_dev, hipStream_t st) {
    check_index(ix);
    if (nq <= 0) return;
    std::shared_lock<std::shared_mutex> lk(ix->rw);
    DeviceGuard dg(ix->device);
    check_sel(ix, sel);
    if (k <= 0) throw VsError(VS_ERR_ARG, "k must be > 0");
    if (ix->ntotal == 0 || k > K_MAX) throw VsError(VS_ERR_ARG, "empty index or k too large");
    if (nq > 0x7FFFFFFF / 3) throw VsError(VS_ERR_ARG, "too many queries in one call");
    CtxLease L(ix, st, false);
    const SelPlan plan = sel_plan(ix, sel, nq, k);
    const int64_t redo = sel_search_ctx(ix, L.c, sel, plan, q_dev, nq, k, SearchOut{D_dev, I_dev, S64_dev}, st);
    sel_note_stats(ix, sel, plan, redo);
}

extern "C" {

int vs_sel_create(vs_index* ix, const uint8_t* bitmap, int64_t nbytes, vs_sel** out) {
    return guarded([&] {
        if (!out) throw VsError(VS_ERR_ARG, "out is null");
        *out = nullptr;
        check_index(ix);
        std::shared_lock<std::shared_mutex> lk(ix->rw);
        DeviceGuard dg(ix->device);
        const int64_t n = ix->ntotal;
        const int64_t need = (n + 7) / 8;
        if (nbytes < need || (need > 0 && !bitmap))
            throw VsError(VS_ERR_ARG, "selector bitmap too short: " + std::to_string(need) + " bytes cover ntotal");
        if (n >= 0xFFFFFFFFll) throw VsError(VS_ERR_ARG, "selector ids are 32-bit");
        std::unique_ptr<vs_sel, void (*)(vs_sel*)> sel(new vs_sel(), vs_sel_destroy);
        sel->ix = ix;
        sel->gen = ix->reset_gen.load();
        sel->device = ix->device;
        sel->n_sel = n;
        if (n > 0) {
            DevBuf tmp;  // per-workgroup counts, then the device's total (8-byte aligned)
            sel->m = sel_host_count(bitmap, n);
            const int64_t nwords = (n + 63) / 64;
            const int64_t groups = sel_compact_groups(n);
            HIP_CHECK(hipMalloc((void**)&sel->bits, (size_t)nwords * 8));
            HIP_CHECK(hipMalloc((void**)&sel->ids, (size_t)std::max<int64_t>(sel->m, 1) * sizeof(uint32_t)));
            const size_t cnt_off = (size_t)round_up(groups * (int64_t)sizeof(unsigned), 8);
            tmp.ensure(cnt_off + 8);
            CtxLease L(ix, nullptr, true);
            hipStream_t st = L.c->stream;
            HIP_CHECK(hipMemsetAsync(sel->bits, 0, (size_t)nwords * 8, st));
            HIP_CHECK(hipMemcpyAsync(sel->bits, bitmap, (size_t)need, hipMemcpyHostToDevice, st));
            unsigned long long* cnt_d = (unsigned long long*)((uint8_t*)tmp.p + cnt_off);
            HIP_CHECK(launch_sel_compact(sel->bits, n, tmp.as<unsigned>(), sel->ids, sel->m, cnt_d, st));
            unsigned long long cnt_h = 0;
            HIP_CHECK(hipMemcpyAsync(&cnt_h, cnt_d, sizeof(cnt_h), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            if ((int64_t)cnt_h != sel->m) throw VsError(VS_ERR_INTERNAL, "selector compaction count mismatch");
        }
        *out = sel.release();
    });
}

void vs_sel_destroy(vs_sel* sel) {
    if (!sel) return;
    int prev = -1;
    (void)hipGetDevice(&prev);
    if (prev != sel->device) (void)hipSetDevice(sel->device);
    if (sel->bits) (void)hipFree(sel->bits);
    if (sel->ids) (void)hipFree(sel->ids);
    if (prev >= 0 && prev != sel->device) (void)hipSetDevice(prev);
    delete sel;
}

int64_t vs_sel_count(const vs_sel* sel) { return sel ? sel->m : -1; }

int vs_set_sel_mode(vs_index* ix, int mode) {
    return guarded([&] {
        check_index(ix);
        if (mode != VS_SEL_AUTO && mode != VS_SEL_SCAN && mode != VS_SEL_OVERFETCH)
            throw VsError(VS_ERR_ARG, "selector mode must be VS_SEL_AUTO, VS_SEL_SCAN or VS_SEL_OVERFETCH");
        ix->sel_mode.store(mode);
    });
}

int vs_sel_last_stats(vs_index* ix, int64_t* out, int cap) {
    return guarded([&] {
        check_index(ix);
        copy_last(ix->sel_mu, ix->sel_stats, 4, out, cap, "stats");
    });
}

int vs_search_sel(vs_index* ix, const vs_sel* sel, const float* q, int64_t nq, int32_t k, float* D, int64_t* I) {
    return guarded([&] {
        check_index(ix);
        if (nq < 0) throw VsError(VS_ERR_ARG, "nq must be >= 0");
        if (k <= 0) throw VsError(VS_ERR_ARG, "k must be > 0");
        std::shared_lock<std::shared_mutex> lk(ix->rw);
        check_sel(ix, sel);
        if (nq == 0) return;
        if (!q || !D || !I) throw VsError(VS_ERR_ARG, "null host buffer");
        DeviceGuard dg(ix->device);
        const float fillD = worst_score(ix);
        // k beyond the rows present: search min(k, ntotal), pad the rest (as vs_search)
        const int kk = (int)std::min<int64_t>(k, ix->ntotal);
        check_k(kk);
        const SelPlan plan = sel_plan(ix, sel, nq, std::max(kk, 1));
        if (ix->ntotal == 0 || sel->m == 0) {  // nothing allowed: all padding
            fill_padding(D, I, nq * k, fillD);
            sel_note_stats(ix, sel, plan, 0);
            return;
        }
        CtxLease L(ix, nullptr, true);
        Ctx* c = L.c;
        hipStream_t st = c->stream;
        // pinned staging in chunks of queries, as vs_search (device and host blocks [I int64 | D fp32])
        const int64_t chunk = stage_chunk(ix, nq, kk, false);
        int64_t redo = 0;
        for (int64_t q0 = 0; q0 < nq; q0 += chunk) {
            const int64_t m = std::min(chunk, nq - q0);
            stage_queries(ix, c, q, q0, m, st);
            const StagedOut so = exact_lists(ix, c, sel, plan, m, kk, LISTS_HOST, st);
            redo += so.redo;
            scatter_padded(so, q0, m, k, kk, fillD, D, I);
        }
        sel_note_stats(ix, sel, plan, redo);
    });
}

}  // extern "C"

// vs_after_host.hip -- host side of the paged search (include/vs.h "paged search"; kernels: vs_after.hip;
// DESIGN §7l): validation, the cursor scoring, the two tiers and their stats.
//   LISTS  exact top-L lists among the members (exact_lists, deepened by deepen_lists of vs_walk.h), cut at
//          the cursor by k_after_cut; complete iff k entries lie behind the cursor or the list held every
//          member.
//   SCAN   the streaming scan over the members with the rows at or before the cursor passed over and
//          counted: queries whose hint puts the page beyond the limit (AUTO), and what the lists left open.
#include "vs_walk.h"

using namespace vs;

namespace {

enum { T_SCORE = 4, T_SCAN = 5 };  // slots of WalkTimes::ms behind the two list tiers'
constexpr int kAfterScanRows = 64;  // list positions (rows) per scan workgroup, at least

// a cut's block for m queries of k entries, on the device and copied to the host:
// [I int64 mk | rank int64 m | D fp32 mk | complete int32 m]
struct AfBlock {
    int64_t *I, *rank;
    float* D;
    int32_t* complete;
    size_t bytes;
};
AfBlock af_block(const void* base, size_t m, size_t mk) {
    Carver c(base);
    AfBlock b{c.take<int64_t>(mk), c.take<int64_t>(m), c.take<float>(mk), c.take<int32_t>(m)};
    b.bytes = c.used;
    return b;
}

// one call's state: the scratch (freed with it, before the call returns) and where the answers go
struct AfCall {
    vs_index* ix;
    Ctx* c;
    hipStream_t st;
    int k;
    float* D;
    int64_t* I;
    int64_t* rank;  // (may be null)
    int64_t members;
    std::vector<int32_t> complete;
    DevBuf qall, after_d, key_d, out_d, qmap_d, scanq, scanI, scanD, scanR, cert;
    std::vector<uint8_t> h;
    std::vector<int64_t> qmap_h;

    AfterCursor cursor(const int64_t* qmap) const { return AfterCursor{after_d.as<int64_t>(), key_d.as<double>(), qmap}; }

    // every query's cursor row scored: q / after -> the device copies and key_d
    void score(const float* q, const int64_t* after, int64_t nq) {
        qall.ensure((size_t)nq * ix->d * sizeof(float));
        after_d.ensure((size_t)nq * sizeof(int64_t));
        key_d.ensure((size_t)nq * sizeof(double));
        HIP_CHECK(hipMemcpyAsync(qall.p, q, (size_t)nq * ix->d * sizeof(float), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync(after_d.p, after, (size_t)nq * sizeof(int64_t), hipMemcpyHostToDevice, st));
        HIP_CHECK(launch_after_score(ix->dtype, ix->metric, ix->data, ix->d, ix->dpad, ix->ntotal, qall.as<float>(),
                                     after_d.as<int64_t>(), nq, key_d.as<double>(), st));
    }

    // the cut of m staged queries (device, [m][d] at qd) with lists Il / Dl [m][L]; staged query j is the
    // call's query qof[idx[j]] and its answer goes there
    void cut(const float* qd, const int64_t* Il, const float* Dl, int64_t L, int64_t m, const int64_t* idx,
             const std::vector<int64_t>& qof, DevEvent* ev_done) {
        const size_t mk = (size_t)m * k;
        const size_t bytes = af_block(nullptr, m, mk).bytes;
        out_d.ensure(bytes);
        const AfBlock dev = af_block(out_d.p, m, mk);
        qmap_h.resize((size_t)m);
        for (int64_t j = 0; j < m; ++j) qmap_h[(size_t)j] = qof[(size_t)idx[j]];
        qmap_d.ensure((size_t)m * sizeof(int64_t));
        HIP_CHECK(hipMemcpyAsync(qmap_d.p, qmap_h.data(), (size_t)m * sizeof(int64_t), hipMemcpyHostToDevice, st));
        AfterCutArgs a{};
        a.corpus = ix->data;
        a.d = ix->d;
        a.dpad = ix->dpad;
        a.dt = ix->dtype;
        a.metric = ix->metric;
        a.n_valid = ix->ntotal;
        a.L = L;
        a.k = k;
        const int64_t qmax = 65536;  // workgroups of one launch
        for (int64_t q0 = 0; q0 < m; q0 += qmax) {
            const int nq = (int)std::min(qmax, m - q0);
            a.q = qd + q0 * ix->d;
            a.I_list = Il + q0 * L;
            a.D_list = Dl + q0 * L;
            a.cur = cursor(qmap_d.as<int64_t>() + q0);
            a.I = dev.I + q0 * k;
            a.D = dev.D + q0 * k;
            a.rank = dev.rank + q0;
            a.complete = dev.complete + q0;
            HIP_CHECK(launch_after_cut(a, nq, st));
        }
        if (ev_done) HIP_CHECK(hipEventRecord(*ev_done, st));
        h.resize(bytes);
        HIP_CHECK(hipMemcpyAsync(h.data(), out_d.p, bytes, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        const AfBlock w = af_block(h.data(), m, mk);
        for (int64_t j = 0; j < m; ++j) {
            const int64_t r = qmap_h[(size_t)j];
            const bool done = w.complete[j] != 0 || L >= members;  // (a list of every member is complete)
            complete[(size_t)r] = done ? 1 : 0;
            if (!done) continue;  // (a deeper list or the scan answers it)
            std::copy(w.I + j * k, w.I + (j + 1) * k, I + r * k);
            std::copy(w.D + j * k, w.D + (j + 1) * k, D + r * k);
            if (rank) rank[r] = w.rank[j];
        }
    }

    // the scan of the call's queries qs[0, np) at depth ks <= k: over the listed rows (ids, n_ids) or over
    // every row; their answers and ranks to the host outputs
    void scan(const float* q, const std::vector<int64_t>& qs, int ks, const uint32_t* ids, int64_t n_ids, float fillD) {
        const int64_t np = (int64_t)qs.size();
        std::vector<float> qsub((size_t)np * ix->d);
        for (int64_t j = 0; j < np; ++j)
            std::copy(q + qs[(size_t)j] * ix->d, q + (qs[(size_t)j] + 1) * ix->d, qsub.begin() + j * ix->d);
        scanq.ensure(qsub.size() * sizeof(float));
        qmap_d.ensure((size_t)np * sizeof(int64_t));
        scanI.ensure((size_t)np * ks * sizeof(int64_t));
        scanD.ensure((size_t)np * ks * sizeof(float));
        scanR.ensure((size_t)np * sizeof(unsigned long long));
        cert.ensure((size_t)np * sizeof(int));
        HIP_CHECK(hipMemcpyAsync(scanq.p, qsub.data(), qsub.size() * sizeof(float), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync(qmap_d.p, qs.data(), (size_t)np * sizeof(int64_t), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemsetAsync(scanR.p, 0, (size_t)np * sizeof(unsigned long long), st));
        for (int64_t q0 = 0; q0 < np; q0 += MFMA_QB) {
            const int nqb = (int)std::min<int64_t>(MFMA_QB, np - q0);
            const SearchOut out{scanD.as<float>() + q0 * ks, scanI.as<int64_t>() + q0 * ks, nullptr, cert.as<int>() + q0};
            const FullScanArgs a = full_scan_args(ix, c, ids ? n_ids : ix->ntotal, kAfterScanRows,
                                                  std::min(ix->num_cu, FS_B), scanq.as<float>() + q0 * ix->d, nqb, ks,
                                                  out, true, st);
            // a short list leaves CUs idle: deal the block's queries over as many slices as fill them
            const int qy = ids ? std::max(1, std::min(nqb, ix->num_cu / a.G)) : 1;
            HIP_CHECK(launch_after_scan(a, cursor(qmap_d.as<int64_t>() + q0), scanR.as<unsigned long long>() + q0, ids, n_ids,
                                        qy, st));
        }
        std::vector<int64_t> hI((size_t)np * ks);
        std::vector<float> hD((size_t)np * ks);
        std::vector<unsigned long long> hR((size_t)np);
        HIP_CHECK(hipMemcpyAsync(hI.data(), scanI.p, hI.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(hD.data(), scanD.p, hD.size() * sizeof(float), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(hR.data(), scanR.p, hR.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        for (int64_t j = 0; j < np; ++j) {
            const int64_t r = qs[(size_t)j];
            fill_padding(D + r * k, I + r * k, k, fillD);
            std::copy(hI.begin() + j * ks, hI.begin() + (j + 1) * ks, I + r * k);
            std::copy(hD.begin() + j * ks, hD.begin() + (j + 1) * ks, D + r * k);
            if (rank) rank[r] = (int64_t)hR[(size_t)j];
        }
    }
};

}  // namespace

extern "C" {

int vs_search_after(vs_index* ix, const vs_sel* sel, const float* q, int64_t nq, int32_t k, const int64_t* after,
                    const int64_t* rank_hint, float* D, int64_t* I, int64_t* rank) {
    return guarded([&] {
        check_index(ix);
        if (nq < 0) throw VsError(VS_ERR_ARG, "nq must be >= 0");
        if (k < 1 || k > K_MAX) throw VsError(VS_ERR_ARG, "k must be in 1.." + std::to_string(K_MAX));
        std::shared_lock<std::shared_mutex> lk(ix->rw);
        if (sel) check_sel(ix, sel);
        if (ix->d > AF_D_MAX) throw VsError(VS_ERR_ARG, "paged search: d must be <= " + std::to_string(AF_D_MAX));
        const WalkState::Depth depth = ix->af.resolve(std::max(4 * k, 64), K_MAX);
        const int64_t limit = depth.limit;
        const int mode = ix->after_mode.load();
        const int tier = mode == VS_AFTER_SCAN ? VS_AFTER_SCAN : VS_AFTER_LISTS;
        int64_t stats[6] = {nq, 0, 0, 0, 0, tier};
        WalkTimes times;
        auto note = [&] { ix->af.note(stats, 6, times.ms, 8); };
        if (nq == 0) {
            note();
            return;
        }
        if (!q || !after || !D || !I) throw VsError(VS_ERR_ARG, "null host buffer");
        for (int64_t i = 0; i < nq; ++i)
            if (after[i] < -1 || after[i] >= ix->ntotal)
                throw VsError(VS_ERR_ARG, "after must be -1 or a stored row's id (query " + std::to_string(i) + ")");
        const float fillD = worst_score(ix);
        fill_padding(D, I, nq * k, fillD);
        if (rank) std::fill(rank, rank + nq, (int64_t)0);
        const int64_t members = sel ? sel->m : ix->ntotal;
        if (members == 0) {  // nothing to rank: all padding, rank 0
            stats[1] = nq;
            note();
            return;
        }
        DeviceGuard dg(ix->device);
        CtxLease lease(ix, nullptr, true);
        Ctx* c = lease.c;
        hipStream_t st = c->stream;
        AfCall call{ix, c, st, k, D, I, rank, members, std::vector<int32_t>((size_t)nq, 0)};
        DevEvent e0(hipEventDefault), e1(hipEventDefault);
        HIP_CHECK(hipEventRecord(e0, st));
        call.score(q, after, nq);
        HIP_CHECK(hipEventRecord(e1, st));
        HIP_CHECK(hipStreamSynchronize(st));
        times.ms[T_SCORE] += ms_between(e0, e1);
        // ---- who takes which road: a hinted page beyond the limit goes straight to the scan (AUTO) ----
        std::vector<int64_t> lq, sq;  // the call's queries for the lists / for the scan, ascending
        int64_t first = depth.first;
        for (int64_t i = 0; i < nq; ++i) {
            const int64_t hint = rank_hint ? rank_hint[i] : -1;
            const bool beyond = hint >= 0 && hint > limit - k;  // hint + k > limit
            if (mode == VS_AFTER_SCAN || (mode == VS_AFTER_AUTO && beyond)) {
                sq.push_back(i);
                continue;
            }
            lq.push_back(i);
            if (hint >= 0 && !beyond) first = std::max(first, hint + k);
        }
        // ---- exact top-L lists of the members, cut at the cursor; not complete goes deeper -------------
        if (!lq.empty()) {
            const int64_t nl = (int64_t)lq.size();
            std::vector<float> qsub;
            const float* ql = q;
            if (nl != nq) {
                qsub.resize((size_t)nl * ix->d);
                for (int64_t j = 0; j < nl; ++j)
                    std::copy(q + lq[(size_t)j] * ix->d, q + (lq[(size_t)j] + 1) * ix->d, qsub.begin() + j * ix->d);
                ql = qsub.data();
            }
            Deepened dl = deepen_lists(
                ix, c, st, sel, members, first, limit, ql, nl, times,
                [&](const StagedOut& so, int64_t L, int64_t m, const int64_t* idx, DevEvent* ev) {
                    call.cut(c->qdev.as<float>(), so.Id, so.Dd, L, m, idx, lq, ev);
                },
                [&](int64_t r) { return call.complete[(size_t)lq[(size_t)r]] != 0; });
            stats[1] = dl.done[0];
            stats[2] = dl.done[1];
            stats[4] = dl.longest;
            for (int64_t r : dl.pending) sq.push_back(lq[(size_t)r]);
            std::sort(sq.begin(), sq.end());
        }
        // ---- SCAN: the members behind the cursor streamed through the running top-k --------------------
        if (!sq.empty()) {
            const int ks = (int)std::min<int64_t>(k, members);
            HIP_CHECK(hipEventRecord(e0, st));
            if (sel) call.scan(q, sq, ks, sel->ids, sel->m, fillD);
            else call.scan(q, sq, ks, nullptr, 0, fillD);
            HIP_CHECK(hipEventRecord(e1, st));
            HIP_CHECK(hipStreamSynchronize(st));
            times.ms[T_SCAN] += ms_between(e0, e1);
            stats[3] = (int64_t)sq.size();
        }
        note();
    });
}

int vs_set_after_mode(vs_index* ix, int tier) {
    return guarded([&] {
        check_index(ix);
        if (tier != VS_AFTER_AUTO && tier != VS_AFTER_LISTS && tier != VS_AFTER_SCAN)
            throw VsError(VS_ERR_ARG, "after tier must be VS_AFTER_AUTO, _LISTS or _SCAN");
        ix->after_mode.store(tier);
    });
}

int vs_set_after_depth(vs_index* ix, int32_t first, int32_t limit) {
    return guarded([&] {
        check_index(ix);
        ix->af.set(first, limit, K_MAX, "after");
    });
}

int vs_after_last_stats(vs_index* ix, int64_t* out, int cap) {
    return guarded([&] {
        check_index(ix);
        copy_last(ix->af.mu, ix->af.stats, 6, out, cap, "stats");
    });
}

int vs_after_last_times(vs_index* ix, double* out, int cap) {
    return guarded([&] {
        check_index(ix);
        copy_last(ix->af.mu, ix->af.times, 6, out, cap, "times");
    });
}

}  // extern "C"

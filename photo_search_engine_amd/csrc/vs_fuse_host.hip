// vs_fuse_host.hip -- host side of the fused search (include/vs.h "fused search"; kernels: vs_fuse.hip;
// DESIGN §7k): the argument checks, the tiers and their stats.
//
//   LISTS  the exact top-L lists of the nq m sub-queries (exact_lists through deepen_lists of vs_walk.h,
//          a fused query's m sub-queries always in one staged chunk), walked by k_fuse_walk: every
//          distinct candidate rescored against all m sub-queries and ranked by (F, id).  ANY is complete
//          at L = min(k, members); ALL deepens until the walk's certificate holds.
//   SCAN   k_fuse_scan over every member, then the walk over its k rows for which and D_sub.
#include "vs_walk.h"

using namespace vs;

namespace {

enum { T_SCAN = 4, T_SCAN_WALK = 5 };         // slots of WalkTimes::ms behind the two list tiers'
constexpr int kFuseScanRows = 64;             // list positions (rows) per scan workgroup, at least
constexpr size_t kFuseWalkScratch = 64u << 20;  // the walk's score scratch per launch, about

int64_t fuse_k_limit(int m) { return std::min<int64_t>(K_MAX, FUSE_WALK_MAX / m); }

// a walk's block for n fused queries of k entries, on the device and copied to the host:
// [I int64 nk | D fp32 nk | D_sub fp32 nk m | which int32 nk | complete int32 n]
struct FuBlock {
    int64_t* I;
    float *D, *U;
    int32_t *which, *complete;
    size_t bytes;
};
FuBlock fu_block(const void* base, size_t n, size_t nk, int m) {
    Carver c(base);
    FuBlock b{c.take<int64_t>(nk), c.take<float>(nk), c.take<float>(nk * m), c.take<int32_t>(nk), c.take<int32_t>(n)};
    b.bytes = c.used;
    return b;
}

// one call's state: the scratch (freed with it, before the call returns) and where the answers go
struct FuCall {
    vs_index* ix;
    Ctx* c;
    hipStream_t st;
    int m, mode, k;
    float* D;
    int64_t* I;
    int32_t* which;  // (may be null)
    float* D_sub;    // (may be null)
    std::vector<int32_t> complete;
    DevBuf out_d, stmp, etmp, scanI, cert, qall;
    std::vector<uint8_t> h;

    // the walk over n fused queries (device, [n][m][d] at qd) and their lists Il [n][nl][L]; answers into
    // rows idx[j] of the outputs
    void walk(const float* qd, const int64_t* Il, int nl, int64_t L, bool certify, int64_t n, const int64_t* idx,
              DevEvent* ev_done) {
        const size_t nk = (size_t)n * k;
        const size_t bytes = fu_block(nullptr, n, nk, m).bytes;
        out_d.ensure(bytes);
        const FuBlock dev = fu_block(out_d.p, n, nk, m);
        const int64_t n_ent = nl * L;
        // the scratch rows of one launch: as many fused queries at a time as kFuseWalkScratch holds
        const int64_t qmax = std::max<int64_t>(1, std::min<int64_t>(65535, kFuseWalkScratch / (n_ent * m * sizeof(double))));
        const int64_t qn = std::min(qmax, n);
        stmp.ensure((size_t)qn * n_ent * m * sizeof(double));
        etmp.ensure((size_t)qn * n_ent * sizeof(uint32_t));
        FuseWalkArgs a{};
        a.corpus = ix->data;
        a.d = ix->d;
        a.dpad = ix->dpad;
        a.dt = ix->dtype;
        a.metric = ix->metric;
        a.n_valid = ix->ntotal;
        a.m = m;
        a.mode = mode;
        a.nl = nl;
        a.L = L;
        a.certify = certify ? 1 : 0;
        a.k = k;
        a.S_tmp = stmp.as<double>();
        a.E_tmp = etmp.as<uint32_t>();
        for (int64_t q0 = 0; q0 < n; q0 += qn) {  // (stream order: a launch's scratch is free for the next)
            const int nq = (int)std::min(qn, n - q0);
            a.q = qd + q0 * m * ix->d;
            a.I_list = Il + q0 * n_ent;
            a.I = dev.I + q0 * k;
            a.D = dev.D + q0 * k;
            a.which = dev.which + q0 * k;
            a.D_sub = dev.U + q0 * k * m;
            a.complete = dev.complete + q0;
            HIP_CHECK(launch_fuse_walk(a, nq, st));
        }
        if (ev_done) HIP_CHECK(hipEventRecord(*ev_done, st));
        h.resize(bytes);
        HIP_CHECK(hipMemcpyAsync(h.data(), out_d.p, bytes, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        const FuBlock w = fu_block(h.data(), n, nk, m);
        for (int64_t j = 0; j < n; ++j) {
            const int64_t r = idx[j];
            std::copy(w.I + j * k, w.I + (j + 1) * k, I + r * k);
            std::copy(w.D + j * k, w.D + (j + 1) * k, D + r * k);
            if (which) std::copy(w.which + j * k, w.which + (j + 1) * k, which + r * k);
            if (D_sub) std::copy(w.U + j * k * m, w.U + (j + 1) * k * m, D_sub + r * k * m);
            complete[(size_t)r] = w.complete[j];
        }
    }

    // the fused scan of n device fused queries at depth ks into scanI [n][ks]: over the listed rows (ids,
    // n_ids) or over every row
    void scan(const float* qd, int64_t n, int ks, const uint32_t* ids, int64_t n_ids) {
        scanI.ensure((size_t)n * ks * sizeof(int64_t));
        cert.ensure((size_t)n * sizeof(int));
        for (int64_t q0 = 0; q0 < n; q0 += MFMA_QB) {
            const int nqb = (int)std::min<int64_t>(MFMA_QB, n - q0);
            const SearchOut out{nullptr, scanI.as<int64_t>() + q0 * ks, nullptr, cert.as<int>() + q0};
            const FullScanArgs a = full_scan_args(ix, c, ids ? n_ids : ix->ntotal, kFuseScanRows,
                                                  std::min(ix->num_cu, FS_B), qd + q0 * m * ix->d, nqb, ks, out,
                                                  true, st);
            // fewer workgroups than CUs (a short list, or deep lists under the scratch budget): deal the block's
            // queries over as many slices as fill them
            const int qy = std::max(1, std::min(nqb, ix->num_cu / a.G));
            HIP_CHECK(launch_fuse_scan(a, m, mode, ids, n_ids, qy, st));
        }
    }
};

}  // namespace

extern "C" {

int vs_search_fused(vs_index* ix, const vs_sel* sel, const float* q, int64_t nq, int32_t m, int32_t mode, int32_t k,
                    float* D, int64_t* I, int32_t* which, float* D_sub) {
    return guarded([&] {
        check_index(ix);
        if (nq < 0) throw VsError(VS_ERR_ARG, "nq must be >= 0");
        if (m < 1 || m > VS_FUSE_MAX_Q)
            throw VsError(VS_ERR_ARG, "fused search: m must be in 1.." + std::to_string(VS_FUSE_MAX_Q));
        if (mode != VS_FUSE_ANY && mode != VS_FUSE_ALL) throw VsError(VS_ERR_ARG, "fuse mode must be VS_FUSE_ANY or VS_FUSE_ALL");
        const int64_t klim = fuse_k_limit(m);
        if (k < 1 || k > klim)
            throw VsError(VS_ERR_ARG, "fused search: k must be in 1.." + std::to_string(klim) + " at m = " + std::to_string(m));
        std::shared_lock<std::shared_mutex> lk(ix->rw);
        if (sel) check_sel(ix, sel);
        // (the depth settings: cut to this call's own limit)
        const int set_first = ix->fu.first.load(), set_limit = ix->fu.limit.load();
        const int64_t limit = set_limit > 0 ? std::min<int64_t>(set_limit, klim) : klim;
        const int64_t first = std::min<int64_t>(set_first > 0 ? set_first : std::max(4 * k, 64), limit);
        const int tier = ix->fuse_mode.load() == VS_FUSE_SCAN ? VS_FUSE_SCAN : VS_FUSE_LISTS;
        int64_t stats[6] = {nq, 0, 0, 0, 0, tier};
        WalkTimes times;
        auto note = [&] { ix->fu.note(stats, 6, times.ms, 8); };
        if (nq == 0) {
            note();
            return;
        }
        if (!q || !D || !I) throw VsError(VS_ERR_ARG, "null host buffer");
        const float fillD = worst_score(ix);
        fill_padding(D, I, nq * k, fillD);
        if (which) std::fill(which, which + nq * k, -1);
        if (D_sub) std::fill(D_sub, D_sub + nq * k * m, fillD);
        const int64_t members = sel ? sel->m : ix->ntotal;
        if (members == 0) {  // nothing to rank: all padding
            stats[1] = nq;
            note();
            return;
        }
        // (the longest walk: ANY's one list of k, ALL's deepest; the scan's walk has k entries)
        const int64_t deepest = tier == VS_FUSE_SCAN ? k : m * (mode == VS_FUSE_ANY ? (int64_t)k : std::max<int64_t>(limit, k));
        if (fuse_walk_lds(std::min<int64_t>(deepest, FUSE_WALK_MAX), ix->d) > FUSE_DYN_CAP)
            throw VsError(VS_ERR_ARG, "fused search: d too large for this depth limit (vs_set_fuse_depth)");
        DeviceGuard dg(ix->device);
        CtxLease lease(ix, nullptr, true);
        Ctx* c = lease.c;
        hipStream_t st = c->stream;
        FuCall call{ix, c, st, m, mode, k, D, I, which, D_sub, std::vector<int32_t>((size_t)nq, 0)};
        std::vector<int64_t> pending;
        if (tier == VS_FUSE_SCAN) {
            pending.resize((size_t)nq);
            for (int64_t i = 0; i < nq; ++i) pending[(size_t)i] = i;
        } else {
            // ---- exact top-L lists of every sub-query, walked on the device; not complete goes deeper ----
            const bool any = mode == VS_FUSE_ANY;
            Deepened dl = deepen_lists(
                ix, c, st, sel, members, any ? k : first, any ? k : limit, q, nq, times,
                [&](const StagedOut& so, int64_t L, int64_t n, const int64_t* idx, DevEvent* ev) {
                    call.walk(c->qdev.as<float>(), so.Id, m, L, !any, n, idx, ev);
                },
                [&](int64_t r) { return call.complete[(size_t)r] != 0; }, m);
            stats[1] = dl.done[0];
            stats[2] = dl.done[1];
            stats[4] = dl.longest;
            pending.swap(dl.pending);
            if (any && !pending.empty()) throw VsError(VS_ERR_INTERNAL, "fused search: ANY's list of k did not complete");
        }
        // ---- SCAN: the fused scan over every member, then the walk over its rows -------------------------
        if (!pending.empty()) {
            const int64_t np = (int64_t)pending.size(), qd = (int64_t)m * ix->d;
            const int ks = (int)std::min<int64_t>(k, members);
            std::vector<float> qsub((size_t)np * qd);
            for (int64_t j = 0; j < np; ++j)
                std::copy(q + pending[(size_t)j] * qd, q + (pending[(size_t)j] + 1) * qd, qsub.begin() + j * qd);
            call.qall.ensure(qsub.size() * sizeof(float));
            DevEvent e0(hipEventDefault), e1(hipEventDefault), e2(hipEventDefault);
            HIP_CHECK(hipEventRecord(e0, st));
            HIP_CHECK(hipMemcpyAsync(call.qall.p, qsub.data(), qsub.size() * sizeof(float), hipMemcpyHostToDevice, st));
            if (sel) call.scan(call.qall.as<float>(), np, ks, sel->ids, sel->m);
            else call.scan(call.qall.as<float>(), np, ks, nullptr, 0);
            HIP_CHECK(hipEventRecord(e1, st));
            call.walk(call.qall.as<float>(), call.scanI.as<int64_t>(), 1, ks, false, np, pending.data(), &e2);
            times.ms[T_SCAN] += ms_between(e0, e1);
            times.ms[T_SCAN_WALK] += ms_between(e1, e2);
            stats[3] = np;
        }
        note();
    });
}

int vs_set_fuse_mode(vs_index* ix, int tier) {
    return guarded([&] {
        check_index(ix);
        if (tier != VS_FUSE_AUTO && tier != VS_FUSE_LISTS && tier != VS_FUSE_SCAN)
            throw VsError(VS_ERR_ARG, "fuse tier must be VS_FUSE_AUTO, _LISTS or _SCAN");
        ix->fuse_mode.store(tier);
    });
}

int vs_set_fuse_depth(vs_index* ix, int32_t first, int32_t limit) {
    return guarded([&] {
        check_index(ix);
        ix->fu.set(first, limit, K_MAX, "fuse");
    });
}

int vs_fuse_last_stats(vs_index* ix, int64_t* out, int cap) {
    return guarded([&] {
        check_index(ix);
        copy_last(ix->fu.mu, ix->fu.stats, 6, out, cap, "stats");
    });
}

int vs_fuse_last_times(vs_index* ix, double* out, int cap) {
    return guarded([&] {
        check_index(ix);
        copy_last(ix->fu.mu, ix->fu.times, 6, out, cap, "times");
    });
}

}  // extern "C"

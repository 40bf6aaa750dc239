// vs_adjust_host.hip -- host side of the adjusted search (include/vs.h "adjusted search"; kernels:
// vs_adjust.hip): the vs_adjust object, its validation, the tiers and their stats.
//
// Every tier walks exact plain top-L lists (exact_lists, deepened by deepen_lists of vs_walk.h) with
// k_adjust_walk, which rescores each entry, forms A and ranks by (A, id):
//   DIRECT  one adjusted scan over the object's adjusted rows first (their exact top-min(k, m_adj) by A);
//           the walk drops the list's adjusted entries and merges the plain ones with that list.  Complete
//           iff the list held k plain entries, or every member.
//   BOUND   complete iff the list's k-th best A strictly beats the bound on every member behind the list.
//   SCAN    the adjusted scan over every member, then a walk over its k rows for their plain scores.
#include "vs_walk.h"

using namespace vs;

namespace {

enum { T_DIRECT_SCAN = 4, T_FULL_SCAN = 5 };  // slots of WalkTimes::ms behind the two list tiers'
constexpr int kAdjScanRows = 64;              // list positions (rows) per scan workgroup, at least

void check_adjust(const vs_index* ix, const vs_adjust* aj) {
    if (!aj) throw VsError(VS_ERR_ARG, "null adjustment");
    if (aj->ix != ix) throw VsError(VS_ERR_ARG, "adjustment belongs to another index");
    if (aj->gen != ix->reset_gen.load() || aj->n_cov > ix->ntotal)
        throw VsError(VS_ERR_ARG, "stale adjustment (the index was reset, or rows were removed, after it was made)");
}

void check_pair(float s, float b, int64_t i) {
    if (!(std::isfinite(s) && s >= 0.0f))
        throw VsError(VS_ERR_ARG, "scale must be finite and >= 0 (entry " + std::to_string(i) + ")");
    if (!std::isfinite(b)) throw VsError(VS_ERR_ARG, "bias must be finite (entry " + std::to_string(i) + ")");
}

// the object of validated dense host arrays (n = ntotal rows)
vs_adjust* make_adjust(vs_index* ix, const std::vector<float>& scale, const std::vector<float>& bias) {
    const int64_t n = (int64_t)scale.size();
    std::unique_ptr<vs_adjust, void (*)(vs_adjust*)> aj(new vs_adjust(), vs_adjust_destroy);
    aj->ix = ix;
    aj->gen = ix->reset_gen.load();
    aj->device = ix->device;
    aj->n_cov = n;
    if (n > 0) {
        std::vector<uint32_t> ids;
        float ext[4] = {scale[0], scale[0], bias[0], bias[0]};
        for (int64_t i = 0; i < n; ++i) {
            if (!(scale[(size_t)i] == 1.0f && bias[(size_t)i] == 0.0f)) ids.push_back((uint32_t)i);
            ext[0] = std::min(ext[0], scale[(size_t)i]);
            ext[1] = std::max(ext[1], scale[(size_t)i]);
            ext[2] = std::min(ext[2], bias[(size_t)i]);
            ext[3] = std::max(ext[3], bias[(size_t)i]);
        }
        aj->m_adj = (int64_t)ids.size();
        aj->smin = ext[0];
        aj->smax = ext[1];
        aj->bmin = ext[2];
        aj->bmax = ext[3];
        aj->scale.ensure((size_t)n * sizeof(float));
        aj->bias.ensure((size_t)n * sizeof(float));
        aj->ids.ensure((size_t)std::max<int64_t>(aj->m_adj, 1) * sizeof(uint32_t));
        aj->ext.ensure(sizeof(ext));
        HIP_CHECK(hipMemcpy(aj->scale.p, scale.data(), (size_t)n * sizeof(float), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(aj->bias.p, bias.data(), (size_t)n * sizeof(float), hipMemcpyHostToDevice));
        if (aj->m_adj)
            HIP_CHECK(hipMemcpy(aj->ids.p, ids.data(), ids.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(aj->ext.p, ext, sizeof(ext), hipMemcpyHostToDevice));
    }
    return aj.release();
}

// a walk's block for m queries of k entries, on the device and copied to the host:
// [I int64 mk | D fp32 mk | D_raw fp32 mk | complete int32 m]
struct AjBlock {
    int64_t* I;
    float *D, *R;
    int32_t* complete;
    size_t bytes;
};
AjBlock aj_block(const void* base, size_t m, size_t mk) {
    Carver c(base);
    AjBlock b{c.take<int64_t>(mk), c.take<float>(mk), c.take<float>(mk), c.take<int32_t>(m)};
    b.bytes = c.used;
    return b;
}

// one call's state: the scratch (freed with it, before the call returns) and where the answers go
struct AjCall {
    vs_index* ix;
    Ctx* c;
    const vs_adjust* aj;
    hipStream_t st;
    int k;
    float* D;
    int64_t* I;
    float* R;  // (may be null)
    std::vector<int32_t> complete;
    DevBuf out_d, stmp, qmap_d, scanI, cert, qall;
    std::vector<uint8_t> h;

    AdjustRows rows(const vs_sel* user_sel) const {
        AdjustRows r{};
        r.scale = aj->scale.as<float>();
        r.bias = aj->bias.as<float>();
        r.n_cov = aj->n_cov;
        r.sel_bits = user_sel ? user_sel->bits : nullptr;
        r.n_sel = user_sel ? user_sel->n_sel : 0;
        return r;
    }

    // the walk over m queries (device, [m][d] at qd): their lists Il [m][L] (or null) and the scan lists
    // Is [..][ks] (or null; query j's is row idx[j] when by_idx); answers into rows idx[j] of the outputs
    void walk(const float* qd, const int64_t* Il, int64_t L, const int64_t* Is, int ks, bool by_idx, int mode, int64_t m,
              const int64_t* idx, DevEvent* ev_done) {
        const size_t mk = (size_t)m * k;
        const size_t bytes = aj_block(nullptr, m, mk).bytes;
        out_d.ensure(bytes);
        const AjBlock dev = aj_block(out_d.p, m, mk);
        const int64_t n_ent = (Il ? L : 0) + (Is ? ks : 0);
        stmp.ensure((size_t)m * n_ent * sizeof(double));
        AdjustWalkArgs a{};
        a.corpus = ix->data;
        a.d = ix->d;
        a.dpad = ix->dpad;
        a.dt = ix->dtype;
        a.metric = ix->metric;
        a.rows = rows(nullptr);
        a.L = L;
        a.ks = ks;
        a.mode = mode;
        a.smin = aj->smin;
        a.smax = aj->smax;
        a.bmin = aj->bmin;
        a.bmax = aj->bmax;
        a.k = k;
        if (Is && by_idx) {
            qmap_d.ensure((size_t)m * sizeof(int64_t));
            HIP_CHECK(hipMemcpyAsync(qmap_d.p, idx, (size_t)m * sizeof(int64_t), hipMemcpyHostToDevice, st));
        }
        const int64_t qmax = 65536;  // workgroups of one launch
        for (int64_t q0 = 0; q0 < m; q0 += qmax) {
            const int nq = (int)std::min(qmax, m - q0);
            a.q = qd + q0 * ix->d;
            a.I_list = Il ? Il + q0 * L : nullptr;
            a.I_scan = Is ? (by_idx ? Is : Is + q0 * ks) : nullptr;
            a.qmap = Is && by_idx ? qmap_d.as<int64_t>() + q0 : nullptr;
            a.S_tmp = stmp.as<double>() + q0 * n_ent;
            a.I = dev.I + q0 * k;
            a.D = dev.D + q0 * k;
            a.D_raw = dev.R + q0 * k;
            a.complete = dev.complete + q0;
            HIP_CHECK(launch_adjust_walk(a, nq, st));
        }
        if (ev_done) HIP_CHECK(hipEventRecord(*ev_done, st));
        h.resize(bytes);
        HIP_CHECK(hipMemcpyAsync(h.data(), out_d.p, bytes, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        const AjBlock w = aj_block(h.data(), m, mk);
        for (int64_t j = 0; j < m; ++j) {
            const int64_t r = idx[j];
            std::copy(w.I + j * k, w.I + (j + 1) * k, I + r * k);
            std::copy(w.D + j * k, w.D + (j + 1) * k, D + r * k);
            if (R) std::copy(w.R + j * k, w.R + (j + 1) * k, R + r * k);
            complete[(size_t)r] = w.complete[j];
        }
    }

    // the adjusted scan of m device queries at depth ks into scanI [m][ks]: over the listed rows (ids, n_ids)
    // or over rows [0, n_cov)
    void scan(const float* qd, int64_t m, int ks, const uint32_t* ids, int64_t n_ids, const vs_sel* user_sel) {
        scanI.ensure((size_t)m * ks * sizeof(int64_t));
        cert.ensure((size_t)m * sizeof(int));
        const AdjustRows r = rows(user_sel);
        for (int64_t q0 = 0; q0 < m; q0 += MFMA_QB) {
            const int nqb = (int)std::min<int64_t>(MFMA_QB, m - q0);
            const SearchOut out{nullptr, scanI.as<int64_t>() + q0 * ks, nullptr, cert.as<int>() + q0};
            FullScanArgs a = full_scan_args(ix, c, ids ? n_ids : aj->n_cov, kAdjScanRows, std::min(ix->num_cu, FS_B),
                                            qd + q0 * ix->d, nqb, ks, out, true, st);
            if (!ids) a.n_valid = aj->n_cov;
            // a short list leaves CUs idle: deal the block's queries over as many slices as fill them
            const int qy = ids ? std::max(1, std::min(nqb, ix->num_cu / a.G)) : 1;
            HIP_CHECK(launch_adjust_scan(a, r, ids, n_ids, qy, st));
        }
    }
};

}  // namespace

extern "C" {

int vs_adjust_create(vs_index* ix, const float* scale, const float* bias, int64_t n, vs_adjust** out) {
    return guarded([&] {
        if (!out) throw VsError(VS_ERR_ARG, "out is null");
        *out = nullptr;
        check_index(ix);
        std::shared_lock<std::shared_mutex> lk(ix->rw);
        DeviceGuard dg(ix->device);
        if (n != ix->ntotal) throw VsError(VS_ERR_ARG, "adjustment: one (scale, bias) per row, n must equal ntotal");
        if (n >= 0xFFFFFFFFll) throw VsError(VS_ERR_ARG, "adjustment ids are 32-bit");
        std::vector<float> s((size_t)n, 1.0f), b((size_t)n, 0.0f);
        if (scale) std::copy(scale, scale + n, s.begin());
        if (bias) std::copy(bias, bias + n, b.begin());
        for (int64_t i = 0; i < n; ++i) check_pair(s[(size_t)i], b[(size_t)i], i);
        *out = make_adjust(ix, s, b);
    });
}

int vs_adjust_create_sparse(vs_index* ix, const int64_t* ids, const float* scale, const float* bias, int64_t m,
                            vs_adjust** out) {
    return guarded([&] {
        if (!out) throw VsError(VS_ERR_ARG, "out is null");
        *out = nullptr;
        check_index(ix);
        std::shared_lock<std::shared_mutex> lk(ix->rw);
        DeviceGuard dg(ix->device);
        const int64_t n = ix->ntotal;
        if (m < 0 || (m > 0 && !ids)) throw VsError(VS_ERR_ARG, "adjustment: m entries need m ids");
        if (n >= 0xFFFFFFFFll) throw VsError(VS_ERR_ARG, "adjustment ids are 32-bit");
        std::vector<float> s((size_t)n, 1.0f), b((size_t)n, 0.0f);
        std::vector<bool> seen((size_t)n, false);
        for (int64_t i = 0; i < m; ++i) {
            if (ids[i] < 0 || ids[i] >= n)
                throw VsError(VS_ERR_ARG, "adjustment id out of range (entry " + std::to_string(i) + ")");
            if (seen[(size_t)ids[i]]) throw VsError(VS_ERR_ARG, "adjustment ids must be distinct (entry " + std::to_string(i) + ")");
            seen[(size_t)ids[i]] = true;
            const float si = scale ? scale[i] : 1.0f, bi = bias ? bias[i] : 0.0f;
            check_pair(si, bi, i);
            s[(size_t)ids[i]] = si;
            b[(size_t)ids[i]] = bi;
        }
        *out = make_adjust(ix, s, b);
    });
}

void vs_adjust_destroy(vs_adjust* aj) {
    if (!aj) return;
    int prev = -1;
    (void)hipGetDevice(&prev);
    if (prev != aj->device) (void)hipSetDevice(aj->device);
    aj->scale.release();
    aj->bias.release();
    aj->ids.release();
    aj->ext.release();
    if (prev >= 0 && prev != aj->device) (void)hipSetDevice(prev);
    delete aj;
}

int64_t vs_adjust_count(const vs_adjust* aj) { return aj ? aj->m_adj : -1; }
int64_t vs_adjust_rows(const vs_adjust* aj) { return aj ? aj->n_cov : -1; }

int vs_search_adjusted(vs_index* ix, const vs_adjust* aj, const vs_sel* sel, const float* q, int64_t nq, int32_t k,
                       float* D, int64_t* I, float* D_raw) {
    return guarded([&] {
        check_index(ix);
        if (nq < 0) throw VsError(VS_ERR_ARG, "nq must be >= 0");
        if (k < 1 || k > K_MAX) throw VsError(VS_ERR_ARG, "k must be in 1.." + std::to_string(K_MAX));
        std::shared_lock<std::shared_mutex> lk(ix->rw);
        check_adjust(ix, aj);
        if (sel) check_sel(ix, sel);
        const int64_t m_adj = aj->m_adj;
        const WalkState::Depth depth = ix->aj.resolve(k + std::min<int64_t>(m_adj, std::max(k, 64)), K_MAX);
        const int64_t limit = depth.limit;
        int tier = ix->adjust_mode.load();
        if (tier == VS_ADJUST_DIRECT && m_adj + k > limit)
            throw VsError(VS_ERR_ARG, "VS_ADJUST_DIRECT needs adjusted rows + k <= the depth limit (vs_set_adjust_depth)");
        if (tier == VS_ADJUST_AUTO) tier = m_adj + k <= limit ? VS_ADJUST_DIRECT : VS_ADJUST_BOUND;
        int64_t stats[7] = {nq, 0, 0, 0, 0, tier, m_adj};
        WalkTimes times;
        auto note = [&] { ix->aj.note(stats, 7, times.ms, 8); };
        if (nq == 0) {
            note();
            return;
        }
        if (!q || !D || !I) throw VsError(VS_ERR_ARG, "null host buffer");
        const float fillD = worst_score(ix);
        fill_padding(D, I, nq * k, fillD);
        if (D_raw) std::fill(D_raw, D_raw + nq * k, fillD);
        if (aj->n_cov == 0 || (sel && sel->m == 0)) {  // nothing to rank: all padding
            stats[1] = nq;
            note();
            return;
        }
        // (the longest walk: the deepest list and, under DIRECT, the scan list behind it)
        if (adjust_walk_lds(std::max<int64_t>(limit, k) + (tier == VS_ADJUST_DIRECT ? std::min<int64_t>(k, m_adj) : 0),
                            ix->d) > AJ_DYN_CAP)
            throw VsError(VS_ERR_ARG, "adjusted search: d too large for this depth limit (vs_set_adjust_depth)");
        DeviceGuard dg(ix->device);
        CtxLease lease(ix, nullptr, true);
        Ctx* c = lease.c;
        hipStream_t st = c->stream;
        // ---- the member set: the covered rows, under the selector those of them it allows -------------
        const vs_sel* msel = nullptr;
        TempSel cover;  // the selector cut to the covered rows, when rows were added behind the adjustment
        int64_t members = aj->n_cov;
        if (sel || aj->n_cov != ix->ntotal) {
            msel = sel;
            if (!sel || sel->n_sel > aj->n_cov) {
                cover.cover(ix, sel, aj->n_cov, st);
                msel = &cover.s;
            }
            members = msel->m;
        }
        if (members == 0) {
            stats[1] = nq;
            note();
            return;
        }
        AjCall call{ix, c, aj, st, k, D, I, D_raw, std::vector<int32_t>((size_t)nq, 0)};
        DevEvent e0(hipEventDefault), e1(hipEventDefault);
        std::vector<int64_t> pending;
        if (tier == VS_ADJUST_SCAN || (tier == VS_ADJUST_BOUND && std::min(limit, members) < std::min<int64_t>(k, members))) {
            // (BOUND: no list within the limit holds k rows, so none can certify)
            pending.resize((size_t)nq);
            for (int64_t i = 0; i < nq; ++i) pending[(size_t)i] = i;
        } else {
            // ---- DIRECT: the exact top-min(k, m_adj) of the adjusted members, every query, one scan ----
            int ks = 0;
            if (tier == VS_ADJUST_DIRECT && m_adj > 0) {
                ks = (int)std::min<int64_t>(k, m_adj);
                call.qall.ensure((size_t)nq * ix->d * sizeof(float));
                HIP_CHECK(hipEventRecord(e0, st));
                HIP_CHECK(hipMemcpyAsync(call.qall.p, q, (size_t)nq * ix->d * sizeof(float), hipMemcpyHostToDevice, st));
                call.scan(call.qall.as<float>(), nq, ks, aj->ids.as<uint32_t>(), m_adj, sel);
                HIP_CHECK(hipEventRecord(e1, st));
                HIP_CHECK(hipStreamSynchronize(st));
                times.ms[T_DIRECT_SCAN] += ms_between(e0, e1);
            }
            // ---- exact plain top-L lists, walked on the device; not complete goes deeper ----------------
            const int mode = tier == VS_ADJUST_DIRECT ? AJ_DIRECT : AJ_BOUND;
            Deepened dl = deepen_lists(
                ix, c, st, msel, members, depth.first, limit, q, nq, times,
                [&](const StagedOut& so, int64_t L, int64_t m, const int64_t* idx, DevEvent* ev) {
                    call.walk(c->qdev.as<float>(), so.Id, L, ks ? call.scanI.as<int64_t>() : nullptr, ks, true, mode, m, idx,
                              ev);
                },
                [&](int64_t r) { return call.complete[(size_t)r] != 0; });
            stats[1] = dl.done[0];
            stats[2] = dl.done[1];
            stats[4] = dl.longest;
            pending.swap(dl.pending);
            if (tier == VS_ADJUST_DIRECT && !pending.empty())
                throw VsError(VS_ERR_INTERNAL, "adjusted search: a list of k + adjusted rows did not complete");
        }
        // ---- SCAN: the adjusted scan over every member, then the walk over its rows ---------------------
        if (!pending.empty()) {
            const int64_t np = (int64_t)pending.size();
            const int ks = (int)std::min<int64_t>(k, members);
            std::vector<float> qsub((size_t)np * ix->d);
            for (int64_t j = 0; j < np; ++j)
                std::copy(q + pending[(size_t)j] * ix->d, q + (pending[(size_t)j] + 1) * ix->d, qsub.begin() + j * ix->d);
            call.qall.ensure(qsub.size() * sizeof(float));
            HIP_CHECK(hipEventRecord(e0, st));
            HIP_CHECK(hipMemcpyAsync(call.qall.p, qsub.data(), qsub.size() * sizeof(float), hipMemcpyHostToDevice, st));
            // (a selector whose rows all lie inside the covered ones is scanned by its own list)
            if (msel) call.scan(call.qall.as<float>(), np, ks, msel->ids, msel->m, nullptr);
            else call.scan(call.qall.as<float>(), np, ks, nullptr, 0, nullptr);
            call.walk(call.qall.as<float>(), nullptr, 0, call.scanI.as<int64_t>(), ks, false, AJ_PLAIN, np, pending.data(), &e1);
            times.ms[T_FULL_SCAN] += ms_between(e0, e1);
            stats[3] = np;
        }
        note();
    });
}

int vs_set_adjust_mode(vs_index* ix, int mode) {
    return guarded([&] {
        check_index(ix);
        if (mode != VS_ADJUST_AUTO && mode != VS_ADJUST_DIRECT && mode != VS_ADJUST_BOUND && mode != VS_ADJUST_SCAN)
            throw VsError(VS_ERR_ARG, "adjust mode must be VS_ADJUST_AUTO, _DIRECT, _BOUND or _SCAN");
        ix->adjust_mode.store(mode);
    });
}

int vs_set_adjust_depth(vs_index* ix, int32_t first, int32_t limit) {
    return guarded([&] {
        check_index(ix);
        ix->aj.set(first, limit, K_MAX, "adjust");
    });
}

int vs_adjust_last_stats(vs_index* ix, int64_t* out, int cap) {
    return guarded([&] {
        check_index(ix);
        copy_last(ix->aj.mu, ix->aj.stats, 7, out, cap, "stats");
    });
}

int vs_adjust_last_times(vs_index* ix, double* out, int cap) {
    return guarded([&] {
        check_index(ix);
        copy_last(ix->aj.mu, ix->aj.times, 6, out, cap, "times");
    });
}

}  // extern "C"

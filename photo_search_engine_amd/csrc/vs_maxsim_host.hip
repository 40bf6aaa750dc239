// vs_maxsim_host.hip -- host side of the multi-vector search (include/vs.h "multi-vector search"; kernels:
// vs_maxsim.hip): the member lists of a groups object, the argument checks, the tiers and their
// stats.
//
//   LISTS  the exact top-L lists of the nq m sub-queries among the members (exact_lists through
//          deepen_lists of vs_walk.h, a query's m sub-queries always in one staged chunk), walked by
//          k_maxsim_walk: the groups the lists touch are scored member by member and ranked by (F, code);
//          deepened until the walk's certificate holds.
//   SCAN   k_maxsim_scan over every member into the per-group table of maxima, k_maxsim_rank for the k best
//          codes, then the same walk over those groups for every output.
#include "vs_walk.h"

using namespace vs;

namespace {

enum { T_SCAN = 4, T_RANK = 5, T_SCAN_WALK = 6 };  // slots of WalkTimes::ms behind the two list tiers'
constexpr int64_t kKeyPad = -0x7FFFFFFFFFFFFFFFll - 1;
constexpr int kMaxsimScanRows = 64;               // rows per scan workgroup, at least
constexpr size_t kMaxsimWalkScratch = 64u << 20;  // the walk's scratch per launch, about
constexpr int64_t kMaxsimWalkRowsPerQuery = 400;  // the default row cap of one walk, per query of the call up to
constexpr int64_t kMaxsimWalkQueries = 256;       // ... this many (where the walk's time meets the scan's)
std::atomic<int64_t> g_maxsim_staging{64ll << 20};  // vs_set_maxsim_staging_bytes

int64_t maxsim_k_limit(int m) { return std::min<int64_t>(K_MAX, FUSE_WALK_MAX / m); }

// The member lists of a groups object, made by the first multi-vector call with it: the covered rows by
// (code, id) and the offsets of every code's list.  The codes are read back and counted on the host, as the
// object's creation sorted them there.  (The device of the object is current.)
void ensure_member_lists(const vs_groups* gr) {
    std::lock_guard<std::mutex> g(gr->ml_mu);
    if (gr->ml_built) return;
    const int64_t n = gr->n_cov, ncodes = gr->G + gr->U;
    std::vector<int32_t> gid((size_t)n);
    HIP_CHECK(hipMemcpy(gid.data(), gr->gid.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    std::vector<int64_t> off((size_t)ncodes + 1, 0);
    auto code_of = [&](int64_t i) {
        const int64_t c = gid[(size_t)i] >= 0 ? (int64_t)gid[(size_t)i] : gr->G + (int64_t)(~gid[(size_t)i]);
        if (c < 0 || c >= ncodes) throw VsError(VS_ERR_INTERNAL, "multi-vector search: a group code out of range");
        return c;
    };
    for (int64_t i = 0; i < n; ++i) ++off[(size_t)code_of(i) + 1];
    for (int64_t c = 0; c < ncodes; ++c) off[(size_t)c + 1] += off[(size_t)c];
    std::vector<int64_t> pos(off.begin(), off.end() - 1);
    std::vector<uint32_t> rows((size_t)n);
    for (int64_t i = 0; i < n; ++i) rows[(size_t)pos[(size_t)code_of(i)]++] = (uint32_t)i;  // (ids ascend inside a code)
    DevBuf d_rows, d_off;
    d_rows.ensure((size_t)n * sizeof(uint32_t));
    d_off.ensure(off.size() * sizeof(int64_t));
    HIP_CHECK(hipMemcpy(d_rows.p, rows.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(d_off.p, off.data(), off.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    gr->ml_rows = std::move(d_rows);
    gr->ml_off = std::move(d_off);
    gr->ml_built = true;
}

// a walk's block for n queries of k groups, on the device and copied to the host:
// [keys int64 nk | F fp64 nk | I_sub int64 nk m | sizes int64 nk | walked int64 n | D_sub fp32 nk m | complete int32 n]
struct MxBlock {
    int64_t* keys;
    double* F;
    int64_t *I, *sizes, *walked;
    float* D;
    int32_t* complete;
    size_t bytes;
};
MxBlock mx_block(const void* base, size_t n, size_t nk, int m) {
    Carver c(base);
    MxBlock b{c.take<int64_t>(nk), c.take<double>(nk),   c.take<int64_t>(nk * m), c.take<int64_t>(nk),
              c.take<int64_t>(n),  c.take<float>(nk * m), c.take<int32_t>(n)};
    b.bytes = c.used;
    return b;
}

// one call's state: the scratch (freed with it, before the call returns) and where the answers go
struct MxCall {
    vs_index* ix;
    const vs_groups* gr;
    const vs_sel* msel;  // the members' selector (null: every covered row)
    hipStream_t st;
    int m, k;
    int64_t members, walk_rows;
    int64_t* keys;
    double* F;
    float* D_sub;    // (may be null)
    int64_t* I_sub;  // (may be null)
    int64_t* sizes;  // (may be null)
    std::vector<int32_t> complete;  // per query: 1 complete, 0 open, 2 over the row cap
    std::vector<int64_t> capped;    // the queries a walk left to the scan, and how many of them per list tier
    int64_t n_capped[2] = {0, 0};
    int variant = 0;  // MaxsimScanArgs::variant
    int64_t walked = 0;
    DevBuf out_d, mtmp, itmp, ctmp, ztmp, table, cand, qall;
    std::vector<uint8_t> h;

    MaxsimGroups groups() const {
        return MaxsimGroups{gr->gid.as<int32_t>(), gr->n_cov, gr->G, gr->G + gr->U, gr->ml_rows.as<uint32_t>(),
                            gr->ml_off.as<int64_t>(), gr->gkey.as<int64_t>(), gr->ukey.as<int64_t>()};
    }

    // the walk over n queries (device, [n][m][d] at qd) and their candidates cand [n][nl][L] (row ids, or
    // group codes); complete answers into rows idx[j] of the outputs
    void walk(const float* qd, const int64_t* cand_d, int nl, int64_t L, bool codes, int64_t n, const int64_t* idx,
              DevEvent* ev_done, int tier = 0) {
        const size_t nk = (size_t)n * k;
        const size_t bytes = mx_block(nullptr, n, nk, m).bytes;
        out_d.ensure(bytes);
        const MxBlock dev = mx_block(out_d.p, n, nk, m);
        const int64_t n_ent = nl * L;
        // the scratch rows of one launch: as many queries at a time as kMaxsimWalkScratch holds
        const int64_t per_q = n_ent * (m * (int64_t)(sizeof(double) + sizeof(uint32_t)) + 8);
        const int64_t qn = std::min(n, std::max<int64_t>(1, std::min<int64_t>(65535, (int64_t)kMaxsimWalkScratch / per_q)));
        mtmp.ensure((size_t)qn * n_ent * m * sizeof(double));
        itmp.ensure((size_t)qn * n_ent * m * sizeof(uint32_t));
        ctmp.ensure((size_t)qn * n_ent * sizeof(uint32_t));
        ztmp.ensure((size_t)qn * n_ent * sizeof(int32_t));
        MaxsimWalkArgs a{};
        a.corpus = ix->data;
        a.d = ix->d;
        a.dpad = ix->dpad;
        a.dt = ix->dtype;
        a.metric = ix->metric;
        a.n_valid = ix->ntotal;
        a.g = groups();
        a.sel_bits = msel ? msel->bits : nullptr;
        a.n_sel = msel ? msel->n_sel : 0;
        a.m = m;
        a.nl = nl;
        a.L = L;
        a.codes = codes ? 1 : 0;
        a.hold_all = !codes && L >= members ? 1 : 0;
        a.walk_rows = walk_rows;
        a.k = k;
        a.M_tmp = mtmp.as<double>();
        a.I_tmp = itmp.as<uint32_t>();
        a.C_tmp = ctmp.as<uint32_t>();
        a.Z_tmp = ztmp.as<int32_t>();
        for (int64_t q0 = 0; q0 < n; q0 += qn) {  // (stream order: a launch's scratch is free for the next)
            const int nq = (int)std::min(qn, n - q0);
            a.q = qd + q0 * m * ix->d;
            a.cand = cand_d + q0 * n_ent;
            a.keys = dev.keys + q0 * k;
            a.F = dev.F + q0 * k;
            a.D_sub = dev.D + q0 * k * m;
            a.I_sub = dev.I + q0 * k * m;
            a.sizes = dev.sizes + q0 * k;
            a.complete = dev.complete + q0;
            a.walked = dev.walked + q0;
            HIP_CHECK(launch_maxsim_walk(a, nq, st));
        }
        if (ev_done) HIP_CHECK(hipEventRecord(*ev_done, st));
        h.resize(bytes);
        HIP_CHECK(hipMemcpyAsync(h.data(), out_d.p, bytes, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        const MxBlock w = mx_block(h.data(), n, nk, m);
        const int64_t km = (int64_t)k * m;
        for (int64_t j = 0; j < n; ++j) {
            const int64_t r = idx[j];
            complete[(size_t)r] = w.complete[j];
            // an open query's next lists are four times as long: past the cap by that estimate, it goes as well
            if (w.complete[j] == 0 && !codes && 4 * w.walked[j] > walk_rows) complete[(size_t)r] = 2;
            if (complete[(size_t)r] == 2) {  // over the row cap: deeper lists only add candidates, the scan answers it
                capped.push_back(r);
                ++n_capped[tier];
            }
            if (w.complete[j] != 1) continue;  // (left open: nothing of it was written)
            walked += w.walked[j];
            std::copy(w.keys + j * k, w.keys + (j + 1) * k, keys + r * k);
            std::copy(w.F + j * k, w.F + (j + 1) * k, F + r * k);
            if (D_sub) std::copy(w.D + j * km, w.D + (j + 1) * km, D_sub + r * km);
            if (I_sub) std::copy(w.I + j * km, w.I + (j + 1) * km, I_sub + r * km);
            if (sizes) std::copy(w.sizes + j * k, w.sizes + (j + 1) * k, sizes + r * k);
        }
    }

    // the scan, the rank and the walk for the np queries idx[0, np) (device, [np][m][d] at qd)
    void scan(const float* qd, int64_t np, const int64_t* idx, WalkTimes& times) {
        const int64_t ncodes = gr->G + gr->U;
        const int64_t row_bytes = (int64_t)m * ncodes * (int64_t)sizeof(unsigned long long);  // one query's table
        const int64_t nqb_max = std::max<int64_t>(1, std::min<int64_t>(np, g_maxsim_staging.load() / row_bytes));
        table.ensure((size_t)(nqb_max * row_bytes));
        cand.ensure((size_t)nqb_max * k * sizeof(int64_t));
        const uint32_t* ids = msel ? msel->ids : nullptr;
        const int64_t nseq = msel ? msel->m : gr->n_cov;
        const int G = (int)std::max<int64_t>(1, std::min<int64_t>(ix->num_cu, (nseq + kMaxsimScanRows - 1) / kMaxsimScanRows));
        DevEvent e0(hipEventDefault), e1(hipEventDefault), e2(hipEventDefault), e3(hipEventDefault);
        for (int64_t q0 = 0; q0 < np; q0 += nqb_max) {
            const int nqb = (int)std::min(nqb_max, np - q0);
            HIP_CHECK(hipEventRecord(e0, st));
            HIP_CHECK(hipMemsetAsync(table.p, 0, (size_t)(nqb * row_bytes), st));
            MaxsimScanArgs a{};
            a.corpus = ix->data;
            a.d = ix->d;
            a.dpad = ix->dpad;
            a.dt = ix->dtype;
            a.metric = ix->metric;
            a.g = groups();
            a.q = qd + q0 * m * ix->d;
            a.nq = nqb;
            a.m = m;
            a.table = table.as<unsigned long long>();
            a.variant = variant;
            // fewer workgroups than CUs (few members): deal the block's queries over as many slices as fill them
            const int qy = std::max(1, std::min(nqb, ix->num_cu / G));
            HIP_CHECK(launch_maxsim_scan(a, ids, nseq, G, qy, st));
            HIP_CHECK(hipEventRecord(e1, st));
            HIP_CHECK(launch_maxsim_rank(table.as<unsigned long long>(), nqb, m, ncodes, ix->metric, k, cand.as<int64_t>(), st));
            HIP_CHECK(hipEventRecord(e2, st));
            walk(qd + q0 * m * ix->d, cand.as<int64_t>(), 1, k, true, nqb, idx + q0, &e3);
            times.ms[T_SCAN] += ms_between(e0, e1);
            times.ms[T_RANK] += ms_between(e1, e2);
            times.ms[T_SCAN_WALK] += ms_between(e2, e3);
        }
    }
};

}  // namespace

extern "C" {

int vs_search_maxsim(vs_index* ix, const vs_groups* gr, const vs_sel* sel, const float* q, int64_t nq, int32_t m,
                     int32_t k, int64_t* keys_out, double* F, float* D_sub, int64_t* I_sub, int64_t* sizes) {
    return guarded([&] {
        check_index(ix);
        if (nq < 0) throw VsError(VS_ERR_ARG, "nq must be >= 0");
        if (m < 1 || m > VS_FUSE_MAX_Q)
            throw VsError(VS_ERR_ARG, "multi-vector search: m must be in 1.." + std::to_string(VS_FUSE_MAX_Q));
        const int64_t klim = maxsim_k_limit(m);
        if (k < 1 || k > klim)
            throw VsError(VS_ERR_ARG,
                          "multi-vector search: k must be in 1.." + std::to_string(klim) + " at m = " + std::to_string(m));
        std::shared_lock<std::shared_mutex> lk(ix->rw);
        check_groups(ix, gr);
        if (sel) check_sel(ix, sel);
        // (the depth settings: cut to this call's own limit)
        const int set_first = ix->mx.first.load(), set_limit = ix->mx.limit.load();
        const int64_t limit = set_limit > 0 ? std::min<int64_t>(set_limit, klim) : klim;
        const int64_t first = std::min<int64_t>(set_first > 0 ? set_first : std::max(4 * k, 64), limit);
        const int64_t set_rows = ix->maxsim_walk_rows.load();
        const int tier = ix->maxsim_mode.load() == VS_MAXSIM_SCAN ? VS_MAXSIM_SCAN : VS_MAXSIM_LISTS;
        int64_t stats[7] = {nq, 0, 0, 0, 0, tier, 0};
        WalkTimes times;
        auto note = [&] { ix->mx.note(stats, 7, times.ms, 8); };
        if (nq == 0) {
            note();
            return;
        }
        if (!q || !keys_out || !F) throw VsError(VS_ERR_ARG, "null host buffer");
        const float fillD = worst_score(ix);
        const int64_t nk = nq * k;
        std::fill(keys_out, keys_out + nk, kKeyPad);
        std::fill(F, F + nk, ix->metric == METRIC_L2 ? (double)INFINITY : -(double)INFINITY);
        if (D_sub) std::fill(D_sub, D_sub + nk * m, fillD);
        if (I_sub) std::fill(I_sub, I_sub + nk * m, (int64_t)-1);
        if (sizes) std::fill(sizes, sizes + nk, (int64_t)0);
        if (gr->n_cov == 0 || (sel && sel->m == 0)) {  // nothing to rank: all padding
            stats[1] = nq;
            note();
            return;
        }
        DeviceGuard dg(ix->device);
        ensure_member_lists(gr);
        CtxLease lease(ix, nullptr, true);
        Ctx* c = lease.c;
        hipStream_t st = c->stream;
        // ---- the member set: the covered rows, under the selector those of them it allows -------------
        const vs_sel* msel = nullptr;
        TempSel cover;  // the selector cut to the covered rows, when rows were added behind the groups
        int64_t members = gr->n_cov;
        if (sel || gr->n_cov != ix->ntotal) {
            msel = sel;
            if (!sel || sel->n_sel > gr->n_cov) {
                cover.cover(ix, sel, gr->n_cov, st);
                msel = &cover.s;
            }
            members = msel->m;
        }
        if (members == 0) {
            stats[1] = nq;
            note();
            return;
        }
        const int64_t walk_rows = set_rows > 0 ? set_rows : kMaxsimWalkRowsPerQuery * std::min(nq, kMaxsimWalkQueries);
        MxCall call{ix, gr, msel, st, m, k, members, walk_rows, keys_out, F, D_sub, I_sub, sizes,
                    std::vector<int32_t>((size_t)nq, 0)};
        if (const char* v = std::getenv("VS_MAXSIM_SCAN_VARIANT")) call.variant = std::atoi(v) & 3;  // (scripts/maxsim_timing.py)
        std::vector<int64_t> pending;
        if (tier == VS_MAXSIM_SCAN) {
            pending.resize((size_t)nq);
            for (int64_t i = 0; i < nq; ++i) pending[(size_t)i] = i;
        } else {
            // ---- exact top-L lists of every sub-query, walked on the device; not complete goes deeper ----
            const int64_t first_len = std::min(first, std::min(limit, members));
            Deepened dl = deepen_lists(
                ix, c, st, msel, members, first, limit, q, nq, times,
                [&](const StagedOut& so, int64_t L, int64_t n, const int64_t* idx, DevEvent* ev) {
                    call.walk(c->qdev.as<float>(), so.Id, m, L, false, n, idx, ev, L > first_len ? 1 : 0);
                },
                [&](int64_t r) { return call.complete[(size_t)r] != 0; }, m);
            stats[1] = dl.done[0] - call.n_capped[0];
            stats[2] = dl.done[1] - call.n_capped[1];
            stats[4] = dl.longest;
            pending.swap(dl.pending);
            pending.insert(pending.end(), call.capped.begin(), call.capped.end());
            std::sort(pending.begin(), pending.end());
        }
        // ---- SCAN: the table of maxima over every member, the k best codes, the walk over them ----------
        if (!pending.empty()) {
            const int64_t np = (int64_t)pending.size(), qd = (int64_t)m * ix->d;
            std::vector<float> qsub((size_t)np * qd);
            for (int64_t j = 0; j < np; ++j)
                std::copy(q + pending[(size_t)j] * qd, q + (pending[(size_t)j] + 1) * qd, qsub.begin() + j * qd);
            call.qall.ensure(qsub.size() * sizeof(float));
            HIP_CHECK(hipMemcpyAsync(call.qall.p, qsub.data(), qsub.size() * sizeof(float), hipMemcpyHostToDevice, st));
            call.scan(call.qall.as<float>(), np, pending.data(), times);
            for (int64_t r : pending)
                if (call.complete[(size_t)r] != 1) throw VsError(VS_ERR_INTERNAL, "multi-vector search: the scan's walk left a query open");
            stats[3] = np;
        }
        stats[6] = call.walked;
        note();
    });
}

int vs_set_maxsim_mode(vs_index* ix, int tier) {
    return guarded([&] {
        check_index(ix);
        if (tier != VS_MAXSIM_AUTO && tier != VS_MAXSIM_LISTS && tier != VS_MAXSIM_SCAN)
            throw VsError(VS_ERR_ARG, "multi-vector tier must be VS_MAXSIM_AUTO, _LISTS or _SCAN");
        ix->maxsim_mode.store(tier);
    });
}

int vs_set_maxsim_depth(vs_index* ix, int32_t first, int32_t limit, int64_t walk_rows) {
    return guarded([&] {
        check_index(ix);
        if (walk_rows < 0) throw VsError(VS_ERR_ARG, "maxsim walk_rows must be >= 0 (0 = default)");
        ix->mx.set(first, limit, K_MAX, "maxsim");
        ix->maxsim_walk_rows.store(walk_rows);
    });
}

int vs_set_maxsim_staging_bytes(int64_t bytes) {
    return guarded([&] {
        if (bytes < 1) throw VsError(VS_ERR_ARG, "maxsim staging bytes must be >= 1");
        g_maxsim_staging.store(bytes);
    });
}

int vs_maxsim_last_stats(vs_index* ix, int64_t* out, int cap) {
    return guarded([&] {
        check_index(ix);
        copy_last(ix->mx.mu, ix->mx.stats, 7, out, cap, "stats");
    });
}

int vs_maxsim_last_times(vs_index* ix, double* out, int cap) {
    return guarded([&] {
        check_index(ix);
        copy_last(ix->mx.mu, ix->mx.times, 7, out, cap, "times");
    });
}

}  // extern "C"

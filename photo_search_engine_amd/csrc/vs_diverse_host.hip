// vs_diverse_host.hip -- host side of the diversified search (include/vs.h "diversified search";
// kernel: vs_diverse.hip).
//
// The accepted list of a walk is prefix-stable, so a walk over the first L rows of a query's exact
// ranking that reaches k acceptances -- or that saw every member -- is the whole answer.  Tiers:
//   1  the exact top-L0 of every query (search_staged with the device block mirrored, or
//      sel_search_ctx), walked on the device;
//   2  the queries still short re-searched at 4 L, up to the limit, and walked again from scratch;
//   3  what is left gets its whole ranking from the range machinery (range_block with an infinite
//      radius, which honours a selector), uploaded as a list and walked by the same kernel.
#include "vs_index.h"

using namespace vs;

namespace {

struct DvTimes {
    double search[3] = {0, 0, 0}, walk[3] = {0, 0, 0};  // ms per tier (HIP events)
};

// where one call's answers go (hidden / examined always exist here; the caller's may be null)
struct DvOut {
    int k;
    float* D;
    int64_t* I;
    std::vector<int32_t> hidden;
    std::vector<int64_t> examined;
    std::vector<int32_t> nacc;
};

// the walk over m device lists [m][L]; rad_h[m]; query j's answer goes to row idx[j] of out
void walk_lists(const vs_index* ix, Ctx* c, const int64_t* Id, const float* Dd, int64_t L, int64_t m, const float* rad_h,
                const int64_t* idx, DvOut& out, hipStream_t st, DevEvent* ev_done) {
    const int k = out.k;
    const size_t mk = (size_t)m * k;
    const int64_t qmax = 65536;  // workgroups of one launch
    // [examined int64 m | I int64 mk | D fp32 mk | hidden int32 mk | nacc int32 m | radius fp32 m]
    const size_t bytes = (size_t)m * 8 + mk * 8 + mk * 4 + mk * 4 + (size_t)m * 4 + (size_t)m * 4;
    c->dv_out.ensure(bytes);
    DiverseArgs a{};
    a.corpus = ix->data;
    a.d = ix->d;
    a.dpad = ix->dpad;
    a.dt = ix->dtype;
    a.metric = ix->metric;
    a.n_valid = ix->ntotal;
    a.L = L;
    a.k = k;
    a.nqs = diverse_query_slots(ix->d);
    int64_t* ex_d = c->dv_out.as<int64_t>();
    int64_t* I_d = ex_d + m;
    float* D_d = (float*)(I_d + mk);
    int32_t* hid_d = (int32_t*)(D_d + mk);
    int32_t* nacc_d = hid_d + mk;
    float* rad_d = (float*)(nacc_d + m);
    HIP_CHECK(hipMemcpyAsync(rad_d, rad_h, (size_t)m * sizeof(float), hipMemcpyHostToDevice, st));
    for (int64_t q0 = 0; q0 < m; q0 += qmax) {
        const int nq = (int)std::min(qmax, m - q0);
        a.I_in = Id + q0 * L;
        a.D_in = Dd + q0 * L;
        a.radius = rad_d + q0;
        a.I = I_d + q0 * k;
        a.D = D_d + q0 * k;
        a.hidden = hid_d + q0 * k;
        a.nacc = nacc_d + q0;
        a.examined = ex_d + q0;
        HIP_CHECK(launch_diverse_walk(a, nq, st));
    }
    if (ev_done) HIP_CHECK(hipEventRecord(*ev_done, st));
    std::vector<uint8_t> h(bytes);
    HIP_CHECK(hipMemcpyAsync(h.data(), c->dv_out.p, bytes, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    const int64_t* ex_h = (const int64_t*)h.data();
    const int64_t* I_h = ex_h + m;
    const float* D_h = (const float*)(I_h + mk);
    const int32_t* hid_h = (const int32_t*)(D_h + mk);
    const int32_t* nacc_h = hid_h + mk;
    for (int64_t j = 0; j < m; ++j) {
        const int64_t g = idx[j];
        std::copy(I_h + j * k, I_h + (j + 1) * k, out.I + g * k);
        std::copy(D_h + j * k, D_h + (j + 1) * k, out.D + g * k);
        std::copy(hid_h + j * k, hid_h + (j + 1) * k, out.hidden.begin() + g * k);
        out.examined[(size_t)g] = ex_h[j];
        out.nacc[(size_t)g] = nacc_h[j];
    }
}

double ms_between(const DevEvent& a, const DevEvent& b) {
    float ms = 0.0f;
    HIP_CHECK(hipEventElapsedTime(&ms, a, b));
    return (double)ms;
}

void note_stats(vs_index* ix, const int64_t (&s)[5], const DvTimes& t) {
    std::lock_guard<std::mutex> g(ix->dv_mu);
    for (int i = 0; i < 5; ++i) ix->dv_stats[i] = s[i];
    for (int i = 0; i < 3; ++i) {
        ix->dv_times[2 * i] = t.search[i];
        ix->dv_times[2 * i + 1] = t.walk[i];
    }
}

}  // namespace

extern "C" {

int vs_search_diverse(vs_index* ix, const vs_sel* sel, const float* q, int64_t nq, int32_t k, const float* radius,
                      float* D, int64_t* I, int32_t* hidden, int64_t* examined) {
    return guarded([&] {
        check_index(ix);
        if (nq < 0) throw VsError(VS_ERR_ARG, "nq must be >= 0");
        if (k <= 0) throw VsError(VS_ERR_ARG, "k must be > 0");
        check_k(k);
        std::shared_lock<std::shared_mutex> lk(ix->rw);
        if (sel) check_sel(ix, sel);
        int64_t stats[5] = {nq, 0, 0, 0, 0};
        DvTimes times;
        if (nq == 0) {
            note_stats(ix, stats, times);
            return;
        }
        if (!q || !radius || !D || !I) throw VsError(VS_ERR_ARG, "null host buffer");
        for (int64_t i = 0; i < nq; ++i)
            if (std::isnan(radius[i])) throw VsError(VS_ERR_ARG, "radius is NaN (query " + std::to_string(i) + ")");
        const int64_t members = sel ? sel->m : ix->ntotal;
        fill_padding(D, I, nq * k, worst_score(ix));
        DvOut out{k, D, I, std::vector<int32_t>((size_t)nq * k, 0), std::vector<int64_t>((size_t)nq, 0),
                  std::vector<int32_t>((size_t)nq, 0)};
        auto deliver = [&] {
            if (hidden) std::copy(out.hidden.begin(), out.hidden.end(), hidden);
            if (examined) std::copy(out.examined.begin(), out.examined.end(), examined);
        };
        if (members == 0) {  // nothing to rank: all padding
            stats[1] = nq;
            deliver();
            note_stats(ix, stats, times);
            return;
        }
        if (diverse_query_slots(ix->d) < 1)
            throw VsError(VS_ERR_ARG, "the walk holds a stored row as an fp64 query in LDS: d must be <= 14336");
        DeviceGuard dg(ix->device);
        const int kmax = KP_MAX * 4 / 5;
        const int set_first = ix->dv_first.load(), set_limit = ix->dv_limit.load();
        const int64_t limit = set_limit > 0 ? set_limit : kmax;
        const int64_t first = std::min<int64_t>(set_first > 0 ? set_first : std::max<int64_t>(4 * (int64_t)k, 64), limit);
        const int64_t Lmax = std::min<int64_t>(limit, members);
        int64_t L = std::min<int64_t>(first, Lmax);
        CtxLease lease(ix, nullptr, true);
        Ctx* c = lease.c;
        hipStream_t st = c->stream;
        DevEvent e0(hipEventDefault), e1(hipEventDefault), e2(hipEventDefault);
        std::vector<int64_t> pending((size_t)nq), next;
        for (int64_t i = 0; i < nq; ++i) pending[(size_t)i] = i;
        std::vector<float> qsub, rsub;
        // ---- tiers 1 and 2: exact top-L lists, walked on the device --------------------------------
        for (bool first_pass = true;; first_pass = false) {
            const int64_t n = (int64_t)pending.size();
            const int tier = first_pass ? 0 : 1;
            const float* qp = q;
            if (!first_pass) {  // the short queries as one batch
                qsub.resize((size_t)n * ix->d);
                for (int64_t j = 0; j < n; ++j)
                    std::copy(q + pending[(size_t)j] * ix->d, q + (pending[(size_t)j] + 1) * ix->d, qsub.begin() + j * ix->d);
                qp = qsub.data();
            }
            rsub.resize((size_t)n);
            for (int64_t j = 0; j < n; ++j) rsub[(size_t)j] = radius[pending[(size_t)j]];
            const int kk = (int)L;
            const SelPlan plan = sel ? sel_plan(ix, sel, n, kk) : SelPlan{0, 0};
            const int64_t chunk = stage_chunk(ix, n, kk, !sel);
            next.clear();
            for (int64_t q0 = 0; q0 < n; q0 += chunk) {
                const int64_t m = std::min(chunk, n - q0);
                HIP_CHECK(hipEventRecord(e0, st));
                stage_queries(ix, c, qp, q0, m, st);
                const StagedOut so = staged_out(c, m, kk, !sel);
                if (sel) sel_search_ctx(ix, c, sel, plan, c->qdev.as<float>(), m, kk, SearchOut{so.Dd, so.Id}, st);
                else search_staged(ix, c, m, kk, so, st, true);
                HIP_CHECK(hipEventRecord(e1, st));
                walk_lists(ix, c, so.Id, so.Dd, L, m, rsub.data() + q0, pending.data() + q0, out, st, &e2);
                times.search[tier] += ms_between(e0, e1);
                times.walk[tier] += ms_between(e1, e2);
                for (int64_t j = 0; j < m; ++j) {
                    const int64_t g = pending[(size_t)(q0 + j)];
                    if (out.nacc[(size_t)g] < k && L < members) next.push_back(g);
                }
            }
            stats[4] = std::max(stats[4], L);
            stats[first_pass ? 1 : 2] += n - (int64_t)next.size();
            pending.swap(next);
            if (pending.empty() || L >= Lmax) break;
            L = std::min<int64_t>(4 * L, Lmax);
        }
        // ---- tier 3: the whole ranking of each query still short -----------------------------------
        const float all = ix->metric == METRIC_IP ? -INFINITY : INFINITY;
        for (int64_t g : pending) {
            HIP_CHECK(hipEventRecord(e0, st));
            stage_queries(ix, c, q, g, 1, st);
            RangeStats stt;
            int64_t counts[MFMA_QB];
            vs_range_result res;
            range_block(ix, c, sel, c->qdev.as<float>(), 1, &all, false, false, st, stt, counts, &res);
            const int64_t n = counts[0];
            ++stats[3];
            if (n <= 0) continue;  // (no member has a score to rank by)
            DevBuf lI, lD;  // (counted in vs_device_bytes_live, freed as the query is done)
            lI.ensure((size_t)n * sizeof(int64_t));
            lD.ensure((size_t)n * sizeof(float));
            HIP_CHECK(hipMemcpyAsync(lI.p, res.I.data(), (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, st));
            HIP_CHECK(hipMemcpyAsync(lD.p, res.D.data(), (size_t)n * sizeof(float), hipMemcpyHostToDevice, st));
            HIP_CHECK(hipEventRecord(e1, st));
            walk_lists(ix, c, lI.as<int64_t>(), lD.as<float>(), n, 1, radius + g, &g, out, st, &e2);
            times.search[2] += ms_between(e0, e1);
            times.walk[2] += ms_between(e1, e2);
            stats[4] = std::max(stats[4], n);
        }
        deliver();
        note_stats(ix, stats, times);
    });
}

int vs_set_diverse_depth(vs_index* ix, int32_t first, int32_t limit) {
    return guarded([&] {
        check_index(ix);
        const int kmax = KP_MAX * 4 / 5;
        if (first < 0 || limit < 0 || first > kmax || limit > kmax || (first > 0 && limit > 0 && first > limit))
            throw VsError(VS_ERR_ARG, "diverse depth: 1 <= first <= limit <= " + std::to_string(kmax) + " (0 = default)");
        ix->dv_first.store(first);
        ix->dv_limit.store(limit);
    });
}

int vs_diverse_last_stats(vs_index* ix, int64_t* out, int cap) {
    return guarded([&] {
        check_index(ix);
        if (!out || cap < 0) throw VsError(VS_ERR_ARG, "bad stats buffer");
        std::lock_guard<std::mutex> g(ix->dv_mu);
        for (int i = 0; i < std::min(cap, 5); ++i) out[i] = ix->dv_stats[i];
    });
}

int vs_diverse_last_times(vs_index* ix, double* out, int cap) {
    return guarded([&] {
        check_index(ix);
        if (!out || cap < 0) throw VsError(VS_ERR_ARG, "bad times buffer");
        std::lock_guard<std::mutex> g(ix->dv_mu);
        for (int i = 0; i < std::min(cap, 6); ++i) out[i] = ix->dv_times[i];
    });
}

}  // extern "C"

// vs_diverse_host.hip -- host side of the diversified search (include/vs.h "diversified search";
// kernel: vs_diverse.hip).
//
// The accepted list of a walk is prefix-stable, so a walk over the first L rows of a query's exact
// ranking that reaches k acceptances -- or that saw every member -- is the whole answer.  Tiers:
//   1  the exact top-L0 of every query (exact_lists, valid on the device), walked on the device;
//   2  the queries still short re-searched at 4 L, up to the limit, and walked again from scratch;
//      (tiers 1 and 2 are deepen_lists of vs_walk.h, shared with the grouped search)
//   3  what is left gets its whole ranking from the range machinery (range_block with an infinite
//      radius, which honours a selector), uploaded as a list and walked by the same kernel.
#include "vs_walk.h"

using namespace vs;

namespace {

// where one call's answers go (hidden / examined always exist here; the caller's may be null)
struct DvOut {
    int k;
    float* D;
    int64_t* I;
    std::vector<int32_t> hidden;
    std::vector<int64_t> examined;
    std::vector<int32_t> nacc;
    std::vector<float> rad;  // a walk's radii, gathered for the upload (one allocation per call)
};

// a walk's block for m queries, on the device and copied to the host:
// [examined int64 m | I int64 mk | D fp32 mk | hidden int32 mk | nacc int32 m | radius fp32 m]
struct DvBlock {
    int64_t *examined, *I;
    float* D;
    int32_t *hidden, *nacc;
    float* radius;
    size_t bytes;
};
DvBlock dv_block(const void* base, size_t m, size_t mk) {
    Carver c(base);  // (a braced list is evaluated left to right: the order of the members)
    DvBlock b{c.take<int64_t>(m), c.take<int64_t>(mk), c.take<float>(mk), c.take<int32_t>(mk), c.take<int32_t>(m),
              c.take<float>(m)};
    b.bytes = c.used;
    return b;
}

// the walk over m device lists [m][L]; query j's radius is radius[idx[j]], its answer goes to row idx[j]
// of out
void walk_lists(const vs_index* ix, Ctx* c, const int64_t* Id, const float* Dd, int64_t L, int64_t m, const float* radius,
                const int64_t* idx, DvOut& out, hipStream_t st, DevEvent* ev_done) {
    const int k = out.k;
    const size_t mk = (size_t)m * k;
    const int64_t qmax = 65536;  // workgroups of one launch
    const size_t bytes = dv_block(nullptr, m, mk).bytes;
    c->dv_out.ensure(bytes);
    const DvBlock dev = dv_block(c->dv_out.p, m, mk);
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
    out.rad.resize((size_t)m);
    for (int64_t j = 0; j < m; ++j) out.rad[(size_t)j] = radius[idx[j]];
    HIP_CHECK(hipMemcpyAsync(dev.radius, out.rad.data(), (size_t)m * sizeof(float), hipMemcpyHostToDevice, st));
    for (int64_t q0 = 0; q0 < m; q0 += qmax) {
        const int nq = (int)std::min(qmax, m - q0);
        a.I_in = Id + q0 * L;
        a.D_in = Dd + q0 * L;
        a.radius = dev.radius + q0;
        a.I = dev.I + q0 * k;
        a.D = dev.D + q0 * k;
        a.hidden = dev.hidden + q0 * k;
        a.nacc = dev.nacc + q0;
        a.examined = dev.examined + q0;
        HIP_CHECK(launch_diverse_walk(a, nq, st));
    }
    if (ev_done) HIP_CHECK(hipEventRecord(*ev_done, st));
    std::vector<uint8_t> h(bytes);
    HIP_CHECK(hipMemcpyAsync(h.data(), c->dv_out.p, bytes, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    const DvBlock host = dv_block(h.data(), m, mk);
    for (int64_t j = 0; j < m; ++j) {
        const int64_t g = idx[j];
        std::copy(host.I + j * k, host.I + (j + 1) * k, out.I + g * k);
        std::copy(host.D + j * k, host.D + (j + 1) * k, out.D + g * k);
        std::copy(host.hidden + j * k, host.hidden + (j + 1) * k, out.hidden.begin() + g * k);
        out.examined[(size_t)g] = host.examined[j];
        out.nacc[(size_t)g] = host.nacc[j];
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
        WalkTimes times;
        auto note = [&] { ix->dv.note(stats, 5, times.ms, 6); };
        if (nq == 0) {
            note();
            return;
        }
        if (!q || !radius || !D || !I) throw VsError(VS_ERR_ARG, "null host buffer");
        check_radii(radius, nq);
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
            note();
            return;
        }
        if (diverse_query_slots(ix->d) < 1)
            throw VsError(VS_ERR_ARG, "the walk holds a stored row as an fp64 query in LDS: d must be <= 14336");
        DeviceGuard dg(ix->device);
        const WalkState::Depth depth = ix->dv.resolve(std::max<int64_t>(4 * (int64_t)k, 64), K_MAX);
        CtxLease lease(ix, nullptr, true);
        Ctx* c = lease.c;
        hipStream_t st = c->stream;
        // ---- tiers 1 and 2: exact top-L lists, walked on the device; short of k acceptances goes deeper
        const Deepened dl = deepen_lists(
            ix, c, st, sel, members, depth.first, depth.limit, q, nq, times,
            [&](const StagedOut& so, int64_t L, int64_t m, const int64_t* idx, DevEvent* ev) {
                walk_lists(ix, c, so.Id, so.Dd, L, m, radius, idx, out, st, ev);
            },
            [&](int64_t g) { return out.nacc[(size_t)g] >= k; });
        stats[1] = dl.done[0];
        stats[2] = dl.done[1];
        stats[4] = dl.longest;
        // ---- tier 3: the whole ranking of each query still short -----------------------------------
        const float all = ix->metric == METRIC_IP ? -INFINITY : INFINITY;
        DevEvent e0, e1, e2;
        if (!dl.pending.empty()) {
            e0.create();
            e1.create();
            e2.create();
        }
        for (int64_t g : dl.pending) {
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
            walk_lists(ix, c, lI.as<int64_t>(), lD.as<float>(), n, 1, radius, &g, out, st, &e2);
            times.search(2) += ms_between(e0, e1);
            times.walk(2) += ms_between(e1, e2);
            stats[4] = std::max(stats[4], n);
        }
        deliver();
        note();
    });
}

int vs_set_diverse_depth(vs_index* ix, int32_t first, int32_t limit) {
    return guarded([&] {
        check_index(ix);
        ix->dv.set(first, limit, K_MAX, "diverse");
    });
}

int vs_diverse_last_stats(vs_index* ix, int64_t* out, int cap) {
    return guarded([&] {
        check_index(ix);
        copy_last(ix->dv.mu, ix->dv.stats, 5, out, cap, "stats");
    });
}

int vs_diverse_last_times(vs_index* ix, double* out, int cap) {
    return guarded([&] {
        check_index(ix);
        copy_last(ix->dv.mu, ix->dv.times, 6, out, cap, "times");
    });
}

}  // extern "C"

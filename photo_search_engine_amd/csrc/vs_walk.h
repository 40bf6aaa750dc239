// vs_walk.h -- what the jobs built as "an exact ranking, then a device walk over it" share on the host
// (vs_diverse_host.hip, vs_group_host.hip, vs_adjust_host.hip, vs_fuse_host.hip, vs_after_host.hip; DESIGN
// §7h-§7l): the
// driver of tiers 1 and 2, which deepens the lists until the walk is complete, the HIP-event stopwatch and
// the carving of a walk's output block.
#pragma once
#include "vs_index.h"

namespace vs {

inline double ms_between(const DevEvent& a, const DevEvent& b) {
    float ms = 0.0f;
    HIP_CHECK(hipEventElapsedTime(&ms, a, b));
    return (double)ms;
}

// A bump pointer over one block: one function per job takes a walk's arrays from it (8-byte types first)
// and is applied to the device base, to the host copy and, for the size alone, to a null base.
struct Carver {
    uintptr_t base;
    size_t used = 0;
    explicit Carver(const void* p) : base((uintptr_t)p) {}
    template <typename T>
    T* take(size_t n) {
        T* p = (T*)(base + used);
        used += n * sizeof(T);
        return p;
    }
};

// ms of a walk job's last call (WalkState::times): {search, walk} per tier; ms[6..] are the job's own
struct WalkTimes {
    double ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    double& search(int tier) { return ms[2 * tier]; }
    double& walk(int tier) { return ms[2 * tier + 1]; }
};

// a selector made by a call itself from a device bitmap over rows [0, n): only `bits` + `ids` are
// read by the filtered search's road; never exported
struct TempSel {
    vs_sel s;
    DevBuf bits, ids, tmp;
    // the bitmap is in bits (ceil(n / 64) words); at most cap rows are set
    void compact(vs_index* ix, int64_t n, int64_t cap, hipStream_t st) {
        const size_t cnt_off = (size_t)round_up(sel_compact_groups(n) * (int64_t)sizeof(unsigned), 8);
        tmp.ensure(cnt_off + 8);
        ids.ensure((size_t)std::max<int64_t>(cap, 1) * sizeof(uint32_t));
        unsigned long long* cnt_d = (unsigned long long*)((uint8_t*)tmp.p + cnt_off);
        HIP_CHECK(launch_sel_compact(bits.as<uint64_t>(), n, tmp.as<unsigned>(), ids.as<uint32_t>(), cap, cnt_d, st));
        unsigned long long cnt_h = 0;
        HIP_CHECK(hipMemcpyAsync(&cnt_h, cnt_d, sizeof(cnt_h), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if ((int64_t)cnt_h > cap) throw VsError(VS_ERR_INTERNAL, "walk: a compacted member set larger than its bound");
        s.ix = ix;
        s.gen = ix->reset_gen.load();
        s.device = ix->device;
        s.n_sel = n;
        s.m = (int64_t)cnt_h;
        s.bits = bits.as<uint64_t>();
        s.ids = ids.as<uint32_t>();
    }
    // the rows of [0, n_cov) that sel allows (null: all of them), for an object that covers fewer rows
    // than the selector or the index does
    void cover(vs_index* ix, const vs_sel* sel, int64_t n_cov, hipStream_t st) {
        const int64_t nwords = (n_cov + 63) / 64;
        bits.ensure((size_t)nwords * 8);
        if (sel) HIP_CHECK(hipMemcpyAsync(bits.p, sel->bits, (size_t)nwords * 8, hipMemcpyDeviceToDevice, st));
        else HIP_CHECK(hipMemsetAsync(bits.p, 0xFF, (size_t)nwords * 8, st));
        compact(ix, n_cov, sel ? std::min(sel->m, n_cov) : n_cov, st);
    }
    ~TempSel() {  // (the buffers free themselves; vs_sel_destroy must never see these pointers)
        s.bits = nullptr;
        s.ids = nullptr;
    }
};

struct Deepened {
    std::vector<int64_t> pending;  // the queries no list completed, ascending
    int64_t done[2] = {0, 0};      // queries complete after the first list, after a deeper one
    int64_t longest = 0;           // the longest list walked
};

// Tiers 1 and 2: the exact top-L lists of every query (L = first), walked on the device; the queries not
// done re-searched as one batch at 4 L, up to min(limit, members), and walked again from scratch.  Per
// staged chunk of m queries, walk(so, L, m, idx, &ev) walks the device lists so.Id / so.Dd [m][L], puts
// query j's answer where the caller's query idx[j] belongs and records ev behind its last kernel;
// done(query) says whether that answer is complete (a list that held every member always is).
// unit > 1 (the fused search): a caller's query is `unit` consecutive rows of q, searched as unit plain
// queries that always travel in one staged chunk -- so.Id / so.Dd are [m unit][L], and m, idx and done
// count the caller's queries.
template <typename Walk, typename Done>
Deepened deepen_lists(vs_index* ix, Ctx* c, hipStream_t st, const vs_sel* sel, int64_t members, int64_t first,
                      int64_t limit, const float* q, int64_t nq, WalkTimes& times, Walk&& walk, Done&& done,
                      int64_t unit = 1) {
    const int64_t qd = unit * ix->d;  // floats of one caller's query
    const int64_t Lmax = std::min<int64_t>(limit, members);
    int64_t L = std::min<int64_t>(first, Lmax);
    DevEvent e0(hipEventDefault), e1(hipEventDefault), e2(hipEventDefault);
    Deepened out;
    std::vector<int64_t>& pending = out.pending;
    std::vector<int64_t> next;
    pending.resize((size_t)nq);
    for (int64_t i = 0; i < nq; ++i) pending[(size_t)i] = i;
    std::vector<float> qsub;
    for (int tier = 0;; tier = 1) {
        const int64_t n = (int64_t)pending.size();
        const float* qp = q;
        if (tier) {  // the queries not done as one batch
            qsub.resize((size_t)n * qd);
            for (int64_t j = 0; j < n; ++j)
                std::copy(q + pending[(size_t)j] * qd, q + (pending[(size_t)j] + 1) * qd, qsub.begin() + j * qd);
            qp = qsub.data();
        }
        const int kk = (int)L;
        const SelPlan plan = sel ? sel_plan(ix, sel, n * unit, kk) : SelPlan{0, 0};
        const int64_t chunk = unit == 1 ? stage_chunk(ix, n, kk, !sel)
                                        : std::max<int64_t>(1, stage_chunk(ix, n * unit, kk, !sel) / unit);
        next.clear();
        for (int64_t q0 = 0; q0 < n; q0 += chunk) {
            const int64_t m = std::min(chunk, n - q0);
            const int64_t* idx = pending.data() + q0;
            HIP_CHECK(hipEventRecord(e0, st));
            stage_queries(ix, c, qp, q0 * unit, m * unit, st);
            const StagedOut so = exact_lists(ix, c, sel, plan, m * unit, kk, LISTS_DEVICE, st);
            HIP_CHECK(hipEventRecord(e1, st));
            walk(so, L, m, idx, &e2);
            times.search(tier) += ms_between(e0, e1);
            times.walk(tier) += ms_between(e1, e2);
            for (int64_t j = 0; j < m; ++j)
                if (!done(idx[j]) && L < members) next.push_back(idx[j]);
        }
        out.longest = L;
        out.done[tier] += n - (int64_t)next.size();
        pending.swap(next);
        if (pending.empty() || L >= Lmax) break;
        L = std::min<int64_t>(4 * L, Lmax);
    }
    return out;
}

}  // namespace vs

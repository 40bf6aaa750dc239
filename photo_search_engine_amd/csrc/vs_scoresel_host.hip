// vs_scoresel_host.hip -- host side of the score selectors (include/vs.h "score selectors"; kernels:
// vs_scoresel.hip over vs_range_scan.h).
//
// Queries are staged in blocks as the facet counts stage them; a block's answer is bits in a bitmap on the
// device.  ANY: every query of every block sets bits in the one accumulator (zeroed once).  ALL: each query
// of a block has a bitmap of its own (zeroed before the block), ANDed into the accumulator (preset to all
// ones) after the block.  The tiers are the range search's (range_tiers, vs_range_tiers.h) with the bit sink.
// The finish kernel applies negate, the members and the tail mask and counts; the ids are vs_sel_create's
// compaction of the result.  Nothing grows with the number of passing rows.
#include "vs_range_tiers.h"

using namespace vs;

namespace {

std::atomic<int64_t> g_scoresel_staging{64ll << 20};  // vs_set_scoresel_staging_bytes

struct BitsStats {
    int64_t m = 0, members = 0, tier = 0, rescanned = 0, blocks = 0;
    double ms[3] = {0, 0, 0};
};

void scoresel_note(vs_index* ix, const BitsStats& s) {
    std::lock_guard<std::mutex> g(ix->ss_mu);
    const int64_t st[5] = {s.m, s.members, s.tier, s.rescanned, s.blocks};
    std::copy(st, st + 5, ix->ss_stats);
    std::copy(s.ms, s.ms + 3, ix->ss_times);
}

using SelPtr = std::unique_ptr<vs_sel, void (*)(vs_sel*)>;

// an empty selector of the index over its n present rows
SelPtr new_sel(vs_index* ix, int64_t n) {
    SelPtr sel(new vs_sel(), vs_sel_destroy);
    sel->ix = ix;
    sel->gen = ix->reset_gen.load();
    sel->device = ix->device;
    sel->n_sel = n;
    return sel;
}

// sel->bits holds the result (tail zero) and *total_d its popcount: m, and the ascending ids as
// vs_sel_create makes them
void sel_take_ids(vs_index* ix, vs_sel* sel, const unsigned long long* total_d, hipStream_t st) {
    const int64_t n = sel->n_sel;
    unsigned long long total_h = 0;
    HIP_CHECK(hipMemcpyAsync(&total_h, total_d, sizeof(total_h), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    if ((int64_t)total_h > n) throw VsError(VS_ERR_INTERNAL, "score selector: more bits than rows");
    sel->m = (int64_t)total_h;
    HIP_CHECK(hipMalloc((void**)&sel->ids, (size_t)std::max<int64_t>(sel->m, 1) * sizeof(uint32_t)));
    DevBuf tmp;  // per-workgroup counts, then the device's total (8-byte aligned)
    const size_t cnt_off = (size_t)round_up(sel_compact_groups(n) * (int64_t)sizeof(unsigned), 8);
    tmp.ensure(cnt_off + 8);
    unsigned long long* cnt_d = (unsigned long long*)((uint8_t*)tmp.p + cnt_off);
    HIP_CHECK(launch_sel_compact(sel->bits, n, tmp.as<unsigned>(), sel->ids, sel->m, cnt_d, st));
    unsigned long long cnt_h = 0;
    HIP_CHECK(hipMemcpyAsync(&cnt_h, cnt_d, sizeof(cnt_h), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    if ((int64_t)cnt_h != sel->m) throw VsError(VS_ERR_INTERNAL, "selector compaction count mismatch");
}

// The queries are nq host vectors (q) or nq stored rows (ids, gathered on the device).  The caller holds
// the shared lock and has checked the index, the base, the mode and the host buffers.
void scoresel_run(vs_index* ix, const vs_sel* base, const float* q, const int64_t* ids, int64_t nq, const float* radius,
                  int32_t mode, int32_t negate, vs_sel** out) {
    const int64_t n = ix->ntotal;
    if (n >= 0xFFFFFFFFll) throw VsError(VS_ERR_ARG, "selector ids are 32-bit");
    BitsStats stt;
    stt.members = base ? base->m : n;
    SelPtr sel = new_sel(ix, n);
    if (n == 0) {  // no rows: the empty selector, as vs_sel_create makes it
        scoresel_note(ix, stt);
        *out = sel.release();
        return;
    }
    DeviceGuard dg(ix->device);
    CtxLease L(ix, nullptr, true);
    Ctx* c = L.c;
    hipStream_t st = c->stream;
    const bool all = mode == VS_SELQ_ALL;
    const int64_t nwords = (n + 63) / 64;
    const size_t wbytes = (size_t)nwords * 8;
    DevBuf acc, qbits, tot;  // (freed when the call returns)
    acc.ensure(wbytes);
    tot.ensure(8);
    HIP_CHECK(hipMemsetAsync(tot.p, 0, 8, st));
    // nq = 0 is decided here: ANY passes nothing, ALL everything (the presets of the two accumulators)
    HIP_CHECK(hipMemsetAsync(acc.p, all ? 0xFF : 0, wbytes, st));
    DevEvent e0(hipEventDefault), e1(hipEventDefault), e2(hipEventDefault);
    // (no members: the result is empty whatever passes, nothing is scored)
    if (nq > 0 && stt.members > 0) {
        const int range_mode = ix->range_mode.load();
        const int qb = all ? (int)std::max<int64_t>(1, std::min<int64_t>(MFMA_QB, g_scoresel_staging.load() / (8 * nwords)))
                           : MFMA_QB;
        if (all) qbits.ensure((size_t)std::min<int64_t>(qb, nq) * wbytes);
        const int64_t* ids_dev = nullptr;
        if (ids) {
            c->row_ids.ensure((size_t)nq * sizeof(int64_t));
            HIP_CHECK(hipMemcpyAsync(c->row_ids.p, ids, (size_t)nq * sizeof(int64_t), hipMemcpyHostToDevice, st));
            ids_dev = c->row_ids.as<int64_t>();
            c->qdev.ensure((size_t)std::min<int64_t>(qb, nq) * ix->d * sizeof(float));
        }
        c->rng_aux.ensure(sizeof(RangeAuxHead));
        RangeAuxHead h{};
        const int64_t nseq = base ? base->m : n;  // the sequence the scan's workgroups split
        for (int64_t q0 = 0; q0 < nq; q0 += qb) {
            const int nqb = (int)std::min<int64_t>(qb, nq - q0);
            ++stt.blocks;
            // (the previous block synchronised the stream after its copies from hq and h)
            if (ids) HIP_CHECK(launch_gather_rows(ix->dtype, ix->data, ids_dev + q0, nqb, ix->d, ix->dpad, c->qdev.as<float>(), st));
            else stage_queries(ix, c, q, q0, nqb, st);
            std::copy(radius + q0, radius + q0 + nqb, h.radius);
            HIP_CHECK(hipMemcpyAsync(c->rng_aux.p, h.radius, sizeof(h.radius), hipMemcpyHostToDevice, st));
            if (all) HIP_CHECK(hipMemsetAsync(qbits.p, 0, (size_t)nqb * wbytes, st));
            RangeArgs a = range_index_args(ix);
            a.n_valid = n;
            a.q = c->qdev.as<float>();
            a.nq = nqb;
            a.radius = range_aux_radius(c);
            const BitsArgs b{all ? qbits.as<unsigned long long>() : acc.as<unsigned long long>(), all ? nwords : 0};
            HIP_CHECK(hipEventRecord(e0, st));
            const RangeTiers t = range_tiers(
                ix, c, a, h, nqb, base ? base->ids : nullptr, base ? base->m : 0, nseq, nullptr, base, range_mode, st, e1,
                [&](const RangeArgs& r, const ScreenArgs& s, int ny) {
                    HIP_CHECK(launch_bits_refine(r, b, s.glist, s.gcnt, s.lcap, ny, st));
                },
                [&](const RangeArgs& r, int G, int qy, const uint32_t* sids, int64_t m) {
                    HIP_CHECK(launch_bits_scan(r, b, G, qy, sids, m, st));
                });
            if (t.screened) stt.tier = VS_RANGE_SCREEN;
            else if (stt.tier == 0) stt.tier = VS_RANGE_SCAN;
            stt.rescanned += t.rescanned;
            if (all) HIP_CHECK(launch_bits_fold(acc.as<uint64_t>(), qbits.as<uint64_t>(), nqb, nwords, st));
            HIP_CHECK(hipEventRecord(e2, st));
            HIP_CHECK(hipStreamSynchronize(st));
            stt.ms[0] += ms_between(e0, e1);
            stt.ms[1] += ms_between(e1, e2);
        }
    }
    HIP_CHECK(hipEventRecord(e0, st));
    HIP_CHECK(hipMalloc((void**)&sel->bits, wbytes));
    HIP_CHECK(launch_bits_finish(acc.as<uint64_t>(), base != nullptr, base ? base->bits : nullptr, base ? base->n_sel : 0,
                                 negate ? 1 : 0, n, sel->bits, tot.as<unsigned long long>(), st));
    sel_take_ids(ix, sel.get(), tot.as<unsigned long long>(), st);
    HIP_CHECK(hipEventRecord(e1, st));
    HIP_CHECK(hipStreamSynchronize(st));
    stt.ms[2] = ms_between(e0, e1);
    stt.m = sel->m;
    scoresel_note(ix, stt);
    *out = sel.release();
}

void check_selq(int64_t nq, int32_t mode, vs_sel** out) {
    if (!out) throw VsError(VS_ERR_ARG, "out is null");
    *out = nullptr;
    if (nq < 0) throw VsError(VS_ERR_ARG, "nq must be >= 0");
    if (mode != VS_SELQ_ANY && mode != VS_SELQ_ALL) throw VsError(VS_ERR_ARG, "mode must be VS_SELQ_ANY or VS_SELQ_ALL");
}

}  // namespace

extern "C" {

int vs_sel_from_range(vs_index* ix, const vs_sel* base, const float* q, int64_t nq, const float* radius, int32_t mode,
                      int32_t negate, vs_sel** out) {
    return guarded([&] {
        check_selq(nq, mode, out);
        check_index(ix);
        std::shared_lock<std::shared_mutex> lk(ix->rw);
        if (base) check_sel(ix, base);
        if (nq > 0) {
            if (!q || !radius) throw VsError(VS_ERR_ARG, "null host buffer");
            check_radii(radius, nq);
        }
        scoresel_run(ix, base, q, nullptr, nq, radius, mode, negate, out);
    });
}

int vs_sel_from_range_rows(vs_index* ix, const vs_sel* base, const int64_t* ids, int64_t n, const float* radius,
                           int32_t mode, int32_t negate, vs_sel** out) {
    return guarded([&] {
        check_selq(n, mode, out);
        check_index(ix);
        std::shared_lock<std::shared_mutex> lk(ix->rw);
        if (base) check_sel(ix, base);
        if (n > 0) {
            if (!ids || !radius) throw VsError(VS_ERR_ARG, "null host buffer");
            check_radii(radius, n);
            for (int64_t i = 0; i < n; ++i)
                if (ids[i] < 0 || ids[i] >= ix->ntotal)
                    throw VsError(VS_ERR_ARG, "row id " + std::to_string(ids[i]) + " (query " + std::to_string(i) +
                                                  ") is outside [0, ntotal = " + std::to_string(ix->ntotal) + ")");
        }
        scoresel_run(ix, base, nullptr, ids, n, radius, mode, negate, out);
    });
}

int vs_sel_combine(vs_index* ix, const vs_sel* a, const vs_sel* b, int32_t op, vs_sel** out) {
    return guarded([&] {
        if (!out) throw VsError(VS_ERR_ARG, "out is null");
        *out = nullptr;
        check_index(ix);
        if (op != VS_SEL_AND && op != VS_SEL_OR && op != VS_SEL_ANDNOT && op != VS_SEL_NOT)
            throw VsError(VS_ERR_ARG, "op must be VS_SEL_AND, VS_SEL_OR, VS_SEL_ANDNOT or VS_SEL_NOT");
        const bool unary = op == VS_SEL_NOT;
        if (unary ? b != nullptr : b == nullptr)
            throw VsError(VS_ERR_ARG, unary ? "VS_SEL_NOT takes one operand (b must be null)" : "the second operand is null");
        std::shared_lock<std::shared_mutex> lk(ix->rw);
        check_sel(ix, a);
        if (b) check_sel(ix, b);
        const int64_t n = unary ? a->n_sel : std::max(a->n_sel, b->n_sel);
        SelPtr sel = new_sel(ix, n);
        if (n == 0) {
            *out = sel.release();
            return;
        }
        DeviceGuard dg(ix->device);
        CtxLease L(ix, nullptr, true);
        hipStream_t st = L.c->stream;
        DevBuf tot;
        tot.ensure(8);
        HIP_CHECK(hipMemsetAsync(tot.p, 0, 8, st));
        HIP_CHECK(hipMalloc((void**)&sel->bits, (size_t)((n + 63) / 64) * 8));
        HIP_CHECK(launch_bits_op(a->bits, a->n_sel, b ? b->bits : nullptr, b ? b->n_sel : 0, op, n, sel->bits,
                                 tot.as<unsigned long long>(), st));
        sel_take_ids(ix, sel.get(), tot.as<unsigned long long>(), st);
        *out = sel.release();
    });
}

int vs_sel_bitmap(const vs_sel* sel, uint8_t* out, int64_t nbytes) {
    return guarded([&] {
        if (!sel) throw VsError(VS_ERR_ARG, "null selector");
        const int64_t need = (sel->n_sel + 7) / 8;
        if (nbytes < need || (need > 0 && !out))
            throw VsError(VS_ERR_ARG, "bitmap buffer too short: " + std::to_string(need) + " bytes cover the selector");
        if (need == 0) return;
        // (the selector owns its bitmap, complete since the call that made it returned: no lock, no stream)
        DeviceGuard dg(sel->device);
        // (a bitmap uploaded by vs_sel_create may carry the caller's bits past n_sel in its last byte)
        HIP_CHECK(hipMemcpy(out, sel->bits, (size_t)need, hipMemcpyDeviceToHost));
        if (sel->n_sel & 7) out[need - 1] &= (uint8_t)((1u << (sel->n_sel & 7)) - 1u);
    });
}

int vs_set_scoresel_staging_bytes(int64_t bytes) {
    return guarded([&] {
        if (bytes < 1) throw VsError(VS_ERR_ARG, "score selector staging bytes must be >= 1");
        g_scoresel_staging.store(bytes);
    });
}

int vs_scoresel_last_stats(vs_index* ix, int64_t* out, int cap) {
    return guarded([&] {
        check_index(ix);
        copy_last(ix->ss_mu, ix->ss_stats, 5, out, cap, "stats");
    });
}

int vs_scoresel_last_times(vs_index* ix, double* out, int cap) {
    return guarded([&] {
        check_index(ix);
        copy_last(ix->ss_mu, ix->ss_times, 3, out, cap, "times");
    });
}

}  // extern "C"

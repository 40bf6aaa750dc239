// vs_rows_host.hip -- host side of the queries taken from stored rows (include/vs.h "queries taken
// from stored rows"; kernels: vs_rows.hip, and the self-aware predicate of vs_range.hip).
//
// Both calls upload the ids once, gather each chunk's rows into the context's query buffer on the
// device (launch_gather_rows: the values vs_reconstruct returns) and continue exactly where
// vs_search / vs_search_sel / vs_range_search continue from their staged queries.
#include "vs_index.h"

using namespace vs;

namespace {

void check_self_mode(int mode, bool range) {
    if (mode == VS_SELF_KEEP || mode == VS_SELF_DROP || (range && mode == VS_SELF_ABOVE)) return;
    throw VsError(VS_ERR_ARG, range ? "self_mode must be VS_SELF_KEEP, VS_SELF_DROP or VS_SELF_ABOVE"
                                    : "self_mode must be VS_SELF_KEEP or VS_SELF_DROP");
}

// every id names a stored row (checked before anything is launched)
void check_row_ids(const vs_index* ix, const int64_t* ids, int64_t n) {
    for (int64_t i = 0; i < n; ++i)
        if (ids[i] < 0 || ids[i] >= ix->ntotal)
            throw VsError(VS_ERR_ARG, "row id " + std::to_string(ids[i]) + " (query " + std::to_string(i) +
                                          ") is outside [0, ntotal = " + std::to_string(ix->ntotal) + ")");
}

// the call's ids on the device, uploaded once (null = rows 0..n-1)
const int64_t* upload_row_ids(Ctx* c, const int64_t* ids, int64_t n, std::vector<int64_t>& iota, hipStream_t st) {
    if (!ids) {
        iota.resize((size_t)n);
        for (int64_t i = 0; i < n; ++i) iota[(size_t)i] = i;
        ids = iota.data();
    }
    c->row_ids.ensure((size_t)n * sizeof(int64_t));
    HIP_CHECK(hipMemcpyAsync(c->row_ids.p, ids, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, st));
    return c->row_ids.as<int64_t>();
}

// rows ids_dev[0, m) as fp32 queries in c->qdev
void gather_queries(const vs_index* ix, Ctx* c, const int64_t* ids_dev, int64_t m, hipStream_t st) {
    c->qdev.ensure((size_t)m * ix->d * sizeof(float));
    HIP_CHECK(launch_gather_rows(ix->dtype, ix->data, ids_dev, m, ix->d, ix->dpad, c->qdev.as<float>(), st));
}

}  // namespace

extern "C" {

int vs_search_rows(vs_index* ix, const vs_sel* sel, const int64_t* ids, int64_t n, int32_t k, int32_t self_mode,
                   float* D, int64_t* I) {
    return guarded([&] {
        check_index(ix);
        if (n < 0) throw VsError(VS_ERR_ARG, "n must be >= 0");
        if (k <= 0) throw VsError(VS_ERR_ARG, "k must be > 0");
        check_self_mode(self_mode, false);
        std::shared_lock<std::shared_mutex> lk(ix->rw);
        if (sel) check_sel(ix, sel);
        if (n == 0) return;
        if (!ids || !D || !I) throw VsError(VS_ERR_ARG, "null host buffer");
        check_row_ids(ix, ids, n);  // (an empty index holds no row to take a query from)
        DeviceGuard dg(ix->device);
        const bool drop = self_mode == VS_SELF_DROP;
        const float fillD = worst_score(ix);
        // DROP: one entry deeper, the row itself goes; k beyond the rows present is padded (as vs_search)
        const int kk = (int)std::min<int64_t>((int64_t)k + (drop ? 1 : 0), ix->ntotal);
        const int ko = std::min<int>(k, kk);  // entries the device writes per query
        check_k(kk);
        const SelPlan plan = sel ? sel_plan(ix, sel, n, kk) : SelPlan{0, 0};
        if (sel && sel->m == 0) {  // nothing allowed: all padding
            fill_padding(D, I, n * k, fillD);
            sel_note_stats(ix, sel, plan, 0);
            return;
        }
        CtxLease L(ix, nullptr, true);
        Ctx* c = L.c;
        hipStream_t st = c->stream;
        std::vector<int64_t> iota;
        const int64_t* ids_dev = upload_row_ids(c, ids, n, iota, st);
        const int64_t chunk = stage_chunk(ix, n, kk, !sel);
        int64_t redo = 0;
        for (int64_t q0 = 0; q0 < n; q0 += chunk) {
            const int64_t m = std::min(chunk, n - q0);
            gather_queries(ix, c, ids_dev + q0, m, st);
            const StagedOut so = exact_lists(ix, c, sel, plan, m, kk, drop ? LISTS_DEVICE : LISTS_HOST, st);
            redo += so.redo;
            if (!drop) {
                scatter_padded(so, q0, m, k, kk, fillD, D, I);
                continue;
            }
            // the lists without the rows themselves: [m][ko] on the device, then the same pinned block
            // (the kk-deep lists it held are no longer needed) and the caller's arrays
            c->row_out.ensure((size_t)m * ko * (sizeof(int64_t) + sizeof(float)));
            RowsTakeArgs t{};
            t.self = ids_dev + q0;
            t.I_in = so.Id;
            t.D_in = so.Dd;
            t.kk = kk;
            t.k = ko;
            t.metric = ix->metric;
            t.I = c->row_out.as<int64_t>();
            t.D = (float*)(t.I + (size_t)m * ko);
            HIP_CHECK(launch_rows_take(t, m, st));
            StagedOut to{};
            to.bytes = (size_t)m * ko * (sizeof(int64_t) + sizeof(float));
            to.Ik = (int64_t*)c->hout.p;
            to.Dk = (float*)(to.Ik + (size_t)m * ko);
            HIP_CHECK(hipMemcpyAsync(c->hout.p, c->row_out.p, to.bytes, hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            scatter_padded(to, q0, m, k, ko, fillD, D, I);
        }
        if (sel) sel_note_stats(ix, sel, plan, redo);
    });
}

int vs_range_search_rows(vs_index* ix, const vs_sel* sel, const int64_t* ids, int64_t n, const float* radius,
                         int32_t self_mode, int64_t max_total, vs_range_result** out) {
    return guarded([&] {
        if (!out) throw VsError(VS_ERR_ARG, "out is null");
        check_index(ix);
        if (n < 0) throw VsError(VS_ERR_ARG, "n must be >= 0");
        check_self_mode(self_mode, true);
        std::unique_ptr<vs_range_result> r(new vs_range_result());
        std::shared_lock<std::shared_mutex> lk(ix->rw);
        if (sel) check_sel(ix, sel);
        if (!ids && n != ix->ntotal)
            throw VsError(VS_ERR_ARG, "ids is null (rows 0..n-1): n must equal ntotal = " + std::to_string(ix->ntotal));
        r->lims.assign((size_t)n + 1, 0);
        RangeStats stt;
        if (n == 0) {
            range_note_stats(ix, stt);
            *out = r.release();
            return;
        }
        if (!radius) throw VsError(VS_ERR_ARG, "null host buffer");
        check_radii(radius, n);
        if (ids) check_row_ids(ix, ids, n);
        if (sel && sel->m == 0) {  // nothing to return
            range_note_stats(ix, stt);
            *out = r.release();
            return;
        }
        DeviceGuard dg(ix->device);
        CtxLease L(ix, nullptr, true);
        Ctx* c = L.c;
        hipStream_t st = c->stream;
        std::vector<int64_t> iota;
        const int64_t* ids_dev = upload_row_ids(c, ids, n, iota, st);
        const int64_t* ids_h = ids ? ids : iota.data();
        const int mode = ix->range_mode.load();
        int64_t counts[MFMA_QB];
        int64_t total = 0;
        for (int64_t q0 = 0; q0 < n; q0 += MFMA_QB) {
            const int nqb = (int)std::min<int64_t>(MFMA_QB, n - q0);
            gather_queries(ix, c, ids_dev + q0, nqb, st);
            RangeSelf self;
            if (self_mode != VS_SELF_KEEP) {
                self.ids = ids_dev + q0;
                self.mode = self_mode;
                // ABOVE: rows below the block's smallest id pass for none of its queries
                if (self_mode == VS_SELF_ABOVE && !sel) self.row0 = *std::min_element(ids_h + q0, ids_h + q0 + nqb);
            }
            const bool screen = mode != VS_RANGE_SCAN && range_screen_applies(ix, sel, nqb);
            const bool count_only = max_total > 0 && total > max_total;  // (the error names the count)
            range_block(ix, c, sel, c->qdev.as<float>(), nqb, radius + q0, screen, count_only, st, stt, counts, r.get(),
                        self);
            for (int j = 0; j < nqb; ++j) r->lims[(size_t)(q0 + j + 1)] = r->lims[(size_t)(q0 + j)] + counts[j];
            total = r->lims[(size_t)(q0 + nqb)];
        }
        stt.total = total;
        range_note_stats(ix, stt);
        if (max_total > 0 && total > max_total)
            throw VsError(VS_ERR_ARG, "range search found " + std::to_string(total) + " results, max_total is " +
                                          std::to_string(max_total));
        std::vector<double>().swap(r->S);
        *out = r.release();
    });
}

}  // extern "C"

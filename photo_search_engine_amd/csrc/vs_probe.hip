// vs_probe.hip -- diagnostics of the flat index: the screen probes, the K1 schedule switch, screen
// timing, the counters and the screen state.
#include "vs_index.h"

using namespace vs;

extern "C" {

// the shared setup of the screen probes: the packed query tile (zeroed on request), every threshold at
// +inf, the candidate buffers; the caller holds the lease and the read lock
static ScreenArgs probe_setup(vs_index* ix, Ctx* c, const float* q_dev, int64_t nq, bool i8, bool zero_queries,
                              hipStream_t st, std::vector<u64>& thr) {
    const int nqb = (int)nq;
    ScreenArgs a = mfma_screen_base(ix, i8);
    mfma_workspace(c, a);
    c->fails.ensure(2 * sizeof(int));
    if (i8) {
        c->qtile.ensure((size_t)MFMA_QB * ix->dpad8);
        c->qfac.ensure(sizeof(float2) * MFMA_QB);
        c->qeps.ensure(sizeof(float) * MFMA_QB);
        HIP_CHECK(launch_pack_qtile_i8(q_dev, nqb, ix->d, ix->dpad8, c->qtile.as<uint8_t>(), c->qfac.as<float2>(),
                                       c->qeps.as<float>(), ix->d_maxsq + 2, c->gcnt.as<int>(), c->drop.as<u64>(), st,
                                       c->fails.as<int>(), ix->metric == METRIC_L2 ? ix->d_maxsq : nullptr,
                                       gamma_of(ix->d)));
        a.qfac = c->qfac.as<float2>();
    } else {
        c->qtile.ensure((size_t)MFMA_QB * ix->dpad * ix->es);
        c->qinfo.ensure(sizeof(float) * 2 * MFMA_QB);
        HIP_CHECK(launch_pack_qtile(ix->dtype, q_dev, nqb, ix->d, ix->dpad, c->qtile.as<uint8_t>(),
                                    c->qinfo.as<float>(), c->gcnt.as<int>(), c->drop.as<u64>(), st));
    }
    if (zero_queries) HIP_CHECK(hipMemsetAsync(c->qtile.p, 0, c->qtile.bytes, st));
    // every query's threshold at the key of +inf: the bound test rejects every column, so the
    // launch is the K loop + the epilogue's bound test with no survivor to insert
    c->thr0.ensure(sizeof(u64) * MFMA_QB);
    thr.assign(MFMA_QB, 0xFF80000000000000ull);
    HIP_CHECK(hipMemcpyAsync(c->thr0.p, thr.data(), sizeof(u64) * MFMA_QB, hipMemcpyHostToDevice, st));
    a.thr0 = c->thr0.as<u64>();
    return a;
}

// a probe waits for its stream before it leaves, on every path: its events, stamp buffer and host
// threshold array are let go only when nothing queued can still touch them, and a launch error is
// reported after that wait
struct StreamDrain {
    hipStream_t st;
    ~StreamDrain() { (void)hipStreamSynchronize(st); }
};

static void probe_checks(vs_index* ix, const float* q_dev, int64_t nq, int32_t screen, const void* out) {
    check_index(ix);
    if (!q_dev || !out || nq <= GEMV_NQ_MAX || nq > MFMA_QB) throw VsError(VS_ERR_ARG, "screen probe: 9..256 device queries");
    const bool i8 = screen == VS_SCREEN_I8;
    if (i8 && (ix->screen != VS_SCREEN_I8 || !ix->data8 || ix->i8_res || !i8_direct_ok(ix->dpad8)))
        throw VsError(VS_ERR_ARG, "screen probe: the int8 probe needs the int8 direct screen (no group residuals)");
    if (!i8 && !((ix->dtype == DT_BF16 || ix->dtype == DT_F16) && d16_direct_ok(ix->dpad)))
        throw VsError(VS_ERR_ARG, "screen probe: the native probe needs bf16 / f16 rows of the direct screen");
    if (ix->ntotal == 0) throw VsError(VS_ERR_ARG, "index is empty");
}

int vs_screen_probe(vs_index* ix, const float* q_dev, int64_t nq, int32_t screen, int32_t zero_queries, void* stream,
                    float* ms) {
    return guarded([&] {
        check_index(ix);
        probe_checks(ix, q_dev, nq, screen, ms);
        std::shared_lock<std::shared_mutex> lk(ix->rw);
        DeviceGuard dg(ix->device);
        const bool i8 = screen == VS_SCREEN_I8;
        hipStream_t st = (hipStream_t)stream;
        CtxLease L(ix, st, false);
        Ctx* c = L.c;
        const int nqb = (int)nq;
        StreamDrain drain{st};
        std::vector<u64> thr;
        ScreenArgs a = probe_setup(ix, c, q_dev, nq, i8, zero_queries != 0, st, thr);
        // kProbeReps launches back to back (the cadence of the timed steps, no host gap between
        // them), each between its own events; the fastest one is reported
        constexpr int kProbeReps = 5;
        DevEvent ev[kProbeReps + 1];
        for (DevEvent& e : ev) e.create();
        HIP_CHECK(hipEventRecord(ev[0], st));
        for (int i = 0; i < kProbeReps; ++i) {
            HIP_CHECK(launch_screen_mfma(i8 ? DT_I8 : ix->dtype, a, c->qtile.as<uint8_t>(), nqb, st));
            HIP_CHECK(hipEventRecord(ev[i + 1], st));
        }
        HIP_CHECK(hipStreamSynchronize(st));
        float best = 0.0f;
        for (int i = 0; i < kProbeReps; ++i) {
            float t = 0.0f;
            HIP_CHECK(hipEventElapsedTime(&t, ev[i], ev[i + 1]));
            if (i == 0 || t < best) best = t;
        }
        *ms = best;
    });
}

int vs_k1_probe(vs_index* ix, const float* q_dev, int64_t nq, int32_t screen, int32_t variant, int32_t zero_queries,
                int32_t reps, void* stream, float* ms, unsigned long long* stamps, int32_t* G_out) {
    return guarded([&] {
        check_index(ix);
        probe_checks(ix, q_dev, nq, screen, ms);
        if (!stamps || !G_out || reps < 1 || reps > 64) throw VsError(VS_ERR_ARG, "vs_k1_probe: 1..64 reps, stamps, G_out");
        std::shared_lock<std::shared_mutex> lk(ix->rw);
        DeviceGuard dg(ix->device);
        const bool i8 = screen == VS_SCREEN_I8;
        if (ix->metric != METRIC_IP) throw VsError(VS_ERR_ARG, "vs_k1_probe: inner-product indexes");
        hipStream_t st = (hipStream_t)stream;
        CtxLease L(ix, st, false);
        Ctx* c = L.c;
        const int nqb = (int)nq;
        DevBuf sbuf;  // (declared before the drain: freed only once the stream is idle)
        StreamDrain drain{st};
        std::vector<u64> thr;
        ScreenArgs a = probe_setup(ix, c, q_dev, nq, i8, zero_queries != 0, st, thr);
        sbuf.ensure(sizeof(unsigned long long) * 4 * (size_t)a.G * (size_t)reps);
        std::vector<DevEvent> ev((size_t)reps + 1);
        for (DevEvent& e : ev) e.create();
        HIP_CHECK(hipEventRecord(ev[0], st));
        for (int r = 0; r < reps; ++r) {
            a.stamps = sbuf.as<unsigned long long>() + (size_t)r * a.G * 4;
            if (launch_k1_probe(variant, i8 ? DT_I8 : ix->dtype, a, c->qtile.as<uint8_t>(), nqb, st) != hipSuccess)
                throw VsError(VS_ERR_ARG, "vs_k1_probe: variant not available for this screen / index");
            HIP_CHECK(hipEventRecord(ev[(size_t)r + 1], st));
        }
        HIP_CHECK(hipStreamSynchronize(st));
        for (int r = 0; r < reps; ++r) HIP_CHECK(hipEventElapsedTime(&ms[r], ev[(size_t)r], ev[(size_t)r + 1]));
        HIP_CHECK(hipMemcpy(stamps, sbuf.p, sizeof(unsigned long long) * 4 * (size_t)a.G * (size_t)reps,
                            hipMemcpyDeviceToHost));
        *G_out = a.G;
    });
}

int vs_set_k1_schedule(int32_t schedule) {
    return guarded([&] {
        if (schedule != 0 && schedule != 1) throw VsError(VS_ERR_ARG, "K1 schedule: 0 or 1");
        set_k1_schedule(schedule);
    });
}
int vs_k1_schedule(void) { return k1_schedule(); }

int vs_set_i8_query_credit(int32_t on) {
    return guarded([&] {
        if (on != 0 && on != 1) throw VsError(VS_ERR_ARG, "int8 query credit: 0 or 1");
        set_i8_query_credit(on);
    });
}
int vs_i8_query_credit(void) { return i8_query_credit(); }

int vs_set_timing(vs_index* ix, int enable) {
    return guarded([&] {
        check_index(ix);
        ix->timing.store(enable != 0);
    });
}

int vs_timing_fetch(vs_index* ix, float* ms, int cap, int* kernel_kind) {
    int count = 0;
    int rc = guarded([&] {
        check_index(ix);
        DeviceGuard dg(ix->device);
        std::lock_guard<std::mutex> g(ix->tmtx);
        for (auto& pr : ix->tev) {
            HIP_CHECK(hipEventSynchronize(pr.second));
            float t = 0.0f;
            HIP_CHECK(hipEventElapsedTime(&t, pr.first, pr.second));
            if (ms && count < cap) ms[count] = t;
            ++count;
        }
        ix->tev.clear();
        if (kernel_kind) *kernel_kind = ix->last_kernel_kind;
    });
    return rc == VS_OK ? std::min(count, cap) : rc;
}

int vs_screen_state(vs_index* ix, double* out, int cap) {
    return guarded([&] {
        check_index(ix);
        if (!out || cap < 0) throw VsError(VS_ERR_ARG, "null output");
        DeviceGuard dg(ix->device);
        HIP_CHECK(hipDeviceSynchronize());
        unsigned bits[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        HIP_CHECK(hipMemcpy(bits, ix->d_maxsq, sizeof(bits), hipMemcpyDeviceToHost));
        auto f = [&](int i) {
            float v;
            std::memcpy(&v, &bits[i], 4);
            return (double)v;
        };
        std::lock_guard<std::mutex> g(ix->h_mu);
        health_poll(ix);
        const double v[VS_SCREEN_STATE_N] = {(double)ix->screen, ix->i8_res ? 1.0 : 0.0, (double)bits[6], f(5), f(2),
                                             f(3), (double)ix->i8_log2, (double)ix->i8_route, (double)ix->seed_log2};
        for (int i = 0; i < cap && i < VS_SCREEN_STATE_N; ++i) out[i] = v[i];
    });
}

int64_t vs_full_scan_count(vs_index* ix) {
    int64_t v = -1;
    int rc = guarded([&] {
        check_index(ix);
        DeviceGuard dg(ix->device);
        HIP_CHECK(hipDeviceSynchronize());
        unsigned u = 0;
        HIP_CHECK(hipMemcpy(&u, ix->d_unres, sizeof(unsigned), hipMemcpyDeviceToHost));
        v = u;
    });
    return rc == VS_OK ? v : rc;
}

int64_t vs_refine_rows_count(vs_index* ix) {
    int64_t v = -1;
    int rc = guarded([&] {
        check_index(ix);
        DeviceGuard dg(ix->device);
        HIP_CHECK(hipDeviceSynchronize());
        unsigned long long u = 0;
        HIP_CHECK(hipMemcpy(&u, ix->d_maxsq + IX_REFINE_ROWS, sizeof(u), hipMemcpyDeviceToHost));
        v = (int64_t)u;
    });
    return rc == VS_OK ? v : rc;
}

int64_t vs_uncertified_count(vs_index* ix) {
    int64_t v = -1;
    int rc = guarded([&] {
        check_index(ix);
        DeviceGuard dg(ix->device);
        HIP_CHECK(hipDeviceSynchronize());
        unsigned u = 0;
        HIP_CHECK(hipMemcpy(&u, ix->d_uncert, sizeof(unsigned), hipMemcpyDeviceToHost));
        v = u;
    });
    return rc == VS_OK ? v : rc;
}

}  // extern "C"

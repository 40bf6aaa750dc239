// vs_store.hip -- the flat index object of libvs: creation, HBM residency and capacity, the int8
// screen copy, row ingest and export, the context pool, the plain accessors.
//
// Replaces faiss.IndexFlatIP/IndexFlatL2 behind the product's vector store (construct, add,
// reconstruct, ntotal, clear).
#include "vs_index.h"

using namespace vs;

vs::FlatView vs::flat_view(vs_index* ix) {
    return {ix->data, ix->d, ix->dpad, ix->dtype, ix->metric, ix->device, ix->ntotal};
}
std::shared_mutex& vs::flat_lock(vs_index* ix) { return ix->rw; }

namespace vs {

Ctx* acquire_ctx(vs_index* ix) {
    std::lock_guard<std::mutex> g(ix->pool_mtx);
    if (!ix->pool_free.empty()) {
        Ctx* c = ix->pool_free.back();
        ix->pool_free.pop_back();
        return c;
    }
    Ctx* c = new Ctx();
    ix->pool_all.push_back(c);  // owned by the pool from here on (freed by vs_destroy)
    HIP_CHECK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    HIP_CHECK(hipEventCreateWithFlags(&c->idle, hipEventDisableTiming));
    return c;
}

void release_ctx(vs_index* ix, Ctx* c) {
    std::lock_guard<std::mutex> g(ix->pool_mtx);
    ix->pool_free.push_back(c);
}


}  // namespace vs

namespace {

void ensure_capacity_i8(vs_index* ix);

// exact: allocate exactly rows_needed (vs_reserve) instead of growing by 1.5x
void ensure_capacity(vs_index* ix, int64_t rows_needed, bool exact = false) {
    const int64_t want = round_up(rows_needed, TR);
    if (want <= ix->cap_rows) return;
    int64_t ncap = exact ? want : std::max(want, ix->cap_rows + ix->cap_rows / 2);
    ncap = round_up(ncap, TR);
    const int64_t tb = tile_bytes(ix->dpad, ix->dtype);
    uint8_t* nd = nullptr;
    float* ns = nullptr;
    HIP_CHECK(hipMalloc(&nd, (size_t)(ncap / TR) * tb));
    hipError_t e = hipMalloc(&ns, (size_t)ncap * sizeof(float));
    if (e != hipSuccess) {
        hipFree(nd);
        HIP_CHECK(e);
    }
    HIP_CHECK(hipMemsetAsync(nd, 0, (size_t)(ncap / TR) * tb, ix->own));
    HIP_CHECK(hipMemsetAsync(ns, 0, (size_t)ncap * sizeof(float), ix->own));
    if (ix->data && ix->ntotal > 0) {
        const int64_t used_tiles = (ix->ntotal + TR - 1) / TR;
        HIP_CHECK(hipMemcpyAsync(nd, ix->data, (size_t)used_tiles * tb, hipMemcpyDeviceToDevice, ix->own));
        HIP_CHECK(hipMemcpyAsync(ns, ix->sqn, (size_t)ix->ntotal * sizeof(float), hipMemcpyDeviceToDevice, ix->own));
    }
    HIP_CHECK(hipStreamSynchronize(ix->own));
    if (ix->data) hipFree(ix->data);
    if (ix->sqn) hipFree(ix->sqn);
    ix->data = nd;
    ix->sqn = ns;
    ix->cap_rows = ncap;
    ensure_capacity_i8(ix);
}

void free_i8(vs_index* ix) {
    if (ix->data8) (void)hipFree(ix->data8);
    if (ix->rsb) (void)hipFree(ix->rsb);
    if (ix->gmean) (void)hipFree(ix->gmean);
    ix->data8 = nullptr;
    ix->rsb = nullptr;
    ix->gmean = nullptr;
    ix->cap8 = 0;
    ix->gcap = 0;
    ix->i8_res = false;
}

// group residuals apply to inner-product indexes whose int8 main pass is the direct form
bool i8_groups_apply(const vs_index* ix) { return ix->metric == METRIC_IP && i8_direct_ok(ix->dpad8); }

// grow the int8 screen copy to ix->cap_rows rows (device copy of the rows present; the old and new
// arrays coexist only for the copy, as for the primary rows)
void ensure_capacity_i8(vs_index* ix) {
    if (ix->screen != VS_SCREEN_I8 || ix->cap8 >= ix->cap_rows) return;
    const int64_t ncap = ix->cap_rows;
    const size_t tb8 = (size_t)TR * ix->dpad8;
    uint8_t* nd = nullptr;
    uint32_t* nr = nullptr;
    uint16_t* ng = nullptr;
    const int64_t gcap = i8_groups_apply(ix) ? (ncap + I8_GROUP_ROWS - 1) / I8_GROUP_ROWS : 0;
    hipError_t e = hipMalloc(&nd, (size_t)(ncap / TR) * tb8);
    if (e == hipSuccess) e = hipMalloc(&nr, (size_t)ncap * sizeof(uint32_t));
    if (e == hipSuccess && gcap) e = hipMalloc(&ng, (size_t)gcap * ix->dpad8 * sizeof(uint16_t));
    if (e != hipSuccess) {
        if (nd) hipFree(nd);
        if (nr) hipFree(nr);
        HIP_CHECK(e);
    }
    if (ix->data8 && ix->ntotal > 0) {
        const int64_t used_tiles = (ix->ntotal + TR - 1) / TR;
        HIP_CHECK(hipMemcpyAsync(nd, ix->data8, (size_t)used_tiles * tb8, hipMemcpyDeviceToDevice, ix->own));
        HIP_CHECK(hipMemcpyAsync(nr, ix->rsb, (size_t)ix->ntotal * sizeof(uint32_t), hipMemcpyDeviceToDevice, ix->own));
        if (ng && ix->gmean) {
            const int64_t used_groups = (ix->ntotal + I8_GROUP_ROWS - 1) / I8_GROUP_ROWS;
            HIP_CHECK(hipMemcpyAsync(ng, ix->gmean, (size_t)used_groups * ix->dpad8 * sizeof(uint16_t),
                                     hipMemcpyDeviceToDevice, ix->own));
        }
    }
    HIP_CHECK(hipStreamSynchronize(ix->own));
    const bool res = ix->i8_res;
    free_i8(ix);
    ix->data8 = nd;
    ix->rsb = nr;
    ix->gmean = ng;
    ix->gcap = gcap;
    ix->i8_res = res;
    ix->cap8 = ncap;
}

}  // namespace

// int8 screen copy of rows [r0, r0 + n) once they are packed (stream-ordered after the pack).  With
// group residuals, the groups the rows fall in get their means (re)computed over every row they
// hold now, and their rows are (re)quantised from the group's first row.
void vs::quantize_rows(vs_index* ix, int64_t r0, int64_t n, hipStream_t st) {
    if (ix->screen != VS_SCREEN_I8 || n <= 0) return;
    if (ix->gmean) {
        // rows already searchable get new codes, bounds and group means: searches still queued on
        // other streams (device-API callers return before their kernels run) must finish first, or
        // one could read a row's new code with the old <mu_g, q> and its key would no longer bound
        // the score (the exclusive lock only orders host calls; vs_set_screen syncs likewise)
        if (r0 % I8_GROUP_ROWS != 0) HIP_CHECK(hipDeviceSynchronize());
        const int64_t g0 = r0 / I8_GROUP_ROWS, g1 = (r0 + n + I8_GROUP_ROWS - 1) / I8_GROUP_ROWS;
        HIP_CHECK(launch_group_means(ix->dtype, ix->data, ix->dpad, ix->d, g0, g1 - g0, r0 + n, ix->dpad8, ix->gmean,
                                     ix->d_maxsq + 5, st));
        n += r0 - g0 * I8_GROUP_ROWS;
        r0 = g0 * I8_GROUP_ROWS;
    }
    HIP_CHECK(launch_quant_rows(ix->dtype, ix->data, ix->dpad, r0, n, ix->d, ix->data8, ix->dpad8, ix->rsb,
                                ix->d_maxsq + 2, st, ix->gmean));
}

// the int8 copy's statistics before every row is quantised anew: the maxima at 0, the minimum of
// ||s c|| at +inf (stream-ordered on st)
void vs::reset_i8_stats(vs_index* ix, hipStream_t st) {
    HIP_CHECK(hipMemsetAsync(ix->d_maxsq + 2, 0, 2 * sizeof(unsigned), st));
    HIP_CHECK(hipMemsetAsync(ix->d_maxsq + 5, 0, 3 * sizeof(unsigned), st));
    HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)(ix->d_maxsq + 2 + I8_MIN_XH), (int)F32_INF_BITS, 1, st));
}

void vs::refresh_maxsq(vs_index* ix) {
    unsigned bits[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    HIP_CHECK(hipMemcpyAsync(bits, ix->d_maxsq, sizeof(bits), hipMemcpyDeviceToHost, ix->own));
    HIP_CHECK(hipStreamSynchronize(ix->own));
    std::memcpy(&ix->maxsq, &bits[0], 4);
    std::memcpy(&ix->i8_bmax, &bits[7], 4);  // int8 copy: the largest ||x - s c|| (GEMV keys' error)
    ix->i8_res = ix->gmean != nullptr && bits[6] != 0;  // some group coded against its mean
}

unsigned* vs::full_scan_counter(vs_index* ix) { return ix->d_unres; }
uint64_t vs::flat_generation(vs_index* ix) { return ix->reset_gen.load(); }

void vs::truncate_rows(vs_index* ix, int64_t n) {
    check_index(ix);
    std::unique_lock<std::shared_mutex> lk(ix->rw);
    if (n < 0 || n > ix->ntotal) throw VsError(VS_ERR_ARG, "truncate_rows: n outside [0, ntotal]");
    ix->ntotal = n;  // the rows behind stay allocated and are never read again (appends overwrite them)
}


int64_t vs::stream_chunk_rows(int d) { return std::max<int64_t>(1, (int64_t)(32 << 20) / ((int64_t)d * 4)); }

// Double-buffered host -> HBM ingest: chunk c is filled on the host (memcpy, file read) into pinned
// buffer c&1 while the copy engine and k_pack_rows still work on chunk c-1.  A pinned buffer is
// refilled only after the event recorded behind its previous pack has fired.
void vs::add_rows_host(vs_index* ix, int64_t n, const std::function<void(int64_t, int64_t, float*)>& fill) {
    check_index(ix);
    std::unique_lock<std::shared_mutex> lk(ix->rw);
    DeviceGuard dg(ix->device);
    if (ix->ntotal + n > (int64_t)0xFFFFFFF0LL) throw VsError(VS_ERR_ARG, "shard exceeds 2^32 rows");
    ensure_capacity(ix, ix->ntotal + n);
    const int64_t rpc = stream_chunk_rows(ix->d);
    const size_t cbytes = (size_t)std::min(n, rpc) * ix->d * sizeof(float);
    ix->pin.ensure(cbytes);
    ix->stage[0].ensure(cbytes);
    ix->stage[1].ensure(cbytes);
    try {
        for (int64_t c = 0, r0 = 0; r0 < n; ++c, r0 += rpc) {
            const int b = (int)(c & 1);
            const int64_t m = std::min(rpc, n - r0);
            if (c >= 2) HIP_CHECK(hipEventSynchronize(ix->pin.done[b]));
            fill(r0, m, ix->pin.host(b));
            HIP_CHECK(hipMemcpyAsync(ix->stage[b].p, ix->pin.host(b), (size_t)m * ix->d * sizeof(float),
                                     hipMemcpyHostToDevice, ix->own));
            HIP_CHECK(launch_pack_rows(ix->dtype, ix->stage[b].as<float>(), m, ix->d, ix->dpad, ix->data,
                                       ix->ntotal + r0, ix->sqn, ix->d_maxsq, ix->own));
            HIP_CHECK(hipEventRecord(ix->pin.done[b], ix->own));
        }
        quantize_rows(ix, ix->ntotal, n, ix->own);
        HIP_CHECK(hipStreamSynchronize(ix->own));
    } catch (...) {
        (void)hipStreamSynchronize(ix->own);  // the pinned chunks may still be in flight
        throw;                                // ntotal unchanged: the packed rows stay invisible
    }
    ix->ntotal += n;
    refresh_maxsq(ix);
}

// Double-buffered HBM -> host export: chunk c is unpacked and copied into pinned buffer c&1 while
// the host consumes chunk c-1 (memcpy out, file write).
void vs::read_rows_host(vs_index* ix, int64_t i0, int64_t n,
                        const std::function<void(int64_t, int64_t, const float*)>& sink) {
    check_index(ix);
    std::shared_lock<std::shared_mutex> lk(ix->rw);
    if (i0 < 0 || n < 0 || i0 + n > ix->ntotal) throw VsError(VS_ERR_ARG, "reconstruct range out of bounds");
    if (n == 0) return;
    DeviceGuard dg(ix->device);
    CtxLease L(ix, nullptr, true);
    Ctx* c = L.c;
    const int64_t rpc = stream_chunk_rows(ix->d);
    const size_t cbytes = (size_t)std::min(n, rpc) * ix->d * sizeof(float);
    c->pin.ensure(cbytes);
    c->rows[0].ensure(cbytes);
    c->rows[1].ensure(cbytes);
    const int64_t nchunks = (n + rpc - 1) / rpc;
    auto enqueue = [&](int64_t ci) {
        const int b = (int)(ci & 1);
        const int64_t r0 = ci * rpc, m = std::min(rpc, n - r0);
        HIP_CHECK(launch_unpack_rows(ix->dtype, ix->data, i0 + r0, m, ix->d, ix->dpad, c->rows[b].as<float>(),
                                     c->stream));
        HIP_CHECK(hipMemcpyAsync(c->pin.host(b), c->rows[b].p, (size_t)m * ix->d * sizeof(float),
                                 hipMemcpyDeviceToHost, c->stream));
        HIP_CHECK(hipEventRecord(c->pin.done[b], c->stream));
    };
    try {
        enqueue(0);
        for (int64_t ci = 0; ci < nchunks; ++ci) {
            if (ci + 1 < nchunks) enqueue(ci + 1);  // pinned buffer (ci+1)&1 was drained at ci-1
            const int b = (int)(ci & 1);
            HIP_CHECK(hipEventSynchronize(c->pin.done[b]));
            const int64_t r0 = ci * rpc;
            sink(r0, std::min(rpc, n - r0), c->pin.host(b));
        }
    } catch (...) {
        (void)hipStreamSynchronize(c->stream);
        throw;
    }
}

extern "C" {

int vs_create(int d, int metric, int dtype, int device, vs_index** out) {
    return guarded([&] {
        if (!out) throw VsError(VS_ERR_ARG, "out is null");
        *out = nullptr;
        if (d <= 0) throw VsError(VS_ERR_ARG, "dimension must be > 0");
        if (metric != VS_METRIC_IP && metric != VS_METRIC_L2) throw VsError(VS_ERR_ARG, "metric must be IP(0) or L2(1)");
        if (dtype < VS_DTYPE_F32 || dtype > VS_DTYPE_F16) throw VsError(VS_ERR_ARG, "dtype must be 0 (f32), 1 (bf16), 2 (f16)");
        int ndev = 0;
        hipError_t e = hipGetDeviceCount(&ndev);
        if (e != hipSuccess || ndev <= 0) throw VsError(VS_ERR_DEVICE, "no HIP device available (libvs needs an MI355X)");
        if (device < 0 || device >= ndev) throw VsError(VS_ERR_ARG, "device ordinal out of range");
        DeviceGuard dg(device);
        hipDeviceProp_t prop;
        HIP_CHECK(hipGetDeviceProperties(&prop, device));
        if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
            throw VsError(VS_ERR_DEVICE, std::string("libvs is built for gfx950, device is ") + prop.gcnArchName);
        vs_index* ix = new vs_index();
        ix->d = d;
        // >= 2 K-steps per tile: the MFMA screen's deferred compaction check runs on the K-step
        // after a tile's epilogue, so a one-step tile would never compact its candidate buffers
        ix->dpad = pad_dim(d, dtype);
        ix->metric = metric;
        ix->dtype = dtype;
        ix->device = device;
        ix->es = es_of(dtype);
        ix->num_cu = prop.multiProcessorCount;
        try {
            HIP_CHECK(hipStreamCreateWithFlags(&ix->own, hipStreamNonBlocking));
            // [0] max ||x||^2, [1] uncertified counter, [2..3] int8 screen maxima (fp32 bits),
            // [4] full-scan counter (vs_full_scan_count), [5..6] group residuals (max ||mu_g||,
            // groups with a mean), [7] max ||x - s c|| of the int8 codes, [8] min ||s c|| (+inf
            // until a row is quantised), [10..11] rows scored by k_refine_wide (vs_internal.h IX_WORDS)
            HIP_CHECK(hipMalloc(&ix->d_maxsq, sizeof(unsigned) * IX_WORDS));
            HIP_CHECK(hipMemset(ix->d_maxsq, 0, sizeof(unsigned) * IX_WORDS));
            ix->d_uncert = ix->d_maxsq + 1;
            ix->d_unres = ix->d_maxsq + 4;
            reset_i8_stats(ix, ix->own);
            HIP_CHECK(hipStreamSynchronize(ix->own));
        } catch (...) {
            delete ix;
            throw;
        }
        *out = ix;
    });
}

void vs_destroy(vs_index* ix) {
    if (!ix) return;
    {  // (the index's own buffers and events go with it, inside this scope: its device is current)
        DeviceGuard dg(ix->device);
        hipDeviceSynchronize();
        for (Ctx* c : ix->pool_all) delete c;
        if (ix->data) hipFree(ix->data);
        if (ix->sqn) hipFree(ix->sqn);
        if (ix->d_maxsq) hipFree(ix->d_maxsq);
        free_i8(ix);
        if (ix->own) hipStreamDestroy(ix->own);
        if (ix->h_ev) hipEventDestroy(ix->h_ev);
        if (ix->h_fails) hipHostFree(ix->h_fails);
        delete ix;
    }
}

int vs_reset(vs_index* ix) {
    return guarded([&] {
        check_index(ix);
        std::unique_lock<std::shared_mutex> lk(ix->rw);
        DeviceGuard dg(ix->device);
        ix->ntotal = 0;
        ix->reset_gen.fetch_add(1);  // (selectors made before this are stale)
        ix->maxsq = 0.0f;
        ix->i8_bmax = 0.0f;
        ix->i8_res = false;
        HIP_CHECK(hipMemsetAsync(ix->d_maxsq, 0, sizeof(unsigned), ix->own));
        reset_i8_stats(ix, ix->own);
        HIP_CHECK(hipStreamSynchronize(ix->own));
    });
}

int vs_add(vs_index* ix, const float* x, int64_t n) {
    return guarded([&] {
        check_index(ix);
        if (n < 0) throw VsError(VS_ERR_ARG, "n must be >= 0");
        if (n == 0) return;
        if (!x) throw VsError(VS_ERR_ARG, "x is null");
        const int64_t d = ix->d;
        add_rows_host(ix, n, [&](int64_t r0, int64_t m, float* dst) {
            std::memcpy(dst, x + r0 * d, (size_t)(m * d) * sizeof(float));
        });
    });
}

int vs_add_device(vs_index* ix, const float* x_dev, int64_t n, void* stream) {
    return guarded([&] {
        check_index(ix);
        if (n < 0) throw VsError(VS_ERR_ARG, "n must be >= 0");
        if (n == 0) return;
        if (!x_dev) throw VsError(VS_ERR_ARG, "x_dev is null");
        std::unique_lock<std::shared_mutex> lk(ix->rw);
        DeviceGuard dg(ix->device);
        if (ix->ntotal + n > (int64_t)0xFFFFFFF0LL) throw VsError(VS_ERR_ARG, "shard exceeds 2^32 rows");
        ensure_capacity(ix, ix->ntotal + n);
        // NULL is the legacy default stream (torch's default stream handle is 0), never the
        // index's private non-blocking stream: that one is unordered with the caller's producers
        hipStream_t st = (hipStream_t)stream;
        HIP_CHECK(launch_pack_rows(ix->dtype, x_dev, n, ix->d, ix->dpad, ix->data, ix->ntotal, ix->sqn, ix->d_maxsq, st));
        quantize_rows(ix, ix->ntotal, n, st);
        HIP_CHECK(hipStreamSynchronize(st));
        ix->ntotal += n;
        refresh_maxsq(ix);
    });
}

int vs_reserve(vs_index* ix, int64_t n) {
    return guarded([&] {
        check_index(ix);
        if (n < 0) throw VsError(VS_ERR_ARG, "n must be >= 0");
        std::unique_lock<std::shared_mutex> lk(ix->rw);
        DeviceGuard dg(ix->device);
        if (ix->ntotal + n > (int64_t)0xFFFFFFF0LL) throw VsError(VS_ERR_ARG, "shard exceeds 2^32 rows");
        ensure_capacity(ix, ix->ntotal + n, true);
    });
}

int64_t vs_capacity(const vs_index* ix) { return ix ? ix->cap_rows : -1; }

int vs_add_synthetic(vs_index* ix, uint64_t seed, int64_t global_row0, int64_t n, int normalize) {
    return guarded([&] {
        check_index(ix);
        if (n < 0 || global_row0 < 0) throw VsError(VS_ERR_ARG, "bad synthetic range");
        if (n == 0) return;
        std::unique_lock<std::shared_mutex> lk(ix->rw);
        DeviceGuard dg(ix->device);
        if (ix->ntotal + n > (int64_t)0xFFFFFFF0LL) throw VsError(VS_ERR_ARG, "shard exceeds 2^32 rows");
        ensure_capacity(ix, ix->ntotal + n);
        HIP_CHECK(launch_synth_rows(ix->dtype, seed, global_row0, n, ix->d, ix->dpad, ix->data, ix->ntotal, normalize,
                                    ix->sqn, ix->d_maxsq, ix->own));
        quantize_rows(ix, ix->ntotal, n, ix->own);
        HIP_CHECK(hipStreamSynchronize(ix->own));
        ix->ntotal += n;
        refresh_maxsq(ix);
    });
}

int vs_synthesize(int device, uint64_t seed, int64_t global_row0, int64_t n, int d, int normalize, int dtype,
                  float* out_dev, void* stream) {
    return guarded([&] {
        if (n < 0 || d <= 0 || global_row0 < 0) throw VsError(VS_ERR_ARG, "bad synthetic shape");
        if (dtype < VS_DTYPE_F32 || dtype > VS_DTYPE_F16) throw VsError(VS_ERR_ARG, "bad dtype");
        if (n == 0) return;
        if (!out_dev) throw VsError(VS_ERR_ARG, "out_dev is null");
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) throw VsError(VS_ERR_DEVICE, "no HIP device available");
        DeviceGuard dg(device);
        HIP_CHECK(launch_synth_f32(dtype, seed, global_row0, n, d, normalize, out_dev, (hipStream_t)stream));
    });
}

int vs_reconstruct_n(vs_index* ix, int64_t i0, int64_t n, float* out) {
    return guarded([&] {
        check_index(ix);
        if (n == 0) return;
        if (!out) throw VsError(VS_ERR_ARG, "out is null");
        const int64_t d = ix->d;
        read_rows_host(ix, i0, n, [&](int64_t r0, int64_t m, const float* src) {
            std::memcpy(out + r0 * d, src, (size_t)(m * d) * sizeof(float));
        });
    });
}

int vs_reconstruct(vs_index* ix, int64_t id, float* out) { return vs_reconstruct_n(ix, id, 1, out); }

int64_t vs_ntotal(const vs_index* ix) { return ix ? ix->ntotal : -1; }
int vs_dim(const vs_index* ix) { return ix ? ix->d : -1; }
int vs_metric(const vs_index* ix) { return ix ? ix->metric : -1; }
int vs_dtype(const vs_index* ix) { return ix ? ix->dtype : -1; }
int vs_device(const vs_index* ix) { return ix ? ix->device : -1; }

int vs_set_screen(vs_index* ix, int screen) {
    return guarded([&] {
        check_index(ix);
        if (screen != VS_SCREEN_NATIVE && screen != VS_SCREEN_I8) throw VsError(VS_ERR_ARG, "screen must be 0 (native) or 1 (int8)");
        std::unique_lock<std::shared_mutex> lk(ix->rw);
        DeviceGuard dg(ix->device);
        if (screen == ix->screen) return;
        if (screen == VS_SCREEN_NATIVE) {
            HIP_CHECK(hipDeviceSynchronize());  // searches in flight may still read the int8 copy
            free_i8(ix);
            ix->screen = VS_SCREEN_NATIVE;
            return;
        }
        ix->screen = VS_SCREEN_I8;
        ix->dpad8 = (int)std::max<int64_t>(round_up(ix->d, 64), 128);  // >= 2 K-steps per tile (see dpad)
        try {
            reset_i8_stats(ix, ix->own);
            ensure_capacity_i8(ix);
            quantize_rows(ix, 0, ix->ntotal, ix->own);
            HIP_CHECK(hipStreamSynchronize(ix->own));
            refresh_maxsq(ix);
        } catch (...) {
            free_i8(ix);
            ix->screen = VS_SCREEN_NATIVE;
            throw;
        }
    });
}

int vs_screen(const vs_index* ix) { return ix ? ix->screen : -1; }

int vs_set_scan_limit(vs_index* ix, int64_t bytes) {
    return guarded([&] {
        check_index(ix);
        if (bytes < 0) throw VsError(VS_ERR_ARG, "scan limit must be >= 0");
        ix->scan_limit.store(bytes);
    });
}

int64_t vs_host_staging_bytes(vs_index* ix) {
    if (!ix) return -1;
    std::lock_guard<std::mutex> g(ix->pool_mtx);
    int64_t b = 0;
    for (const Ctx* c : ix->pool_all) b += (int64_t)(c->hq.bytes + c->hout.bytes);
    return b;
}

int64_t vs_screen_copy_bytes(vs_index* ix) {
    if (!ix) return -1;
    if (!ix->data8) return 0;
    const int64_t rows = ix->cap8;
    return (rows / TR) * (int64_t)TR * ix->dpad8 + rows * (int64_t)sizeof(uint32_t) +
           ix->gcap * ix->dpad8 * (int64_t)sizeof(uint16_t);
}

}  // extern "C"

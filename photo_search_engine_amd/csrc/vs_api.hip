// vs_api.hip -- C ABI of libvs (include/vs.h): the error channel, the version and the entry points
// that belong to no index (the rest: vs_store.hip, vs_search.hip, vs_sel_host.hip,
// vs_range_host.hip, vs_probe.hip).
#include "vs_index.h"

using namespace vs;

namespace {
thread_local std::string g_err;
}  // namespace

void vs::set_last_error(const std::string& msg) { g_err = msg; }

extern "C" {

const char* vs_last_error(void) { return g_err.c_str(); }
const char* vs_version(void) { return "libvs 0.1 (gfx950)"; }

int vs_merge_shards_device(int metric, const double* S_in, const int64_t* I_in, int32_t in_stride, int G, int64_t nq,
                           int32_t k, double* S_out, int64_t* I_out, float* D_out, void* stream) {
    return guarded([&] {
        if (G <= 0 || G > 64) throw VsError(VS_ERR_ARG, "G must be in [1, 64]");
        if (k <= 0 || nq < 0) throw VsError(VS_ERR_ARG, "bad k / nq");
        if (in_stride < 1) throw VsError(VS_ERR_ARG, "in_stride must be >= 1");
        if (nq == 0) return;
        HIP_CHECK(launch_merge_shards(metric, S_in, I_in, G, nq, k, S_out, I_out, D_out, (hipStream_t)stream,
                                      in_stride));
    });
}

int vs_seed_select_device(int device, const float* maxima, int32_t M, int64_t nq, int32_t rank, uint64_t* thr,
                          void* stream) {
    return guarded([&] {
        if (M <= 0 || M > 8192 || rank < 1 || nq < 0) throw VsError(VS_ERR_ARG, "bad M / rank / nq");
        if (nq == 0) return;
        DeviceGuard dg(device);
        HIP_CHECK(launch_seed_select(maxima, M, (int)nq, rank, (u64*)thr, (hipStream_t)stream));
    });
}

int64_t vs_device_bytes_live(void) { return g_dev_bytes_live.load(std::memory_order_relaxed); }

}  // extern "C"
